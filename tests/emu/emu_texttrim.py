"""ctypes wrapper of tests/emu/libcfemu_texttrim.so — the CPU harness of the record and pack passes with a trim and a skip
(TEST ONLY; see emu_texttrim.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PAD = 128
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_texttrim64.so" if wave64 else "libcfemu_texttrim.so")
    src = os.path.join(HERE, "emu_texttrim.cpp")
    deps = [src] + [os.path.join(ROOT, "centrifuge_amd/csrc", f) for f in ("cf_platform.hpp", "cf_textio.hpp")]

    def fresh():
        return os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps)
    if fresh():
        return lib
    # built under a lock and moved into place: several test processes (pytest -n) may get here at once
    import fcntl
    with open(lib + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if fresh():
            return lib
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-fno-strict-aliasing"] + (["-DCF_EMU_WAVE64=1"] if wave64 else []) + ["-o", tmp, src])
        os.replace(tmp, lib)
    return lib


class TrimIn(C.Structure):
    """EmuTrimIn of emu_texttrim.cpp"""
    _fields_ = [("text", C.c_void_p), ("nBytes", C.c_uint64), ("posCap", C.c_uint64),
                ("format", C.c_uint32), ("globalSeed", C.c_uint32), ("recCap", C.c_uint32), ("textBase", C.c_uint32), ("stride", C.c_uint32),
                ("mate", C.c_uint32), ("trim5", C.c_uint32), ("trim3", C.c_uint32), ("skip", C.c_uint32), ("pad", C.c_uint32),
                ("rlen", C.c_void_p), ("seeds", C.c_void_p), ("seqOff", C.c_void_p), ("idOff", C.c_void_p), ("idLen", C.c_void_p), ("qualOff", C.c_void_p),
                ("status", C.c_void_p)]


def lib(wave64=False):
    if wave64 not in _libs:
        L = C.CDLL(build(wave64))
        L.emu_trim_parse.restype = C.c_uint32
        L.emu_trim_parse.argtypes = [C.POINTER(TrimIn)]
        L.emu_trim_pack.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        L.emu_trim_wave_lanes.restype = C.c_int
        assert L.emu_trim_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


def upload(blocks, fmt, trim5=0, trim3=0, skip=0, max_reads=0, seed=0, wave64=False, rec_cap=None):
    """What cf_batch_upload_text does with one block (or the two blocks of mates), the slot's trim and skip set, and the plan stage's
    pack pass.  -> (flags, None) when the device refuses, else (0, dict): n_reads, n_bases, max_len (the sums as the device reports
    them), buf (the buffer the places count in, bytes) and per read of the batch rlen, seeds, seqOff, idOff, idLen, qualOff (FASTQ),
    bases / nmask (lists of the read's packed words)"""
    L = lib(wave64)
    stride = len(blocks)
    at, total = [], 0
    for t in blocks:
        at.append(total)
        total += (len(t) + 63) // 64 * 64 + PAD
    buf = np.zeros(total + 64, dtype=np.uint8)
    for t, a in zip(blocks, at):
        buf[a:a + len(t)] = np.frombuffer(t, dtype=np.uint8)
    n_marks = [t.count(b">") if fmt == 0 else t.count(b"\n") // 4 for t in blocks]
    cap = rec_cap if rec_cap is not None else max(n_marks) + 16
    arr = {k: np.full(stride * (cap + 80), 0xdeadbeef, dtype=np.uint32) for k in ("rlen", "seeds", "seqOff", "idOff", "idLen", "qualOff")}
    status = np.zeros(4, dtype=np.uint64)
    n_rec = []
    for m, (t, a) in enumerate(zip(blocks, at)):
        x = TrimIn()
        x.text, x.nBytes, x.posCap = buf.ctypes.data + a, len(t), cap if fmt == 0 else 4 * cap
        x.format, x.globalSeed, x.recCap, x.textBase, x.stride, x.mate = fmt, seed, cap, a, stride, m
        x.trim5, x.trim3, x.skip = trim5, trim3, min(skip, 2 ** 32 - 1)
        for k, v in arr.items():
            setattr(x, k, v.ctypes.data if (k != "qualOff" or fmt == 1) else None)
        x.status = status.ctypes.data
        n_rec.append(L.emu_trim_parse(C.byref(x)))
    flags = int(status[3])
    if flags:
        return flags, None
    assert len(set(n_rec)) == 1, "the blocks of mates hold different numbers of records"
    nq = n_rec[0] - min(n_rec[0], skip)                       # (cf_device.hip uploadTextBlocks: the skip first, then max_reads)
    if max_reads and nq > max_reads:
        nq = max_reads
    n = nq * stride
    out = {k: v[:n].copy() for k, v in arr.items()}
    # nothing behind the reads that are kept (but for those max_reads cuts off) is written
    written = (n_rec[0] - min(n_rec[0], skip)) * stride
    for k, v in arr.items():
        if k != "qualOff" or fmt == 1:
            assert (v[written:] == 0xdeadbeef).all(), k
    out.update(n_reads=n, n_words=int(status[0]), n_bases=int(status[1]), max_len=int(status[2]), buf=bytes(buf), n_rec=n_rec[0])
    words = (out["rlen"].astype(np.uint64) + 31) // 32
    nw = int(words.sum())
    bases, nmask = np.zeros(nw + 1, dtype=np.uint64), np.zeros(nw + 1, dtype=np.uint32)
    L.emu_trim_pack(buf.ctypes.data, n, out["seqOff"].ctypes.data, out["rlen"].ctypes.data, bases.ctypes.data, nmask.ctypes.data)
    woff = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
    out["bases"] = [bases[woff[r]:woff[r + 1]].tolist() for r in range(n)]
    out["nmask"] = [nmask[woff[r]:woff[r + 1]].tolist() for r in range(n)]
    return 0, out
