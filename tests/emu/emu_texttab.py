"""ctypes wrapper of tests/emu/libcfemu_texttab.so — the CPU harness of the marker, record and pack passes over a tabbed block
(TEST ONLY; see emu_texttab.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PAD = 128
TAB5, TAB6 = 2, 3
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_texttab64.so" if wave64 else "libcfemu_texttab.so")
    src = os.path.join(HERE, "emu_texttab.cpp")
    deps = [src] + [os.path.join(ROOT, "centrifuge_amd/csrc", f) for f in ("cf_platform.hpp", "cf_textio.hpp")]

    def fresh():
        return os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps)
    if fresh():
        return lib
    import fcntl
    with open(lib + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if fresh():
            return lib
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                               "-fno-strict-aliasing"] + (["-DCF_EMU_WAVE64=1"] if wave64 else []) + ["-o", tmp, src])
        os.replace(tmp, lib)
    return lib


class TabIn(C.Structure):
    """EmuTabIn of emu_texttab.cpp"""
    _fields_ = [("text", C.c_void_p), ("nBytes", C.c_uint64), ("posCap", C.c_uint64),
                ("format", C.c_uint32), ("globalSeed", C.c_uint32), ("recCap", C.c_uint32), ("textBase", C.c_uint32), ("stride", C.c_uint32),
                ("mate", C.c_uint32), ("trim5", C.c_uint32), ("trim3", C.c_uint32), ("skip", C.c_uint32), ("pad", C.c_uint32),
                ("rlen", C.c_void_p), ("seeds", C.c_void_p), ("seqOff", C.c_void_p), ("idOff", C.c_void_p), ("idLen", C.c_void_p), ("qualOff", C.c_void_p),
                ("status", C.c_void_p)]


def lib(wave64=False):
    if wave64 not in _libs:
        L = C.CDLL(build(wave64))
        L.emu_tab_parse.restype = C.c_uint32
        L.emu_tab_parse.argtypes = [C.POINTER(TabIn)]
        L.emu_tab_pack.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        L.emu_tab_wave_lanes.restype = C.c_int
        assert L.emu_tab_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


def upload(text, fmt, trim5=0, trim3=0, skip=0, max_reads=0, seed=0, wave64=False):
    """What cf_batch_upload_text does with one tabbed block, and the plan stage's pack pass.  -> (flags, None) when the device
    refuses, else (0, dict): paired, n_reads, n_bases, max_len, buf and per read rlen, seeds, seqOff, idOff, idLen, qualOff, bases,
    nmask"""
    L = lib(wave64)
    buf = np.zeros((len(text) + 63) // 64 * 64 + PAD + 64, dtype=np.uint8)
    buf[:len(text)] = np.frombuffer(text, dtype=np.uint8)
    cap = text.count(b"\n") + 16
    arr = {k: np.full(2 * (cap + 80), 0xdeadbeef, dtype=np.uint32) for k in ("rlen", "seeds", "seqOff", "idOff", "idLen", "qualOff")}
    status = np.zeros(5, dtype=np.uint64)
    x = TabIn()
    x.text, x.nBytes, x.posCap = buf.ctypes.data, len(text), 4 * cap
    x.format, x.globalSeed, x.recCap, x.textBase, x.stride, x.mate = fmt, seed, cap, 0, 1, 0
    x.trim5, x.trim3, x.skip = trim5, trim3, min(skip, 2 ** 32 - 1)
    for k, v in arr.items():
        setattr(x, k, v.ctypes.data)
    x.status = status.ctypes.data
    n_rec = L.emu_tab_parse(C.byref(x))
    flags = int(status[3])
    if flags:
        return flags, None
    per = 2 if status[4] else 1
    kept = n_rec - min(n_rec, skip)
    nq = min(kept, max_reads) if max_reads else kept
    n = nq * per
    out = {k: v[:n].copy() for k, v in arr.items()}
    for k, v in arr.items():                                  # nothing behind the reads that are kept is written
        assert (v[kept * per:] == 0xdeadbeef).all(), k
    out.update(paired=bool(status[4]), n_reads=n, n_words=int(status[0]), n_bases=int(status[1]), max_len=int(status[2]), buf=bytes(buf), n_rec=n_rec)
    words = (out["rlen"].astype(np.uint64) + 31) // 32
    nw = int(words.sum())
    bases, nmask = np.zeros(nw + 1, dtype=np.uint64), np.zeros(nw + 1, dtype=np.uint32)
    L.emu_tab_pack(buf.ctypes.data, n, out["seqOff"].ctypes.data, out["rlen"].ctypes.data, bases.ctypes.data, nmask.ctypes.data)
    woff = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
    out["bases"] = [bases[woff[r]:woff[r + 1]].tolist() for r in range(n)]
    out["nmask"] = [nmask[woff[r]:woff[r + 1]].tolist() for r in range(n)]
    return 0, out
