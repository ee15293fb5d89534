"""ctypes wrapper of tests/emu/libcfemu_cols.so — the CPU harness of the column-program formatter (TEST ONLY; see emu_cols.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_cols64.so" if wave64 else "libcfemu_cols.so")
    src = os.path.join(HERE, "emu_cols.cpp")
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


class ColsIn(C.Structure):
    """EmuColsIn of emu_cols.cpp"""
    _fields_ = [("text", C.c_void_p), ("idOff", C.c_void_p), ("idLen", C.c_void_p), ("rlen", C.c_void_p), ("qualOff", C.c_void_p),
                ("bases", C.c_void_p), ("nmask", C.c_void_p), ("rows", C.c_void_p), ("qinfo", C.c_void_p), ("score2", C.c_void_p), ("maxScore", C.c_void_p),
                ("nQueries", C.c_uint32), ("paired", C.c_uint32),
                ("strs", C.c_void_p), ("uidOff", C.c_void_p), ("rankOff", C.c_void_p), ("taxOff", C.c_void_p), ("taxLeaf", C.c_void_p),
                ("nRefs", C.c_uint32), ("nTaxa", C.c_uint32), ("idxZero", C.c_uint32), ("nCols", C.c_uint32),
                ("taxStrs", C.c_void_p), ("trankOff", C.c_void_p), ("tnameOff", C.c_void_p), ("cols", C.c_void_p),
                ("defaultBodies", C.c_uint32), ("tuplesCap", C.c_uint32),
                ("out", C.c_void_p), ("outCap", C.c_uint64), ("single", C.c_void_p), ("tuples", C.c_void_p), ("tupleWords", C.c_void_p), ("size", C.c_void_p)]


def lib(wave64=False):
    if wave64 not in _libs:
        L = C.CDLL(build(wave64))
        L.emu_cols_format.restype = C.c_uint64
        L.emu_cols_format.argtypes = [C.POINTER(ColsIn)]
        L.emu_cols_wave_lanes.restype = C.c_int
        L.emu_cols_lds_bytes.restype = C.c_uint32
        assert L.emu_cols_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


UNWRITTEN = 0x5A       # what a byte of the room holds that no body wrote


def format_rows(world, batch, cols, wave64=False, default_bodies=False, out_cap=None):
    """world: the string tables (dict of arrays), batch: the block and what the kernels left per read / query (dict of arrays);
    cols: column codes.  -> text (bytes), singles (u64 per taxon), tuples (u32 words)"""
    text, _, n, single, tuples, _ = format_full(world, batch, cols, wave64, default_bodies, out_cap)
    return text[:n], single, tuples


def format_full(world, batch, cols, wave64=False, default_bodies=False, out_cap=None, tuples_cap=None):
    """as format_rows, with what capi.debug_format gives for the device -> the room's out_cap bytes (UNWRITTEN where nothing was
    written), the bytes per query, the bytes the size pass summed, singles, the tuple words that fit tuples_cap, the words all
    tuples need"""
    L = lib(wave64)
    keep = []

    def arr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dtype=dt)
        keep.append(a)
        return a.ctypes.data
    nq = len(batch["qinfo"])
    x = ColsIn()
    x.text = arr(np.frombuffer(batch["text"] + bytes(256), dtype=np.uint8), np.uint8)
    x.idOff, x.idLen, x.rlen = arr(batch["idOff"], np.uint32), arr(batch["idLen"], np.uint32), arr(batch["rlen"], np.uint32)
    x.qualOff = arr(batch.get("qualOff"), np.uint32)
    x.bases, x.nmask = arr(np.append(batch["bases"], np.zeros(2, np.uint64)), np.uint64), arr(np.append(batch["nmask"], np.zeros(2, np.uint32)), np.uint32)
    x.rows, x.qinfo = arr(batch["rows"], np.uint32), arr(batch["qinfo"], np.uint8)
    x.score2, x.maxScore = arr(batch["score2"], np.uint32), arr(batch["maxScore"], np.uint32)
    x.nQueries, x.paired = nq, int(batch["paired"])
    x.strs = arr(np.frombuffer(world["strs"] + bytes(16), dtype=np.uint8), np.uint8)
    x.uidOff, x.rankOff, x.taxOff, x.taxLeaf = arr(world["uidOff"], np.uint32), arr(world["rankOff"], np.uint32), arr(world["taxOff"], np.uint32), arr(world["taxLeaf"], np.uint8)
    x.nRefs, x.nTaxa, x.idxZero = world["nRefs"], world["nTaxa"], world["idxZero"]
    x.taxStrs = arr(np.frombuffer(world["taxStrs"] + bytes(16), dtype=np.uint8), np.uint8)
    x.trankOff, x.tnameOff = arr(world["trankOff"], np.uint32), arr(world["tnameOff"], np.uint32)
    x.cols, x.nCols = arr(np.asarray(cols, dtype=np.uint8), np.uint8), len(cols)
    x.defaultBodies = int(default_bodies)
    cap = int(out_cap if out_cap is not None else batch["outCap"])
    out = np.zeros(cap + 16, dtype=np.uint8)
    single = np.zeros(world["nTaxa"] + 1, dtype=np.uint64)
    tcap = nq * 64 + 16 if tuples_cap is None else int(tuples_cap)
    tuples = np.full(tcap + 16, 0x5A5A5A5A, dtype=np.uint32)
    size = np.zeros(nq + 1, dtype=np.uint32)
    x.size = size.ctypes.data
    tw = C.c_uint32(0)
    x.tuplesCap, x.out, x.outCap, x.single, x.tuples, x.tupleWords = tcap, out.ctypes.data, cap, single.ctypes.data, tuples.ctypes.data, C.addressof(tw)
    n = L.emu_cols_format(C.byref(x))
    assert n != 2 ** 64 - 1, "more columns than the kernels take"
    assert n != 2 ** 64 - 2, "the write pass wrote past the room it was given"
    assert np.all(tuples[tcap:] == 0x5A5A5A5A), "the write pass wrote a tuple behind the room it was given"
    return out[:cap].tobytes(), size[:nq].copy(), int(n), single, tuples[:min(tw.value, tcap)].copy(), int(tw.value)
