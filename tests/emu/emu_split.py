"""ctypes wrapper of tests/emu/libcfemu_split.so — the CPU harness of the read splitter (TEST ONLY; see emu_split.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_split64.so" if wave64 else "libcfemu_split.so")
    src = os.path.join(HERE, "emu_split.cpp")
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


class SplitIn(C.Structure):
    """EmuSplitIn of emu_split.cpp"""
    _fields_ = [("text", C.c_void_p), ("idOff", C.c_void_p), ("idLen", C.c_void_p), ("rlen", C.c_void_p), ("qualOff", C.c_void_p),
                ("bases", C.c_void_p), ("nmask", C.c_void_p), ("qinfo", C.c_void_p),
                ("nQueries", C.c_uint32), ("paired", C.c_uint32), ("sinks", C.c_uint32), ("pad", C.c_uint32),
                ("out", C.c_void_p * 4), ("outCap", C.c_uint64 * 4), ("bytes", C.c_uint64 * 4), ("records", C.c_uint64 * 4), ("sized", C.c_uint32 * 4)]


def lib(wave64=False):
    if wave64 not in _libs:
        L = C.CDLL(build(wave64))
        L.emu_split_run.restype = C.c_int
        L.emu_split_run.argtypes = [C.POINTER(SplitIn)]
        L.emu_split_wave_lanes.restype = C.c_int
        assert L.emu_split_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


UNWRITTEN = 0x5A       # what a byte of a sink's room holds that no body wrote


def split(batch, sinks, wave64=False, cap=1 << 22):
    """batch: the block and what the kernels left per read / query (dict of arrays, as emu_cols.format_rows takes it); sinks: the
    CF_SPLIT_* bits.  -> per sink (text, bytes the size pass counted, records, sized)"""
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
    x = SplitIn()
    x.text = arr(np.frombuffer(batch["text"] + bytes(256), dtype=np.uint8), np.uint8)
    x.idOff, x.idLen, x.rlen = arr(batch["idOff"], np.uint32), arr(batch["idLen"], np.uint32), arr(batch["rlen"], np.uint32)
    x.qualOff = arr(batch.get("qualOff"), np.uint32)
    x.bases, x.nmask = arr(np.append(batch["bases"], np.zeros(2, np.uint64)), np.uint64), arr(np.append(batch["nmask"], np.zeros(2, np.uint32)), np.uint32)
    x.qinfo = arr(batch["qinfo"], np.uint8)
    x.nQueries, x.paired, x.sinks = len(batch["qinfo"]), int(batch["paired"]), int(sinks)
    caps = [int(cap)] * 4 if np.isscalar(cap) else [int(c) for c in cap]
    outs = [np.zeros(c + 16, dtype=np.uint8) for c in caps]
    for s in range(4):
        x.out[s] = outs[s].ctypes.data
        x.outCap[s] = caps[s]
    bad = L.emu_split_run(C.byref(x))
    assert not bad, "the write pass wrote outside a sink's room"
    return [(outs[s][:min(x.bytes[s], caps[s])].tobytes(), int(x.bytes[s]), int(x.records[s]), bool(x.sized[s])) for s in range(4)]
