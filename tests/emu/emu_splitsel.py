"""ctypes wrapper of tests/emu/libcfemu_splitsel.so — the CPU harness of the read splitter's size pass by a selection of taxa
(TEST ONLY; see emu_splitsel.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu.emu_split import SplitIn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_splitsel64.so" if wave64 else "libcfemu_splitsel.so")
    src = os.path.join(HERE, "emu_splitsel.cpp")
    deps = [src, os.path.join(HERE, "emu_split.cpp")] + [os.path.join(ROOT, "centrifuge_amd/csrc", f) for f in ("cf_platform.hpp", "cf_textio.hpp")]

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


def lib(wave64=False):
    if wave64 not in _libs:
        L = C.CDLL(build(wave64))
        L.emu_splitsel_run.restype = C.c_int
        L.emu_splitsel_run.argtypes = [C.POINTER(SplitIn), C.c_void_p, C.c_void_p, C.c_uint32]
        L.emu_split_wave_lanes.restype = C.c_int
        assert L.emu_split_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


def split_taxa(batch, rows, mask, sinks, wave64=False, cap=1 << 22):
    """batch, sinks, cap and the result: as emu_split.split; rows: four words per printed row (uniqueID, dense taxon, score,
    hitLength); mask: a byte per dense taxon and one more for taxID 0"""
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
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    bad = L.emu_splitsel_run(C.byref(x), arr(rows, np.uint32), mask.ctypes.data, len(mask) - 1)
    assert not bad, "a pass wrote outside its room"
    return [(outs[s][:min(x.bytes[s], caps[s])].tobytes(), int(x.bytes[s]), int(x.records[s]), bool(x.sized[s])) for s in range(4)]
