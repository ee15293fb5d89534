"""ctypes wrapper of tests/emu/libcfemu_matecut.so — the CPU harness of the common cut of a BGZF pair upload (TEST ONLY; see emu_matecut.cpp)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_matecut64.so" if wave64 else "libcfemu_matecut.so")
    src = os.path.join(HERE, "emu_matecut.cpp")
    deps = [src] + [os.path.join(ROOT, "centrifuge_amd/csrc", f) for f in ("cf_platform.hpp", "cf_inflate.hpp")]

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
        L.emu_text_cut_pair.restype = C.c_uint32
        L.emu_text_cut_pair.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.POINTER(C.c_uint64)]
        L.emu_matecut_wave_lanes.restype = C.c_int
        L.emu_matecut_bad_start.restype = C.c_uint32
        assert L.emu_matecut_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


def bad_start(wave64=False):
    return lib(wave64).emu_matecut_bad_start()


def text_cut_pair(text0, text1, fastq, last0, last1, pos_cap0=1 << 30, pos_cap1=1 << 30, wave64=False):
    """-> (cut 0, markers in front of it), (cut 1, markers in front of it), flags"""
    out = (C.c_uint64 * 4)()
    flags = lib(wave64).emu_text_cut_pair(text0, len(text0), text1, len(text1), int(fastq), int(last0), int(last1), pos_cap0, pos_cap1, out)
    return (out[0], out[1]), (out[2], out[3]), flags
