"""ctypes wrapper of tests/emu/libcfemu_deflate.so — the CPU harness of the device deflater (TEST ONLY; see emu_deflate.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MEMBER = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_lib = None


def build(hash_bits=None, window=None):
    """hash_bits / window: a harness with another table or window than the library's (tools/deflate_ratio.py), in a file of its own"""
    variant = hash_bits is not None or window is not None
    defs = ([] if hash_bits is None else ["-DCF_DEF_HASH_BITS=%d" % hash_bits]) + ([] if window is None else ["-DCF_DEF_WINDOW=%d" % window])
    lib = os.path.join(HERE, "libcfemu_deflate%s.so" % ("_%s_%s" % (hash_bits, window) if variant else ""))
    src = os.path.join(HERE, "emu_deflate.cpp")
    deps = [src] + [os.path.join(ROOT, "centrifuge_amd/csrc", f) for f in ("cf_platform.hpp", "cf_inflate.hpp", "cf_deflate.hpp")]

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
                               "-fno-strict-aliasing"] + defs + ["-o", tmp, src])
        os.replace(tmp, lib)
    return lib


def load(path):
    L = C.CDLL(path)
    L.emu_deflate.restype = C.c_uint64
    L.emu_deflate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    L.emu_deflate_stride.restype = C.c_uint32
    L.emu_deflate_stride.argtypes = [C.c_uint32]
    L.emu_deflate_table_bytes.restype = C.c_uint32
    L.emu_deflate_window.restype = C.c_uint32
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


def deflate(text, member=MEMBER, L=None):
    """-> the BGZF members of text (bytes, one after the other), their sizes (u32 per member); L: a variant's library (load(build(...)))"""
    L = L or lib()
    text = bytes(text)
    n_members = (len(text) + member - 1) // member
    out = np.zeros(n_members * L.emu_deflate_stride(member) + 1, dtype=np.uint8)
    size = np.zeros(n_members + 1, dtype=np.uint32)
    n = C.c_uint64(0)
    rc = L.emu_deflate(text, len(text), member, out.ctypes.data, C.byref(n), size.ctypes.data)
    assert rc != 2 ** 64 - 2, "a guard byte around the text or the members was changed"
    assert rc != 2 ** 64 - 3, "the member size is not a multiple of 64 in 64 .. 65280"
    assert rc == 0
    return out[:n.value].tobytes(), size[:n_members].copy()
