"""ctypes wrapper of tests/emu/libcfemu_kreport{,64}.so — the CPU harness of the Kraken-style report's tally (TEST ONLY; see
emu_kreport.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_libs = {}


def build(wave64=False):
    lib = os.path.join(HERE, "libcfemu_kreport%s.so" % ("64" if wave64 else ""))
    src = [os.path.join(HERE, "emu_kreport.cpp"), os.path.join(ROOT, "centrifuge_amd/csrc/cf_index.cpp")]
    deps = src + [os.path.join(ROOT, "centrifuge_amd/csrc", f) for f in ("cf_kernels.hpp", "cf_platform.hpp", "cf_index.hpp", "cf_kreport_tree.hpp")]

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
                               "-fno-strict-aliasing"] + (["-DCF_EMU_WAVE64=1"] if wave64 else []) + ["-o", tmp] + src)
        os.replace(tmp, lib)
    return lib


def lib(wave64=False):
    if wave64 not in _libs:
        L = C.CDLL(build(wave64))
        u64p, u32p = C.c_void_p, C.c_void_p
        L.emu_kreport_table.restype = C.c_int
        L.emu_kreport_table.argtypes = [C.c_uint64, u64p, u64p, u64p, C.c_uint64, u64p, C.c_char_p]
        L.emu_kreport_index.restype = C.c_uint64
        L.emu_kreport_index.argtypes = [C.c_char_p, u64p, u64p, C.c_uint64]
        L.emu_kreport_lca.restype = C.c_uint32
        L.emu_kreport_lca.argtypes = [u64p, C.c_uint32, C.c_uint32]
        L.emu_kreport.restype = C.c_uint32
        L.emu_kreport.argtypes = [u64p, C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u64p]
        for f in ("emu_kreport_field_rows", "emu_kreport_slot_bits", "emu_kreport_probes", "emu_kreport_chunk"):
            getattr(L, f).restype = C.c_uint32
        _libs[wave64] = L
    return _libs[wave64]


class Refused(Exception):
    pass


def table(nodes, taxa, wave64=False):
    """nodes: (tid, parent) pairs as the index lists them; taxa: the dense taxon ids (sorted; 0 and 1 among them) -> the device's table (u64 per taxon)"""
    tid = np.array([t for t, _ in nodes], dtype=np.uint64)
    par = np.array([p for _, p in nodes], dtype=np.uint64)
    taxa = np.ascontiguousarray(taxa, dtype=np.uint64)
    tab = np.zeros(len(taxa), dtype=np.uint64)
    msg = C.create_string_buffer(128)
    if lib(wave64).emu_kreport_table(len(tid), tid.ctypes.data, par.ctypes.data, taxa.ctypes.data, len(taxa), tab.ctypes.data, msg):
        raise Refused(msg.value.decode())
    return tab


def index_table(base, wave64=False):
    """-> the dense taxon ids of an index, their table"""
    cap = 1 << 22
    taxa, tab = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    n = lib(wave64).emu_kreport_index(base.encode(), taxa.ctypes.data, tab.ctypes.data, cap)
    assert n, "emu_kreport_index failed"
    return taxa[:n].copy(), tab[:n].copy()


def lca(tab, a, b, wave64=False):
    return int(lib(wave64).emu_kreport_lca(tab.ctypes.data, int(a), int(b)))


def tally(tab, n_out, rows, q_lo=0, q_hi=None, chunk=None, slot_bits=None, wave64=False):
    """kreport_body over the queries: n_out rows each, rows[q, j] their dense taxon indices -> counts (nTaxa + 1: per taxon, then the
    reads), what of them went through the LDS tallies (nTaxa), blocks run"""
    L = lib(wave64)
    n_out = np.ascontiguousarray(n_out, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    nq, k = rows.shape
    assert len(n_out) == nq and k >= 1
    counts, lds = np.zeros(len(tab) + 1, dtype=np.uint64), np.zeros(len(tab), dtype=np.uint64)
    blocks = L.emu_kreport(tab.ctypes.data, len(tab), nq, n_out.ctypes.data, rows.ctypes.data, k, q_lo, nq if q_hi is None else q_hi,
                           chunk or L.emu_kreport_chunk(), slot_bits or L.emu_kreport_slot_bits(), counts.ctypes.data, lds.ctypes.data)
    assert blocks != 2 ** 32 - 1, "the body wrote behind its LDS"
    return counts, lds, blocks
