"""ctypes wrapper of tests/emu/libcfemu_inflate.so — the CPU harness of the device inflater (TEST ONLY; see emu_inflate.cpp)."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_libs = {}


def build(wave64):
    lib = os.path.join(HERE, "libcfemu_inflate64.so" if wave64 else "libcfemu_inflate.so")
    src = os.path.join(HERE, "emu_inflate.cpp")
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
        L.emu_inflate.restype = C.c_uint64
        L.emu_inflate.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.emu_text_cut.restype = C.c_uint64
        L.emu_text_cut.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.emu_bgzf_member_table.restype = C.c_uint32
        L.emu_bgzf_member_table.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.emu_inflate_wave_lanes.restype = C.c_int
        L.emu_inflate_table_bytes.restype = C.c_uint32
        assert L.emu_inflate_wave_lanes() == (64 if wave64 else 1)
        _libs[wave64] = L
    return _libs[wave64]


# InfErr of cf_inflate.hpp
(OK, BAD_BLOCK_TYPE, STORED_LEN, TOO_MANY_CODES, OVER_SUBSCRIBED, INCOMPLETE, BAD_REPEAT, NO_END_CODE, BAD_CODE, BAD_LEN_SYM, BAD_DIST_SYM,
 DIST_TOO_FAR, OUT_OVERRUN, IN_OVERRUN, OUT_SHORT, CRC) = range(16)


def bgzf_member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, payload=None):
    """one BGZF member (bytes) that holds text; payload: the raw deflate stream to put into it instead of zlib's"""
    if payload is None:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        payload = co.compress(text) + co.flush()
    assert len(text) <= 65536 and len(payload) + 26 <= 65536
    head = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(payload) + 25)
    return head + payload + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text))


def member_table(blob):
    """the per-member table (offset, length of the payload; place, length of the text; CRC32) of whole BGZF members"""
    rows, at, out = [], 0, 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00"
        xlen, = struct.unpack_from("<H", blob, at + 10)
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", blob, at + bsize - 8)
        rows.append((at + 12 + xlen, bsize - 12 - xlen - 8, out, isize, crc))
        at += bsize
        out += isize
    return np.array(rows, dtype=np.uint32).reshape(-1, 5), out


HEADER = 16                       # kInfHeader: a member whose gzip header or size is not BGZF's


def host_member_table(blob, in_at=0, text_at=0):
    """the library's own table of the members (bgzf_member_table of cf_inflate.hpp, which the uploads use), made as they make it: a
    call for the count and the total, one for the table -> table, total, status (OK, or HEADER), the member refused or None;
    OverflowError: refused by exception (members that claim 2^32 - 65536 bytes of text or more)"""
    L = lib()
    blob = bytes(blob)
    n, total = C.c_uint64(0), C.c_uint64(0)
    table = None
    for fill in (False, True):
        if fill:
            table = np.full((n.value + 1, 5), 0xA5A5A5A5, dtype=np.uint32)          # (a guard row behind the members')
            counted = (n.value, total.value)
        st = L.emu_bgzf_member_table(blob, len(blob), in_at, text_at, table.ctypes.data if fill else None, C.byref(n), C.byref(total))
        if st == 0xffffffff:
            raise OverflowError("the members' text does not fit the 32-bit places of a batch")
        if st:
            return None, None, st, n.value
    assert (n.value, total.value) == counted and (table[-1] == 0xA5A5A5A5).all(), "the two calls disagree, or the table was overrun"
    return table[:-1], total.value, OK, None


def inflate(blob, table, n_out, wave64=False, blocks=None):
    """blocks: a list that is filled with the members' numbers of deflate blocks
    -> text (n_out bytes; 0x5A where nothing was written), err (one word per member), first bad member or None"""
    L = lib(wave64)
    comp = np.frombuffer(bytes(blob) + b"\0", dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.uint32)
    out = np.zeros(n_out + 1, dtype=np.uint8)
    err = np.zeros(len(table) + 1, dtype=np.uint32)
    nblk = np.zeros(len(table) + 1, dtype=np.uint32)
    bad = L.emu_inflate(comp.ctypes.data, len(blob), table.ctypes.data, len(table), out.ctypes.data, n_out, err.ctypes.data, nblk.ctypes.data)
    assert bad != 2 ** 64 - 2, "a guard byte around the compressed bytes or the text was changed"
    assert bad != 2 ** 64 - 3, "the table names bytes outside the buffers"
    if blocks is not None:
        blocks[:] = [int(x) for x in nblk[:len(table)]]
    return out[:n_out].tobytes(), err[:len(table)].copy(), (0xffffffff - bad if bad else None)


def text_cut(text, fastq, last, pos_cap=1 << 30, wave64=False):
    n = C.c_uint64(0)
    cut = lib(wave64).emu_text_cut(text, len(text), int(fastq), int(last), pos_cap, C.byref(n))
    return cut, n.value
