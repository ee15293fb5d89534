"""cf_bgzf_eof and cf_bgzf_deflate_host (include/centrifuge_amd.h): the BGZF container made on the host — no device needed."""
import ctypes as C
import gzip

import numpy as np
import pytest

from centrifuge_amd import capi
from emu import emu_inflate as I


def test_eof_member():
    eof = capi.bgzf_eof()
    assert eof == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000") and gzip.decompress(eof) == b""


@pytest.mark.parametrize("member", [None, "64", "4096"])
def test_host_members_inflate_to_the_text(member, monkeypatch):
    if member:
        monkeypatch.setenv("CF_BGZF_OUT_MEMBER", member)
    size = int(member or 65280)
    rng = np.random.default_rng(3)
    rows = b"".join(b"r%d_%d\tseq%d\t%d\t%d\t0\t99\t100\t1\n" % (i, i % 7, i % 30, 1000 + i % 30, 81 * (i % 90)) for i in range(4000))
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()           # (deflates to more than it is: stored)
    for text in (b"", b"a", rows[:size - 1], rows[:size], rows[:size + 1], rows, noise):
        text = text[:300 * size]                                              # (64-byte members: a short text is enough)
        z = capi.bgzf_deflate_host(text)
        if not text:
            assert z == b""
            continue
        table, n = I.member_table(z)
        assert n == len(text) and len(table) == (len(text) + size - 1) // size and all(int(r[3]) <= size for r in table)
        assert gzip.decompress(z + capi.bgzf_eof()) == text
        out, err, bad = I.inflate(z, table, n)
        assert bad is None and out == text


def test_too_little_room_and_a_bad_member_size_are_argument_errors(monkeypatch):
    L = capi.lib()
    text = b"some text, some text, some text\n" * 10
    out, n = (C.c_uint8 * 30)(), C.c_uint64(0)
    assert L.cf_bgzf_deflate_host(text, len(text), out, 30, C.byref(n)) != 0 and b"too small" in L.cf_last_error()
    monkeypatch.setenv("CF_BGZF_OUT_MEMBER", "100")
    with pytest.raises(capi.CfError):
        capi.bgzf_deflate_host(text)
