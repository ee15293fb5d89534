"""The device inflater (inflate_body, centrifuge_amd/csrc/cf_inflate.hpp) in the CPU harness of tests/emu/emu_inflate.cpp — one lane
per member and wavefronts of 64 lanes — against zlib, byte for byte: BGZF members made here with zlib's raw deflate (stored, fixed
and dynamic blocks, every strategy that changes what the stream holds), the sizes and distances at the format's limits, and corrupt
streams: every check the decoder makes once, and seeded single-byte flips.  A corrupt stream ends in a status, the guard bytes the
harness puts around the compressed bytes and around the text stay as they are (emu_inflate.inflate asserts it).  The streams are
those of tests/codeccases.py, which tests/test_gpu_codec.py gives to the device as well.  The cut rule of a
BGZF upload (text_cut_body) is stated here once more in plain Python."""
import struct
import zlib

import numpy as np
import pytest

import codeccases as K
from codeccases import CRAFTED, TEXT, fastq_text
from emu import emu_inflate as E

WAVES = [False, True]


def inflate_members(members, wave64, blocks=None):
    """whole members (bytes each) through the harness -> text, err, bad"""
    blob = b"".join(members)
    table, n = E.member_table(blob)
    return E.inflate(blob, table, n, wave64, blocks)


def roundtrip(members_text, wave64, blocks=None, **kw):
    out, err, bad = inflate_members([E.bgzf_member(t, **kw) for t in members_text], wave64, blocks)
    assert bad is None and not err.any(), (bad, err)
    assert out == b"".join(members_text)


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("name", sorted(K.STREAMS))
def test_streams(name, wave64):
    roundtrip(K.STREAM_TEXTS, wave64, **K.STREAMS[name])


@pytest.mark.parametrize("wave64", WAVES)
def test_sizes_and_distances(wave64):
    for texts, kw in K.sizes_and_distances():
        roundtrip(texts, wave64, **kw)


@pytest.mark.parametrize("wave64", WAVES)
def test_a_match_at_the_distance_limit(wave64):
    """codeccases.distance_limit: one match at distance 32,768 behind exactly 32,768 bytes, and behind 32,767"""
    (payload, text), (short, claimed) = K.distance_limit()
    assert zlib.decompress(payload, -15) == text
    out, err, bad = inflate_members([E.bgzf_member(text, payload=payload)], wave64)
    assert bad is None and not err.any() and out == text
    out, err, bad = inflate_members([E.bgzf_member(claimed, payload=short)], wave64)
    assert bad == 0 and err[0] == E.DIST_TOO_FAR


@pytest.mark.parametrize("wave64", WAVES)
def test_fastq_member_with_several_deflate_blocks(wave64):
    text = fastq_text(65280, 11)
    blocks = []
    roundtrip([text], wave64, blocks, level=6)
    assert blocks[0] >= 2, blocks


@pytest.mark.parametrize("name", K.WELL_FORMED_NAMES)
def test_every_well_formed_stream_is_zlibs_text(name):
    """the table's own claim: every member, as a gzip member and as a raw stream, gives its text under zlib, whole"""
    members, min_blocks = K.well_formed()[name]
    for text, m in members:
        assert zlib.decompress(m, 31) == text
        d = zlib.decompressobj(-15)
        assert d.decompress(m[18:-8]) == text and d.eof and d.unused_data == b""
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(text), len(text)) and len(m) <= 65536 and len(text) <= 65536


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("name", K.WELL_FORMED_NAMES)
def test_well_formed_streams_of_the_formats_corners(name, wave64):
    """the streams the device is given (tests/test_gpu_codec.py), between two short members and an empty one: the text, a status of 0
    for every member, the deflate blocks the case claims"""
    members, min_blocks = K.well_formed()[name]
    good = E.bgzf_member(K.GOOD_NEIGHBOUR)
    blocks = []
    out, err, bad = inflate_members([good, E.bgzf_member(b"")] + [m for _, m in members] + [good], wave64, blocks)
    assert bad is None and not err.any(), (bad, err)
    assert out == K.GOOD_NEIGHBOUR + b"".join(t for t, _ in members) + K.GOOD_NEIGHBOUR
    assert blocks[2] >= min_blocks, blocks


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_corrupt_streams_end_in_a_status(name, wave64):
    payload, text, word = CRAFTED[name]
    try:                                             # zlib refuses it too, or leaves another text
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) != text or not d.eof
    except zlib.error:
        pass
    good = E.bgzf_member(K.GOOD_NEIGHBOUR)
    blob = good + E.bgzf_member(text, payload=payload) + good
    table, n = E.member_table(blob)
    out, err, bad = E.inflate(blob, table, n, wave64)
    assert bad == 1 and list(err) == [0, word, 0]
    assert out[:21] == b"the member before it\n" and out[n - 21:] == b"the member before it\n"      # the others are inflated all the same


@pytest.mark.parametrize("wave64", WAVES)
def test_crc_is_checked(wave64):
    m = K.crc_flip()
    table, n = E.member_table(m)
    out, err, bad = E.inflate(m, table, n, wave64)
    assert bad == 0 and err[0] == E.CRC and out == K.CRC_TEXT == TEXT[:5000]


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("level", [0, 6])
def test_single_byte_flips(level, wave64):
    text = K.FLIP_TEXT
    n_bad = 0
    series = K.flips(level)
    assert len(series) == 100 and len(text) == 3000
    for x, ref_ok in series:
        table, n = E.member_table(x)
        out, err, bad = E.inflate(x, table, n, wave64)
        assert (bad is None) == ref_ok, err
        if bad is None:
            assert out == text
        n_bad += bad is not None
    assert n_bad > 50


def plain_cut(text, fastq, last):
    if last:
        return len(text)
    if fastq:
        ends = [i for i, ch in enumerate(text) if ch == 10]
        k = len(ends) & ~3
        return ends[k - 1] + 1 if k else 0
    starts = [i for i, ch in enumerate(text) if ch == 62 and (i == 0 or text[i - 1] == 10)]
    return starts[-1] if starts else 0


def test_cut_rule():
    fq = fastq_text(3000, 5)
    fa = b">r1 x\nACGT\nAC\n>r2 a>b\nGGG\n>r3\nAC"
    for text, fastq in [(fq, 1), (fa, 0)]:
        for end in list(range(0, 120)) + [len(text)]:
            for last in (0, 1):
                t = text[:end]
                cut, k = E.text_cut(t, fastq, last)
                assert cut == plain_cut(t, fastq, last), (end, fastq, last)
                marker = 10 if fastq else 62
                assert k == sum(1 for ch in t[:cut] if ch == marker)
    # more markers than are kept: nothing is cut (the record pass refuses such a block)
    assert E.text_cut(fq, 1, 0, pos_cap=5)[0] == len(fq)


# ---- the member table the host makes of an upload's members (bgzf_member_table: the only reader of BGZF headers on the upload path)
def blob_of(text, size):
    return b"".join(E.bgzf_member(text[i:i + size]) for i in range(0, len(text), size)) + E.bgzf_member(b"")     # (the empty member a BGZF file ends with)


def wide_member(text):
    """a member with XLEN 12: the BC subfield first, six bytes of another subfield behind it"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = co.compress(text) + co.flush()
    head = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 12) + b"BC" + struct.pack("<HH", 2, 12 + 12 + len(payload) + 8 - 1) + b"XY\x02\x00\x07\x09"
    return head + payload + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text))


TABLE_BLOBS = {
    "no_member": b"",
    "one_empty_member": E.bgzf_member(b""),
    "members_of_700": blob_of(TEXT, 700),
    "members_of_65280": blob_of(fastq_text(150000, 2), 65280),
    "xlen_12": wide_member(TEXT[:900]) + E.bgzf_member(TEXT[900:1000]) + wide_member(b""),
}


@pytest.mark.parametrize("in_at,text_at", [(0, 0), (4104, 1000003)])
@pytest.mark.parametrize("name", sorted(TABLE_BLOBS))
def test_member_table_of_well_formed_members(name, in_at, text_at):
    blob = TABLE_BLOBS[name]
    want, want_total = E.member_table(blob)
    want = want.astype(np.uint64)
    want[:, 0] += in_at; want[:, 2] += text_at
    table, total, status, bad = E.host_member_table(blob, in_at, text_at)
    assert (status, bad) == (E.OK, None) and total == want_total
    assert table.shape == want.shape and np.array_equal(table, want)
    if name == "xlen_12":
        assert table[0, 0] == in_at + 24 and len(table) == 3


def altered(at, value):
    def f(m):
        m = bytearray(m); m[at] = value
        return bytes(m)
    return f


GOOD = E.bgzf_member(b">r\nACGT\n")
REFUSED = {                                                # what is done to the second of three members
    "fewer_than_18_bytes_left": lambda m: m[:17],          # (nothing follows it: the blob ends inside the header)
    "magic_first_byte": altered(0, 0x1e), "magic_second_byte": altered(1, 0x8a),
    "cm_not_8": altered(2, 9), "fextra_clear": altered(3, 0),
    "xlen_below_6": altered(10, 5),
    "no_B": altered(12, ord("X")), "no_C": altered(13, ord("X")), "slen_low": altered(14, 3), "slen_high": altered(15, 1),
    "bsize_below_header_and_trailer": lambda m: m[:16] + struct.pack("<H", 12 + 6 + 8 - 2) + m[18:],
    "bsize_beyond_the_bytes_given": lambda m: m[:16] + struct.pack("<H", 0xffff) + m[18:],
    "isize_65537": lambda m: m[:-4] + struct.pack("<I", 65537),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_member_table_refuses_a_header_that_is_not_bgzfs(name):
    assert E.host_member_table(GOOD * 3)[2:] == (E.OK, None)
    second = REFUSED[name](GOOD)
    blob = GOOD + second + (GOOD if len(second) == len(GOOD) else b"")
    assert 3 * len(GOOD) < 0xffff
    assert E.host_member_table(blob, 8, 64)[2:] == (E.HEADER, 1)
    assert E.host_member_table(second + GOOD)[2:] == (E.HEADER, 0)


def test_member_table_refuses_a_text_beyond_the_32_bit_places():
    """ISIZE trailers that sum to 2^32 - 65536 or more: refused by exception from the trailers alone (members that claim 64 KiB each)"""
    big = E.bgzf_member(b"")[:-4] + struct.pack("<I", 65536)
    with pytest.raises(OverflowError):
        E.host_member_table(big * 65540)
    with pytest.raises(OverflowError):
        E.host_member_table(big * 65535)                   # 2^32 - 65536 itself
    table, total, status, bad = E.host_member_table(big * 65534)
    assert status == E.OK and total == 65534 * 65536 and int(table[-1, 2]) + 65536 == total
