"""The device inflater (inflate_body, centrifuge_amd/csrc/cf_inflate.hpp) in the CPU harness of tests/emu/emu_inflate.cpp — one lane
per member and wavefronts of 64 lanes — against zlib, byte for byte: BGZF members made here with zlib's raw deflate (stored, fixed
and dynamic blocks, every strategy that changes what the stream holds), the sizes and distances at the format's limits, and corrupt
streams: every check the decoder makes once, and seeded single-byte flips.  A corrupt stream ends in a status, the guard bytes the
harness puts around the compressed bytes and around the text stay as they are (emu_inflate.inflate asserts it).  The cut rule of a
BGZF upload (text_cut_body) is stated here once more in plain Python."""
import random
import struct
import zlib

import numpy as np
import pytest

from emu import emu_inflate as E

WAVES = [False, True]


def fastq_text(n_bytes, seed):
    rng = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n_bytes:
        L = rng.choice([36, 100, 151])
        out += b"@read%d/1\n%s\n+\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(L)), bytes(rng.randrange(33, 74) for _ in range(L)))
        i += 1
    return bytes(out[:n_bytes])


def roundtrip(members_text, wave64, blocks=None, **kw):
    blob = b"".join(E.bgzf_member(t, **kw) for t in members_text)
    table, n = E.member_table(blob)
    out, err, bad = E.inflate(blob, table, n, wave64, blocks)
    assert bad is None and not err.any(), (bad, err)
    assert out == b"".join(members_text)
    return blob


TEXT = fastq_text(40000, 1)
STREAMS = {
    "stored": dict(level=0),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
}


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_streams(name, wave64):
    roundtrip([TEXT, TEXT[:777], b"", TEXT[5:6]], wave64, **STREAMS[name])


@pytest.mark.parametrize("wave64", WAVES)
def test_sizes_and_distances(wave64):
    rng = random.Random(7)
    far = bytes(rng.randrange(256) for _ in range(32768))
    for level in (1, 6, 9):
        roundtrip([b"", b"A", b"", fastq_text(65536, 3)[:65536]], wave64, level=level)
        roundtrip([b"G" * 65536], wave64, level=level)                 # distance 1, matches of 258
        roundtrip([far + far[:300]], wave64, level=level)               # (zlib stores it: the match at that distance is the next test's)
        roundtrip([b"ACGTA" * 13000], wave64, level=level)              # a distance shorter than the match, no power of two
    # 65,536 bytes stored (the member is larger than its text: level 0 of a shorter text, for the 64 KiB a BGZF member may take)
    roundtrip([far + far[:32000]], wave64, level=0)


@pytest.mark.parametrize("wave64", WAVES)
def test_a_match_at_the_distance_limit(wave64):
    """zlib never emits a distance beyond 32,768 - 262 (and stores random bytes), so the stream is written by hand: 32,768 bytes in a
    stored block, then a fixed block with ONE match — length symbol 285 (258 bytes), distance symbol 29 with its 13 extra bits all
    set: 24,577 + 8,191 = 32,768, the format's limit and exactly what the member has produced — and the end-of-block code."""
    rng = random.Random(7)
    far = bytes(rng.randrange(256) for _ in range(32768))
    payload = Bits().put(0, 1).put(0, 2).bytes() + struct.pack("<HH", 32768, 32768 ^ 0xffff) + far
    payload += Bits().put(1, 1).put(1, 2).code(0xc5, 8).code(29, 5).put(8191, 13).code(0, 7).bytes()
    text = far + far[:258]
    assert zlib.decompress(payload, -15) == text
    blob = E.bgzf_member(text, payload=payload)
    table, n = E.member_table(blob)
    out, err, bad = E.inflate(blob, table, n, wave64)
    assert bad is None and not err.any() and out == text
    # one byte further back than the member has produced: the same stream behind 32,767 bytes
    short = Bits().put(0, 1).put(0, 2).bytes() + struct.pack("<HH", 32767, 32767 ^ 0xffff) + far[:32767]
    short += Bits().put(1, 1).put(1, 2).code(0xc5, 8).code(29, 5).put(8191, 13).code(0, 7).bytes()
    blob = E.bgzf_member(far[:32767] + bytes(258), payload=short)
    table, n = E.member_table(blob)
    out, err, bad = E.inflate(blob, table, n, wave64)
    assert bad == 0 and err[0] == E.DIST_TOO_FAR


@pytest.mark.parametrize("wave64", WAVES)
def test_fastq_member_with_several_deflate_blocks(wave64):
    text = fastq_text(65280, 11)
    blocks = []
    roundtrip([text], wave64, blocks, level=6)
    assert blocks[0] >= 2, blocks


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):                 # as the format packs numbers: least significant bit first
        self.v |= value << self.n
        self.n += nbits
        return self

    def code(self, value, nbits):                # a Huffman code: most significant bit first
        for i in range(nbits - 1, -1, -1):
            self.put((value >> i) & 1, 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(b, ch):
    return b.code(0x30 + ch, 8) if ch < 144 else b.code(0x190 + ch - 144, 9)


def crafted():
    """name -> (payload, text the trailer names, the decoder's word)"""
    c = {}
    c["block type 3"] = (Bits().put(1, 1).put(3, 2).bytes(), b"", E.BAD_BLOCK_TYPE)
    c["stored LEN / NLEN"] = (Bits().put(1, 1).put(0, 2).put(0, 5).put(3, 16).put(0xfffd, 16).bytes() + b"abc", b"abc", E.STORED_LEN)
    c["stored past the payload"] = (Bits().put(1, 1).put(0, 2).put(0, 5).put(9, 16).put(0xfff6, 16).bytes() + b"abc", b"abcdefghi", E.IN_OVERRUN)
    c["length symbol 286"] = (fixed_lit(Bits().put(1, 1).put(1, 2), 65).code(0xc6, 8).bytes(), b"A" * 4, E.BAD_LEN_SYM)
    c["length symbol 287"] = (fixed_lit(Bits().put(1, 1).put(1, 2), 65).code(0xc7, 8).bytes(), b"A" * 4, E.BAD_LEN_SYM)
    for d in (30, 31):
        c["distance symbol %d" % d] = (fixed_lit(Bits().put(1, 1).put(1, 2), 65).code(1, 7).code(d, 5).bytes(), b"A" * 4, E.BAD_DIST_SYM)
    c["distance before the member"] = (fixed_lit(Bits().put(1, 1).put(1, 2), 65).code(1, 7).code(1, 5).code(0, 7).bytes(), b"A" * 4, E.DIST_TOO_FAR)
    good = fixed_lit(fixed_lit(Bits().put(1, 1).put(1, 2), 65), 66).code(0, 7).bytes()
    c["text shorter than ISIZE"] = (good, b"ABC", E.OUT_SHORT)
    c["text longer than ISIZE"] = (good, b"A", E.OUT_OVERRUN)
    c["match longer than ISIZE"] = (fixed_lit(Bits().put(1, 1).put(1, 2), 65).code(2, 7).code(0, 5).code(0, 7).bytes(), b"AAAA", E.OUT_OVERRUN)
    c["no end of block"] = (fixed_lit(Bits().put(1, 1).put(1, 2), 65).bytes()[:1], b"A", E.IN_OVERRUN)
    # dynamic blocks: HLIT 257, HDIST 1, then the code-length code's lengths in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    dyn = lambda hclen: Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(hclen - 4, 4)
    c["code-length code over-subscribed"] = (dyn(4).put(1, 3).put(1, 3).put(1, 3).put(0, 3).bytes(), b"", E.OVER_SUBSCRIBED)
    c["code-length code incomplete"] = (dyn(4).put(1, 3).put(0, 3).put(0, 3).put(0, 3).bytes(), b"", E.INCOMPLETE)
    b = dyn(18)
    for i in range(18):
        b.put(1 if i in (15, 17) else 0, 3)          # lengths 1 for the symbols 2 and 1: "0" = a length of 1, "1" = a length of 2
    over = Bits().put(b.v, b.n)
    for _ in range(258):
        over.put(0, 1)                               # 258 codes of one bit
    c["length code over-subscribed"] = (over.bytes(), b"", E.OVER_SUBSCRIBED)
    c["too many codes"] = (Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).bytes() + bytes(8), b"", E.TOO_MANY_CODES)
    c["repeat without a length before it"] = (Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(1, 3).put(1, 1).put(0, 2).bytes() + bytes(4), b"", E.BAD_REPEAT)
    return c


CRAFTED = crafted()


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_corrupt_streams_end_in_a_status(name, wave64):
    payload, text, word = CRAFTED[name]
    try:                                             # zlib refuses it too, or leaves another text
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) != text or not d.eof
    except zlib.error:
        pass
    good = E.bgzf_member(b"the member before it\n")
    blob = good + E.bgzf_member(text, payload=payload) + good
    table, n = E.member_table(blob)
    out, err, bad = E.inflate(blob, table, n, wave64)
    assert bad == 1 and list(err) == [0, word, 0]
    assert out[:21] == b"the member before it\n" and out[n - 21:] == b"the member before it\n"      # the others are inflated all the same


@pytest.mark.parametrize("wave64", WAVES)
def test_crc_is_checked(wave64):
    m = bytearray(E.bgzf_member(TEXT[:5000]))
    m[-8] ^= 1
    table, n = E.member_table(bytes(m))
    out, err, bad = E.inflate(bytes(m), table, n, wave64)
    assert bad == 0 and err[0] == E.CRC and out == TEXT[:5000]


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("level", [0, 6])
def test_single_byte_flips(level, wave64):
    text = TEXT[:3000]
    m = E.bgzf_member(text, level=level)
    rng = random.Random(1234 + level)
    n_bad = 0
    for _ in range(100):
        at = rng.randrange(18, len(m) - 4)           # the payload and the CRC (the header and ISIZE are the host's to read)
        x = bytearray(m)
        x[at] ^= 1 << rng.randrange(8)
        try:
            d = zlib.decompressobj(-15)
            ref = d.decompress(bytes(x[18:-8]))
            ref_ok = d.eof and ref == text and struct.unpack_from("<I", x, len(x) - 8)[0] == zlib.crc32(text)
        except zlib.error:
            ref_ok = False
        table, n = E.member_table(bytes(x))
        out, err, bad = E.inflate(bytes(x), table, n, wave64)
        assert (bad is None) == ref_ok, (at, err)
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
