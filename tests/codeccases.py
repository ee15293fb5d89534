"""The DEFLATE codec's cases, one table for both builds: the CPU harness (tests/test_inflate_emu.py, tests/test_deflate_emu.py)
and the device (tests/test_gpu_codec.py) read the same streams and texts.

Inflate: BGZF members made with zlib's raw deflate in every strategy that changes what a stream holds (STREAMS), the sizes and
distances at the format's limits, streams written by hand from explicit code lengths (a small canonical-Huffman writer: Block) —
the reference of a hand-written stream is zlib.decompress(payload, -15), asserted where the stream is made —, and corrupt streams:
one per check the decoder makes (crafted()) and seeded single-byte flips (flips()).

Deflate: the text shapes at a lane piece's and a member's edges (EDGE_SIZES, rows_text() and what follows them)."""
import random
import struct
import zlib

import numpy as np

from emu import emu_inflate as E

MEMBER = 65280                                   # kDefMember of cf_deflate.hpp


def fastq_text(n_bytes, seed):
    rng = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n_bytes:
        L = rng.choice([36, 100, 151])
        out += b"@read%d/1\n%s\n+\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(L)), bytes(rng.randrange(33, 74) for _ in range(L)))
        i += 1
    return bytes(out[:n_bytes])


TEXT = fastq_text(40000, 1)
STREAMS = {
    "stored": dict(level=0),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
}
STREAM_TEXTS = [TEXT, TEXT[:777], b"", TEXT[5:6]]


def far_bytes():
    rng = random.Random(7)
    return bytes(rng.randrange(256) for _ in range(32768))


def sizes_and_distances():
    """-> [(the members' texts, what bgzf_member is given)]"""
    far = far_bytes()
    out = []
    for level in (1, 6, 9):
        out.append(([b"", b"A", b"", fastq_text(65536, 3)[:65536]], dict(level=level)))
        out.append(([b"G" * 65536], dict(level=level)))                 # distance 1, matches of 258
        out.append(([far + far[:300]], dict(level=level)))               # (zlib stores it: the match at that distance is distance_limit()'s)
        out.append(([b"ACGTA" * 13000], dict(level=level)))              # a distance shorter than the match, no power of two
    # 65,536 bytes stored (the member is larger than its text: level 0 of a shorter text, for the 64 KiB a BGZF member may take)
    out.append(([far + far[:32000]], dict(level=0)))
    return out


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


def distance_limit():
    """zlib never emits a distance beyond 32,768 - 262 (and stores random bytes), so the stream is written by hand: 32,768 bytes in a
    stored block, then a fixed block with ONE match — length symbol 285 (258 bytes), distance symbol 29 with its 13 extra bits all
    set: 24,577 + 8,191 = 32,768, the format's limit and exactly what the member has produced — and the end-of-block code.
    -> (payload, text) of that stream, (payload, the text its trailer names) of the same stream behind 32,767 bytes: one byte
    further back than the member has produced"""
    far = far_bytes()
    payload = Bits().put(0, 1).put(0, 2).bytes() + struct.pack("<HH", 32768, 32768 ^ 0xffff) + far
    payload += Bits().put(1, 1).put(1, 2).code(0xc5, 8).code(29, 5).put(8191, 13).code(0, 7).bytes()
    text = far + far[:258]
    assert zlib.decompress(payload, -15) == text
    short = Bits().put(0, 1).put(0, 2).bytes() + struct.pack("<HH", 32767, 32767 ^ 0xffff) + far[:32767]
    short += Bits().put(1, 1).put(1, 2).code(0xc5, 8).code(29, 5).put(8191, 13).code(0, 7).bytes()
    return (payload, text), (short, far[:32767] + bytes(258))


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
GOOD_NEIGHBOUR = b"the member before it\n"
CRC_TEXT = TEXT[:5000]


def crc_flip():
    """a member whose trailer names another CRC32 than its text's"""
    m = bytearray(E.bgzf_member(CRC_TEXT))
    m[-8] ^= 1
    return bytes(m)


FLIP_TEXT = TEXT[:3000]


def flips(level):
    """100 seeded single-bit flips in the payload or the CRC of one member -> [(the member, zlib reads FLIP_TEXT from it and the CRC is its)]"""
    m = E.bgzf_member(FLIP_TEXT, level=level)
    rng = random.Random(1234 + level)
    out = []
    for _ in range(100):
        at = rng.randrange(18, len(m) - 4)           # the payload and the CRC (the header and ISIZE are the host's to read)
        x = bytearray(m)
        x[at] ^= 1 << rng.randrange(8)
        try:
            d = zlib.decompressobj(-15)
            ref = d.decompress(bytes(x[18:-8]))
            ref_ok = d.eof and ref == FLIP_TEXT and struct.unpack_from("<I", x, len(x) - 8)[0] == zlib.crc32(FLIP_TEXT)
        except zlib.error:
            ref_ok = False
        out.append((bytes(x), ref_ok))
    return out


# ---- streams written by hand: literals and matches (tokens) in blocks of given code lengths
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def len_symbol(n):
    """a match length -> (symbol - 257, extra bits' value); 258 is symbol 285's alone"""
    if n == 258:
        return 28, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= n)
    assert n - LEN_BASE[s] < 1 << LEN_EXTRA[s]
    return s, n - LEN_BASE[s]


def dist_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    assert d - DIST_BASE[s] < 1 << DIST_EXTRA[s]
    return s, d - DIST_BASE[s]


def canonical(lengths):
    """code lengths per symbol -> {symbol: (code, length)}, numbered as RFC 1951 3.2.2 numbers them"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """the code space the lengths take, in units of 2^-15 (32768: a complete code)"""
    return sum(1 << (15 - l) for l in lengths if l)


def skewed(k, maxbits):
    """the lengths of a complete code over k >= 2 symbols that is as lopsided as maxbits allows: 1, 2, 3, ... and the rest balanced"""
    out, depth, r = [], 0, k
    while r > 1 and r - 1 <= 1 << (maxbits - depth - 1):
        depth += 1
        out.append(depth)
        r -= 1
    if r == 1:
        out.append(depth)
    else:
        b = (r - 1).bit_length()
        out += [depth + b - 1] * ((1 << b) - r) + [depth + b] * (2 * r - (1 << b))
    assert kraft(out) == 32768 and max(out) <= maxbits and len(out) == k
    return out


def apply_tokens(tokens, text=b""):
    """literals (an int) and matches ((length, distance)) -> the text, behind what the member holds already"""
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out) and d <= 32768
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(text):])


def run_ops(lens):
    """the code lengths of a dynamic block as the code-length code's symbols, runs folded greedily
    -> [(symbol, extra bits, their value, the place in lens the symbol starts at, the lengths it stands for)]"""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            n = min(run, 138)
            ops.append((17, 3, n - 3, i, n) if n <= 10 else (18, 7, n - 11, i, n))
            i += n
        elif v and i and lens[i - 1] == v and run >= 3:
            n = min(run, 6)
            ops.append((16, 2, n - 3, i, n))
            i += n
        else:
            ops.append((v, 0, 0, i, 1))
            i += 1
    return ops


class Block:
    """one deflate block written into a Bits; .used: the literal / length and the distance symbols whose codes were written,
    .ops: a dynamic block's code-length symbols (run_ops), .start: the bit the block's header starts at"""

    def __init__(self, bits, final):
        self.b, self.final, self.start = bits, final, bits.n
        self.used, self.dused, self.ops = set(), set(), []

    def stored(self, data):
        self.b.put(self.final, 1).put(0, 2)
        self.b.put(0, -self.b.n % 8)
        self.b.put(len(data), 16).put(len(data) ^ 0xffff, 16)
        for ch in data:
            self.b.put(ch, 8)
        return self

    def fixed(self, tokens):
        self.b.put(self.final, 1).put(1, 2)
        return self._tokens(tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))

    def dynamic(self, tokens, lit, dist, cl_maxbits=7):
        """lit: the literal / length code's lengths (HLIT = len(lit)), dist: the distance code's (HDIST = len(dist))"""
        assert 257 <= len(lit) <= 286 and 1 <= len(dist) <= 30
        self.ops = run_ops(list(lit) + list(dist))
        # the code-length code: complete, over the symbols in use (one more where there is only one), lopsided up to cl_maxbits
        freq = {}
        for op in self.ops:
            freq[op[0]] = freq.get(op[0], 0) + 1
        if len(freq) == 1:
            freq[0 if 0 not in freq else 1] = 0
        syms = sorted(freq, key=lambda s: (-freq[s], s))
        cl = [0] * 19
        for s, l in zip(syms, skewed(len(syms), cl_maxbits)):
            cl[s] = l
        ncode = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
        self.b.put(self.final, 1).put(2, 2).put(len(lit) - 257, 5).put(len(dist) - 1, 5).put(ncode - 4, 4)
        for i in range(ncode):
            self.b.put(cl[CL_ORDER[i]], 3)
        codes = canonical(cl)
        for sym, eb, ev, _, _ in self.ops:
            self.b.code(*codes[sym])
            self.b.put(ev, eb)
        self.cl = cl
        return self._tokens(tokens, canonical(lit), canonical(dist))

    def _tokens(self, tokens, lc, dc):
        for t in tokens:
            if isinstance(t, int):
                self.b.code(*lc[t]); self.used.add(t)
                continue
            n, d = t
            s, ev = len_symbol(n)
            self.b.code(*lc[257 + s]); self.used.add(257 + s)
            self.b.put(ev, LEN_EXTRA[s])
            s, ev = dist_symbol(d)
            self.b.code(*dc[s]); self.dused.add(s)
            self.b.put(ev, DIST_EXTRA[s])
        self.b.code(*lc[256]); self.used.add(256)
        return self


def hand(payload, text):
    """a hand-written member: zlib reads the text from its payload, to the stream's end"""
    d = zlib.decompressobj(-15)
    assert d.decompress(payload) == text and d.eof and not d.unused_data
    return [(text, E.bgzf_member(text, payload=payload))]


def long_codes():
    """Codes beyond the first-level lookups (10 bits for literal / length codes, 8 for distance codes): the literal / length code has
    the lengths 1, 2, ..., 14, 15, 15 over sixteen symbols, the end of the block among the 15-bit ones; the distance code 1, 2, ...,
    15, 15 over the symbols 0 .. 15.  The text uses every code, and the 11- to 15-bit literals are each followed by a match."""
    order = [65, 257, 67, 71, 270, 84, 78, 97, 99, 285, 103, 116, 110, 10, 64, 256]        # lengths 1 .. 15, 15 in this order
    lit = [0] * 286
    for l, s in zip(list(range(1, 16)) + [15], order):
        lit[s] = l
    dist = list(range(1, 16)) + [15]
    assert kraft(lit) == 32768 and kraft(dist) == 32768 and lit[256] == 15
    tokens = [s for s in order if s < 256] * 20                       # 240 bytes: distance symbol 15 (193 .. 256) has its room
    for k, s in enumerate(range(16)):
        longlit = [103, 116, 110, 10, 64][k % 5]                       # a literal of 11 .. 15 bits, directly followed by a match
        tokens += [longlit, ([3, 23, 26, 258][k % 4], DIST_BASE[s] + (k % (1 << DIST_EXTRA[s])))]
        tokens += [65, 67, (3, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)]
    b = Bits()
    blk = Block(b, 1).dynamic(tokens, lit, dist)
    assert blk.used == set(order) and blk.dused == set(range(16))
    assert {lit[t] for i, t in enumerate(tokens[:-1]) if isinstance(t, int) and not isinstance(tokens[i + 1], int)} >= {11, 12, 13, 14, 15}
    return hand(b.bytes(), apply_tokens(tokens))


def every_symbol():
    """HLIT = 286 and HDIST = 30, every length and distance symbol at least once: every extra-bit class with its smallest and its
    largest value, length 258 through symbol 285, the lengths 3 .. 10 that have no extra bits.  Both codes reach 15 bits."""
    tokens = list(range(256))
    for s in range(28):
        tokens += [(LEN_BASE[s], 1 + s), (LEN_BASE[s] + (1 << LEN_EXTRA[s]) - 1, 256)]
    tokens += [(258, 256)] * 120                                     # room for the far distances: 24,577 and beyond
    have = len(apply_tokens(tokens))
    assert have > 32768
    for s in range(30):
        tokens += [(3 + s, DIST_BASE[s]), (4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)]
    tokens += [(258, 32768), 0, 255]
    freq = [0] * 286
    for t in tokens:
        freq[t if isinstance(t, int) else 257 + len_symbol(t[0])[0]] += 1
    lit = [0] * 286
    for s, l in zip(sorted(range(286), key=lambda s: (-freq[s], s)), skewed(286, 15)):
        lit[s] = l
    lit[256], lit[0] = lit[0], lit[256]                               # (the end of the block once: a long code is enough for it)
    dist = skewed(30, 15)
    b = Bits()
    blk = Block(b, 1).dynamic(tokens, lit, dist)
    assert blk.used == set(range(286)) and blk.dused == set(range(30)) and max(lit) == 15 and max(dist) == 15 and min(lit) == 1
    text = apply_tokens(tokens)
    assert len(text) <= 65536
    return hand(b.bytes(), text)


def repeat_across(kind):
    """A code-length repeat that starts in the literal / length code's lengths and ends in the distance code's (i < nlen < i + rep):
    symbol 16 (the lengths 3 3 3 3 | 3 3 ... : `previous length` repeated) or symbol 18 (zeros behind the last length symbol in use
    and in front of the first distance symbol in use)"""
    if kind == 16:
        lit = [0] * 258
        for s in (97, 98, 99, 100, 254, 255, 256, 257):
            lit[s] = 3
        dist = [3] * 8
        tokens = [97, 98, 99, 100, 254, 255, (3, 6), (3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 7), (3, 9), (3, 13), 97]
    else:
        lit = [0] * 286
        for s in (97, 98, 256, 257):
            lit[s] = 2
        dist = [0, 0, 0, 0, 1, 1]
        tokens = [97, 98, 98, 97, 97, 98, 97, (3, 5), (3, 7), (3, 6), 98, (3, 8)]
    b = Bits()
    blk = Block(b, 1).dynamic(tokens, lit, dist)
    nlen = len(lit)
    assert any(sym == kind and i < nlen < i + rep for sym, _, _, i, rep in blk.ops), blk.ops
    return hand(b.bytes(), apply_tokens(tokens))


def one_distance_code(sym):
    """a distance code that is a single one-bit code (incomplete, as zlib writes and accepts it)"""
    lit = [0] * 259
    for s, l in zip((120, 121, 256, 257, 258), (2, 2, 2, 3, 3)):
        lit[s] = l
    tokens = [120, 121, 120, 120, (4, 1 + sym), 121, (3, 1 + sym), (4, 1 + sym)]
    b = Bits()
    blk = Block(b, 1).dynamic(tokens, lit, [0] * sym + [1])
    assert blk.dused == {sym}
    return hand(b.bytes(), apply_tokens(tokens))


def no_distance_code():
    """HDIST = 1 with the length 0: literals only"""
    lit = [0] * 257
    for s, l in zip((120, 200, 256, 10), (1, 2, 3, 3)):
        lit[s] = l
    tokens = [120, 200, 10, 120, 120, 200]
    b = Bits()
    Block(b, 1).dynamic(tokens, lit, [0])
    return hand(b.bytes(), apply_tokens(tokens))


def mixed_blocks():
    """One member: a stored block, a fixed block, an EMPTY stored block, a dynamic block, a stored block again.  The matches of the
    fixed block reach back into the stored one, those of the dynamic block into both; the stored blocks in the middle and at the end
    start at bits other than a byte's first, and not three bits in front of a byte's end either: there is padding to skip."""
    rng = random.Random(21)
    a = bytes(rng.randrange(256) for _ in range(301))
    b = Bits()
    Block(b, 0).stored(a)
    t1 = [65, 66, (40, 301), 67, (258, 150), (3, 3), 200, (65, 64)]
    Block(b, 0).fixed(t1)
    text = a + apply_tokens(t1, a)
    at_fixed = len(a)
    empty = Block(b, 0)
    empty.stored(b"")
    lit = [0] * 286
    order = [97, 257, 98, 285, 99, 269, 256]
    for s, l in zip(order, skewed(len(order), 15)):
        lit[s] = l
    t2 = [97, 98, (3, len(text) + 2), 99, (258, len(text) - at_fixed), (19, 5), (3, 2), 97, (258, 700), 98, (3, 1)]
    Block(b, 0).dynamic(t2, lit, skewed(30, 15))
    text += apply_tokens(t2, text)
    last = Block(b, 1)
    tail = bytes(rng.randrange(256) for _ in range(77))
    last.stored(tail)
    text += tail
    for blk in (empty, last):
        assert blk.start % 8 not in (0, 5), blk.start
    return hand(b.bytes(), text)


def lane_stride_matches():
    """Matches with the distances 1, 2, 3, 63, 64, 65 and the lengths 3, 64, 65, 258: both sides of the 64 lanes that copy a match"""
    tokens = [33 + (7 * i) % 90 for i in range(65)]
    for d in (1, 2, 3, 63, 64, 65):
        for n in (3, 64, 65, 258):
            tokens += [(n, d), 33 + (d + n) % 90]
    b = Bits()
    Block(b, 1).fixed(tokens)
    return hand(b.bytes(), apply_tokens(tokens))


def fixed_literals(text):
    """the text as the literals of one fixed block: 9 bits for a byte >= 144"""
    b = Bits()
    Block(b, 1).fixed(list(text))
    return hand(b.bytes(), text)


def zlib_members(texts, **kw):
    return [(t, E.bgzf_member(t, **kw)) for t in texts]


_well_formed = None


def well_formed():
    """name -> ([(text, member)], the deflate blocks the first member holds at least): every STREAMS entry and the streams of the
    format's corners.  Made once."""
    global _well_formed
    if _well_formed is None:
        w = {}
        for name in sorted(STREAMS):
            w["streams " + name] = (zlib_members(STREAM_TEXTS, **STREAMS[name]), 1)
        w["several deflate blocks"] = (zlib_members([fastq_text(65280, 11)], level=6), 2)
        w["distance 32768"] = (hand(*distance_limit()[0]), 2)
        w["codes of 11 to 15 bits"] = (long_codes(), 1)
        w["every length and distance symbol"] = (every_symbol(), 1)
        w["repeat 16 across the codes"] = (repeat_across(16), 1)
        w["repeat 18 across the codes"] = (repeat_across(18), 1)
        w["one distance code, symbol 0"] = (one_distance_code(0), 1)
        w["one distance code, symbol 1"] = (one_distance_code(1), 1)
        w["no distance code"] = (no_distance_code(), 1)
        w["stored, fixed, dynamic, stored"] = (mixed_blocks(), 5)
        w["distances around 64"] = (lane_stride_matches(), 1)
        rnd = np.random.default_rng(3)
        # (zlib stores random bytes whatever the strategy: their fixed block is written here)
        w["random bytes, fixed"] = (fixed_literals(rnd.integers(0, 256, 6000, dtype=np.uint8).tobytes()), 1)
        w["bytes from 144, fixed"] = (zlib_members([rnd.integers(144, 256, 20000, dtype=np.uint8).tobytes()], level=6, strategy=zlib.Z_FIXED), 1)
        assert all((m[0][1][18] >> 1) & 3 == 1 for m in (w["random bytes, fixed"][0], w["bytes from 144, fixed"][0]))
        w["65536 bytes at level 9"] = (zlib_members([fastq_text(65536, 13)], level=9), 2)
        _well_formed = w
    return _well_formed


WELL_FORMED_NAMES = ["streams " + n for n in sorted(STREAMS)] + [
    "several deflate blocks", "distance 32768", "codes of 11 to 15 bits", "every length and distance symbol", "repeat 16 across the codes",
    "repeat 18 across the codes", "one distance code, symbol 0", "one distance code, symbol 1", "no distance code",
    "stored, fixed, dynamic, stored", "distances around 64", "random bytes, fixed", "bytes from 144, fixed", "65536 bytes at level 9"]


# ---- the deflater's texts
PIECE = MEMBER // 64
EDGE_SIZES = [1, 2, 3, 4, PIECE - 1, PIECE, PIECE + 1, MEMBER - 1, MEMBER, MEMBER + 1]
ONE_BYTE_RUNS = [3, 257, 258, 259, 260, PIECE, PIECE + 2, 3 * PIECE + 7, MEMBER, MEMBER + 300]
PERIODS = [1, 2, 52, 500, 13056, 13057]


def rows_text(n):
    """n bytes of rows as the formatter writes them"""
    rng = np.random.default_rng(n)
    words = [b"seq%d\t" % i for i in range(40)] + [b"\n", b"100\t", b"genus\t"]
    text = b"".join(words[int(k)] for k in rng.integers(0, len(words), n // 3 + 2))[:n]
    assert len(text) == n
    return text


def match_end_texts(piece=PIECE):
    """matches at a text's very end, and runs that start in front of a piece's end and go on behind it"""
    out = [b"abcdefgh-xyz-abc", b"0123456789" * 7 + b"##" + b"789"]
    unit = bytes(range(33, 97))
    for lead in (piece - 70, piece - 5, piece - 3, piece - 2, piece - 1):
        if lead >= 64:
            out.append(bytes((7 * i) % 23 + 97 for i in range(lead - 64)) + unit + unit + unit + b"tail")
    return out


def member_end_text():
    text = (b"r%d\tgenus\t102\n" % 7) * 5100
    assert len(text) > MEMBER
    return text


def high_bytes():
    return np.random.default_rng(5).integers(144, 256, 3000, dtype=np.uint8).tobytes()


def nine_bit_texts():
    """-> [(text, member size)]: bytes >= 144 (9 bits as literals) mixed with ASCII"""
    hi = high_bytes()
    return [(b"".join(b"read_%d\t" % i + hi[3 * i:3 * i + 3] + b"\tseq7\t1007\n" for i in range(1000)), MEMBER), (hi, MEMBER),
            (hi[:700] + b"plain ascii plain ascii plain ascii" * 30 + hi[700:1500], 1024)]


def random_member():
    return np.random.default_rng(11).integers(0, 256, MEMBER, dtype=np.uint8).tobytes()


def threshold_text():
    """40 members of 64 random bytes and one of 5 (no three bytes repeat inside a member: literals only)"""
    return random_member()[:64 * 40 + 5]


def literals_fixed_bytes(piece):
    """the payload of a fixed block of the piece's literals: 3 bits, 8 or 9 a byte, 7 for the end of the block"""
    return (3 + sum(8 if c < 144 else 9 for c in piece) + 7 + 7) // 8


def stored_where_shorter(text, member, stored):
    """stored[m]: member m came out stored.  The stored form (the text and 5 bytes) is taken exactly where the fixed block is LONGER:
    the text holds members on either side and members where the two are equal, which stay fixed"""
    pieces = [text[i:i + member] for i in range(0, len(text), member)]
    want = [literals_fixed_bytes(p) > len(p) + 5 for p in pieces]
    ties = [literals_fixed_bytes(p) == len(p) + 5 for p in pieces]
    assert True in want and False in want and True in ties
    return list(stored) == want


def high_then_ascii():
    """4,096 bytes >= 144 (stored: 9 bits a literal), then 4,096 'A' (not stored)"""
    return np.random.default_rng(12).integers(144, 256, 4096, dtype=np.uint8).tobytes() + b"A" * 4096
