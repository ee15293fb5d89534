"""One table of FASTA / FASTQ blocks for the device parser (centrifuge_amd/csrc/cf_textio.hpp: text_count_body, text_mark_body,
text_record_body, text_pack_body), read by the CPU harness (tests/test_textio_emu.py, both builds) and by the GPU
(tests/test_gpu_textcases.py).  Every block is made here, from fixed seeds, so both see the same bytes.

    plain_cases()      blocks in the plain form: the device must take them and give the host parser's reads
    irregular_cases()  blocks outside it, each with the reason bit it must carry
    capacity_cases()   blocks around and far beyond the record capacity of an upload
    mutated(fmt)       the 160 randomly damaged blocks per format: whatever the device takes, it parses as the host parser does

The capacity of an upload (cf_device.hip, uploadTextBlocks), which CAPACITY is worked out from:
    recCap = total / 32 + 1024          total: the block's bytes
    posCap = recCap (FASTA: a marker a record), 4 * recCap (FASTQ: a marker a line)
    a block fits while  records <= recCap  and  markers <= posCap"""
import os
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

import common

FASTA, FASTQ = 0, 1
PIECE, PAD, TILE = 64, 128, 4096
BAD_START, NO_NAME_END, EMPTY_NAME, CARRIAGE_RETURN, BAD_BASE, EMPTY_SEQ, BAD_PLUS, QUAL_LEN, BAD_QUAL, LINE_COUNT, TOO_MANY = (1 << i for i in range(11))
SEEDS = (0, 12345)

Plain = namedtuple("Plain", "group name fmt text text2")
Irregular = namedtuple("Irregular", "group name fmt text bit")


def rec_cap(total):
    return total // 32 + 1024


def pos_cap(total, fmt):
    return rec_cap(total) if fmt == FASTA else 4 * rec_cap(total)


# ------------------------------------------------------------------------------------------------ what the harness had
def make_records(rng, n, fmt, wrap=0, lower=False, ns=True):
    names, recs = [], []
    for i in range(n):
        ln = int(rng.integers(1, 300))
        alphabet = "ACGTN" if ns and rng.random() < 0.3 else "ACGT"
        seq = "".join(rng.choice(list(alphabet), ln))
        if lower and rng.random() < 0.5:
            seq = seq.lower()
        name = ("r%d" % i).encode()
        style = int(rng.integers(0, 7))
        if style == 1:
            name += b" some comment/here"
        elif style == 2:
            name += b"/1"
        elif style == 3:
            name += b"\tx/2"
        elif style == 4:
            name = b"sample/" + name + b"/3"
        elif style == 5:
            name += bytes([200, 255]) + b"x"             # bytes >= 128: the seed takes them sign-extended
        names.append(name)
        if fmt == FASTA:
            body = seq if not wrap else "\n".join(seq[k:k + wrap] for k in range(0, ln, wrap))
            recs.append(b">" + name + b"\n" + body.encode() + b"\n")
        else:
            qual = bytes(int(q) for q in rng.integers(33, 127, ln))
            recs.append(b"@" + name + b"\n" + seq.encode() + b"\n+" + (name if rng.random() < 0.2 else b"") + b"\n" + qual + b"\n")
    return b"".join(recs)


PLAIN_TRIALS = [(1, 0, False), (3, 0, False), (70, 0, True), (200, 60, True), (130, 7, False), (64, 0, False), (65, 1, True)]


def plain_trials(fmt):
    """the harness's plain blocks (records, FASTA wrap, lower case), one generator through all of them"""
    rng = np.random.default_rng(11 + fmt)
    return [make_records(rng, n, fmt, wrap=wrap if fmt == FASTA else 0, lower=lower) for n, wrap, lower in PLAIN_TRIALS]


IRREGULAR_FASTA = [
    (b"\n>a\nACGT\n", 1), (b"#comment\n>a\nACGT\n", 1), (b"ACGT\n>a\nACGT\n", 1),      # does not start with '>'
    (b">a\nACGT\n>b", 2), (b">a>b\nACGT\n", 2),                                           # a name line without its end
    (b">\nACGT\n", 4),                                                                    # no name: the host names it by its ordinal
    (b">a\r\nACGT\r\n", 8), (b">a\nAC\rGT\n", 16),
    (b">a\nACRT\n", 16), (b">a\nAC-T\n", 16), (b">a\nAC.T\n", 16), (b">a\nAC GT\n", 16), (b">a\nAC*\n", 16),
    (b">a\n>b\nACGT\n", 32), (b">a\n\n>b\nACGT\n", 32), (b">a\nACGT\n>b\n", 32),
]
IRREGULAR_FASTQ = [
    (b"\n@a\nACGT\n+\nIIII\n", 1), (b"x\n@a\nACGT\n+\nIIII\n", 1),
    (b"@a\nACGT\n+\nIIII", 512), (b"@a\nACGT\n+\nIIII\n\n", 512), (b"@a\nAC\nGT\n+\nIIII\n", 512),
    (b"@\nACGT\n+\nIIII\n", 4), (b"@a\r\nACGT\r\n+\r\nIIII\r\n", 8),
    (b"@a\nAC.T\n+\nIIII\n", 16), (b"@a\nACRT\n+\nIIII\n", 16), (b"@a\nAC T\n+\nIIII\n", 16),
    (b"@a\n\n+\n\n", 32),
    (b"@a\nACGT\n-\nIIII\n", 64), (b"@a\nACGT\n\nIIII\n", 64),
    (b"@a\nACGT\n+\nIII\n", 128), (b"@a\nACGT\n+\nIIIII\n", 128),
    (b"@a\nACGT\n+\nII I\n", 256), (b"@a\nACGT\n+\nII\tI\n", 256),
    (b"@a\nAC\nGT\n+\nII\nII\n@b\nAC\n", 1 | 64),                                      # wrapped lines: the line count happens to fit
]
# byte 32 at each of the eight offsets of tx_quals' word, in a line of 8 and in the second word of a line of 13
BAD_QUALS = [(b"@a\nACGTACGT\n+\n" + b"I" * o + b" " + b"I" * (7 - o) + b"\n", 256) for o in range(8)] + \
            [(b"@a\nACGTACGTACGTA\n+\n" + b"I" * (8 + o) + b" " + b"I" * (4 - o) + b"\n", 256) for o in range(5)]

JUNK = [b"\r", b">", b"@", b"+", b"\n", b".", b"-", b"R", b"n", b" ", b"\t", b"/", b"/1", b"\n\n", b"*", b"a", b"\x00", b"\xff"]
N_MUTATED = 160


def mutated(fmt):
    """the harness's damaged blocks: a few records, one to three insertions, deletions or replacements"""
    rng = np.random.default_rng(2024 + fmt)
    out = []
    for _ in range(N_MUTATED):
        text = bytearray(make_records(rng, int(rng.integers(1, 8)), fmt, wrap=int(rng.choice([0, 0, 5])) if fmt == FASTA else 0, lower=True))
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(text) + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                text[at:at] = JUNK[int(rng.integers(0, len(JUNK)))]
            elif kind == 1 and at < len(text):
                del text[at:at + int(rng.integers(1, 4))]
            elif at < len(text):
                text[at:at + 1] = JUNK[int(rng.integers(0, len(JUNK)))]
        out.append(bytes(text))
    return out


# ------------------------------------------------------------------------------------------------ records made to measure
def rec(fmt, name, seq, qual=None, plus=b"", wrap=0):
    """one record in the plain form (name, seq, qual: bytes)"""
    if fmt == FASTA:
        body = seq if not wrap else b"\n".join(seq[k:k + wrap] for k in range(0, len(seq), wrap))
        return b">" + name + b"\n" + body + b"\n"
    return b"@" + name + b"\n" + seq + b"\n+" + plus + b"\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


def bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)).encode()


def short(fmt, n, seed=1, first=0):
    """n short records (names r<first>.., 1 to 60 bases, qualities over the whole range) — 40 bytes and more on average, so that a block
    of any number of them fits the upload's capacity"""
    rng = np.random.default_rng(1000 * seed + fmt)
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 61))
        seq = bases(rng, ln, "ACGTN" if rng.random() < 0.2 else "ACGT")
        qual = bytes(int(q) for q in rng.integers(33, 127, ln))
        out.append(rec(fmt, b"r%d" % (first + i), seq, qual))
    return out


def sized(fmt, pieces, residue, seed=2):
    """a block of `pieces` pieces of 64 bytes whose length is `residue` beyond whole pieces: short records, the last readID lengthened"""
    size = pieces * PIECE if residue == 0 else (pieces - 1) * PIECE + residue
    out, have, i = [], 0, 0
    rng = np.random.default_rng(1000 * seed + fmt)
    long = pieces > 64                                         # (the tile-sized blocks: of long reads, a tenth of the records)
    while True:
        ln = int(rng.integers(200, 301)) if long else int(rng.integers(1, 61))
        r = rec(fmt, b"r%d" % i, bases(rng, ln))
        if have + len(r) > size:
            if out:
                break
            continue                                           # (a tiny block: until a record is short enough)
        out.append(r); have += len(r); i += 1
    assert out, (pieces, residue)
    mark = out[-1].index(b"\n")
    out[-1] = out[-1][:mark] + b"x" * (size - have) + out[-1][mark:]
    text = b"".join(out)
    assert len(text) == size and (len(text) + PIECE - 1) // PIECE == pieces and len(text) % PIECE == residue
    return text


COUNTS = (1, 63, 64, 65, 255, 256, 257, 4160)            # 4,160 records: 65 wavefronts, the 64 stripes of the sums wrap
PIECES = (1, 2, TILE - 1, TILE, TILE + 1)                # the marker passes' scan: a tile is 4,096 pieces, the outputs number n + 1
RESIDUES = (63, 0, 1)
MARKER_AT = (0, 7, 8, 15, 16, 63)                        # the halves of cf_load16, the edges of tx_match8's word
SEQ_LENGTHS = tuple(range(1, 41)) + (63, 64, 65, 95, 96, 97, 300)
WRAPS = (1, 7, 8, 9, 60)
NAME_LENGTHS = (1, 2, 255, 256, 300)
QUAL_BYTES = (33, 126, 127, 128, 255)
MATE_COUNTS = (64, 65, 97)
PLACES = (0, 63, 64, 255, 256, 300)                      # where a bad record stands among 300 good ones


def fastq_line_end_at(which, at):
    """a FASTQ record whose line `which` (0 name .. 3 qualities) ends at byte `at`"""
    for ln in range(1, 200):
        for ls in range(1, 200):
            ends = (1 + ln, 2 + ln + ls, 4 + ln + ls, 5 + ln + 2 * ls)
            if ends[which] == at:
                r = rec(FASTQ, b"n" * ln, b"ACGT" * (ls // 4) + b"ACGT"[:ls % 4])
                assert r[at:at + 1] == b"\n" and r.count(b"\n", 0, at) == which
                return r
    raise AssertionError((which, at))


def plain_cases():
    out = []
    for fmt, f in ((FASTA, "fa"), (FASTQ, "fq")):
        def add(group, name, text, text2=None):
            out.append(Plain(group, "%s-%s-%s" % (group, name, f), fmt, text, text2))
        for i, text in enumerate(plain_trials(fmt)):
            add("trials", "n%d-wrap%d-%s" % (PLAIN_TRIALS[i][0], PLAIN_TRIALS[i][1], "lower" if PLAIN_TRIALS[i][2] else "upper"), text)
        if fmt == FASTA:
            add("trials", "no-last-newline", b">a\nACGT\n>b x\nGGN")
        add("trials", "empty", b"")
        # ---- record counts
        for n in COUNTS:
            add("counts", "%d" % n, b"".join(short(fmt, n)))
        # ---- piece and tile edges
        for p in PIECES:
            for r in RESIDUES:
                if p == 1 and r == 1:
                    continue                                   # (no record is one byte long)
                add("pieces", "%dp-mod%d" % (p, r), sized(fmt, p, r))
        # ---- marker placement: the first record is sized so that the marker falls on byte k of the second piece
        for k in MARKER_AT:
            if fmt == FASTA:
                first = rec(fmt, b"first", b"ACGT" * 14 + b"ACGTACGT"[:k])
                first = first[:6] + b"y" * (PIECE + k - len(first)) + first[6:]
                assert len(first) == PIECE + k
                add("markers", "start-at-%d" % k, first + b"".join(short(fmt, 3, seed=3)))
            else:
                for which in range(4):
                    add("markers", "line%d-ends-at-%d" % (which, k), fastq_line_end_at(which, PIECE + k) + b"".join(short(fmt, 3, seed=3)))
        if fmt == FASTA:
            add("markers", "start-then-one-base-at-the-end", b"".join(short(fmt, 2, seed=3)) + b">z\nA")    # ('>' itself as the last byte: irregular_cases)
        # ---- sequence lines
        rng = np.random.default_rng(40 + fmt)
        seqs = [bases(rng, n, "ACGTN" if i % 3 == 0 else "ACGT") for i, n in enumerate(SEQ_LENGTHS)]
        add("seqlines", "lengths", b"".join(rec(fmt, b"len%d" % len(s), s) for s in seqs))
        add("seqlines", "lengths-lower", b"".join(rec(fmt, b"len%d" % len(s), s.lower()) for s in seqs))
        add("seqlines", "lengths-mixed", b"".join(rec(fmt, b"len%d" % len(s), bytes(c | 0x20 if (i * 7 + len(s)) % 3 == 0 else c for i, c in enumerate(s))) for s in seqs))
        if fmt == FASTA:
            for w in WRAPS:
                add("seqlines", "wrap%d" % w, b"".join(rec(fmt, b"len%d" % len(s), s, wrap=w) for s in seqs))
            # the '\n' at each of the eight offsets of tx_load8's window: lines of 8 behind names of 1 to 8 bytes
            add("seqlines", "wrap8-every-phase", b"".join(rec(fmt, b"p" * k, seqs[-1], wrap=8) for k in range(1, 9)))
        for back, bg in (("A", lambda n: b"A" * n), ("mix", lambda n: bases(rng, n))):
            add("seqlines", "n-at-0-to-31-over-%s" % back, b"".join(rec(fmt, b"n%d" % p, bytes(bg(p) + b"N" + bg(39 - p))) for p in range(32)))
        runs = [(5, 10), (6, 9), (7, 8), (0, 15), (14, 17), (15, 16), (8, 15), (1, 38)]
        add("seqlines", "n-runs", b"".join(rec(fmt, b"run%d-%d" % (a, b), bases(rng, a) + b"N" * (b - a + 1) + bases(rng, 39 - b)) for a, b in runs))
        add("seqlines", "all-n", b"".join(rec(fmt, b"alln%d" % n, (b"N" if n % 2 else b"n") * n) for n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65)))
        # ---- names
        body = b"ACGTNACGTA"
        names = [b"x" * n for n in NAME_LENGTHS]
        names += [b"read/1", b"read/2", b"read/3", b"read/4", b"/1", b"/4", b"r/", b"r/12", b"r/1/1", b"r/1 x", b"a/1\t/2"]
        names += [b"/abcdefg", b"a/bcdefg", b"abcd/efg", b"abcd/efg/2"]
        names += [b"ab /cd", b"ab\t/cd", b"ab/ cd", b"ab/\tcd", b"ab / cd/1", b" /1", b"ab cd"]
        names += [b"abcdefgh"[:k] + bytes([hi]) + b"xyz" for hi in (128, 200, 255) for k in range(4)]
        names += [bytes([128, 200, 255, 129]), bytes([255]) + b"/1", b"ab" + bytes([200]) + b"/" + bytes([255])]
        add("names", "edges", b"".join(rec(fmt, nm, body) for nm in names))
        if fmt == FASTQ:
            add("names", "plus-repeats-the-name", b"".join(rec(fmt, nm, body, plus=nm) for nm in names))
        # ---- qualities
        if fmt == FASTQ:
            add("quals", "lengths-1-to-17", b"".join(rec(fmt, b"q%d" % n, bases(rng, n), bytes(int(q) for q in rng.integers(33, 127, n))) for n in range(1, 18)))
            for qb in QUAL_BYTES:
                add("quals", "byte%d-at-each-offset" % qb, b"".join(rec(fmt, b"q%d" % o, b"ACGTACGTACGTACGTA", b"5" * o + bytes([qb]) + b"5" * (16 - o)) for o in range(17)))
                add("quals", "byte%d-throughout" % qb, b"".join(rec(fmt, b"q%d" % n, b"ACGTACGTACGTACGTA"[:n], bytes([qb]) * n) for n in range(1, 18)))
        # ---- mates: two blocks in one upload, the first one's length at every residue (the second block's place follows from it)
        for n in MATE_COUNTS:
            for r in RESIDUES:
                t1 = short(fmt, n, seed=5)
                size = sum(len(x) for x in t1)
                mark = t1[-1].index(b"\n")
                t1[-1] = t1[-1][:mark] + b"x" * ((r - size) % PIECE) + t1[-1][mark:]
                t1 = b"".join(t1)
                assert len(t1) % PIECE == r
                add("mates", "%d-mod%d" % (n, r), t1, b"".join(short(fmt, n, seed=6)))
        # ---- capacity: the largest blocks of the shortest records that still fit
        for unit, n, fits in CAPACITY[fmt]:
            if fits:
                add("capacity", "%d-records-of-%d-bytes" % (n, len(unit)), unit * n)
    return out


# The record counts at the capacity's edge, from the formula in this file's docstring.  FASTA, ">a\nA\n", 5 bytes a record: n
# records fit while n <= 5 n / 32 + 1024 (whole division): 1,213 do (6,065 / 32 = 189, 189 + 1024 = 1,213), 1,214 do not (6,070 / 32
# = 189).  FASTQ: a record of 10 bytes, "@ab\nA\n+\nI\n", fits up to 1,489 (14,890 / 32 = 465, 465 + 1024 = 1,489) and not at 1,490
# (14,900 / 32 = 465); the 9-byte record "@a\nA\n+\nI\n" fits up to 1,424 (12,816 / 32 = 400, 400 + 1024 = 1,424), not at 1,425
# (12,825 / 32 = 400), and so not at 1,489 or 1,490 either.  The markers follow the records: posCap is recCap for FASTA, 4 recCap for
# FASTQ's four lines a record.
CAPACITY = {
    FASTA: [(b">a\nA\n", 1213, True), (b">a\nA\n", 1214, False)],
    FASTQ: [(b"@ab\nA\n+\nI\n", 1489, True), (b"@ab\nA\n+\nI\n", 1490, False),
            (b"@a\nA\n+\nI\n", 1424, True), (b"@a\nA\n+\nI\n", 1425, False), (b"@a\nA\n+\nI\n", 1489, False), (b"@a\nA\n+\nI\n", 1490, False)],
}
FLOOD = 70000                                            # markers and nothing else: far beyond posCap (3,211 / 12,844 for 70,000 bytes)


def capacity_cases():
    """blocks that must come back as kTxTooMany and nothing else"""
    out = []
    for fmt, f in ((FASTA, "fa"), (FASTQ, "fq")):
        for unit, n, fits in CAPACITY[fmt]:
            if not fits:
                out.append(Irregular("capacity", "capacity-%d-records-of-%d-bytes-%s" % (n, len(unit), f), fmt, unit * n, TOO_MANY))
        out.append(Irregular("capacity", "capacity-%d-markers-%s" % (FLOOD, f), fmt, (b">" if fmt == FASTA else b"\n") * FLOOD, TOO_MANY))
    return out


def start_only(text, bit):
    """what is only wrong at the start of a block"""
    return bool(bit & 1) or text[:1] in (b"\n", b"#", b"x", b"A")


def irregular_cases():
    """every block of the lists alone (group 'alone'), behind the harness's 70 records ('after70'), and as record 0, 63, 64, 255, 256
    and 300 of 300 short good records ('placed'): the flag then comes from a lane, a wavefront and a workgroup other than the first.
    A case whose bit is LINE_COUNT stands for a damaged line structure: placed in front of other records it may show as another bit
    (the lines that follow are counted off wrongly) — such a block must be refused, its bit is whatever the CPU harness says."""
    out = []
    for fmt, f, cases in ((FASTA, "fa", IRREGULAR_FASTA + [(b">a\nACGT\n>", NO_NAME_END)]), (FASTQ, "fq", IRREGULAR_FASTQ + BAD_QUALS)):
        good70 = make_records(np.random.default_rng(5), 70, fmt)
        good = short(fmt, 300, seed=7)
        for i, (text, bit) in enumerate(cases):
            out.append(Irregular("alone", "alone-%d-%s" % (i, f), fmt, text, bit))
            if start_only(text, bit):
                out.append(Irregular("placed", "placed-%d-at-0-%s" % (i, f), fmt, text + b"".join(good), bit))
                continue
            out.append(Irregular("after70", "after70-%d-%s" % (i, f), fmt, good70 + text, bit))
            for at in PLACES:
                out.append(Irregular("placed", "placed-%d-at-%d-%s" % (i, at, f), fmt, b"".join(good[:at]) + text + b"".join(good[at:]), bit))
    return out


def carries(flags, bit):
    """the rule of the irregular cases: the block is refused with the case's bit (a damaged line count: refused, with any bit)"""
    return flags & bit == bit or (flags != 0 and bit == LINE_COUNT)


def groups(cases):
    out = {}
    for c in cases:
        out[c.group] = out.get(c.group, 0) + 1
    return out


# ------------------------------------------------------------------------------------------------ the host parser
CLI = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-class")
_host = {}


def read_id(name):
    """aln_sink.h:2203-2217"""
    if len(name) >= 2 and name[-2:] in (b"/1", b"/2", b"/3"):
        name = name[:-2]
    for i, c in enumerate(name):
        if c in b" \t\n\v\f\r":
            return name[:i]
    return name


def host_records(text, fmt, seed=0):
    """the host parser through --dump-reads, one temporary file and one call per block, kept per (block, seed): None when it refuses
    the input, else (name, bases, qualities, seed) per read"""
    key = (text, fmt, seed)
    if key not in _host:
        with tempfile.NamedTemporaryFile(suffix=".fa" if fmt == FASTA else ".fq") as f:
            f.write(text)
            f.flush()
            r = subprocess.run([CLI, "--dump-reads", "-f" if fmt == FASTA else "-q", "--seed", str(seed), "-U", f.name], capture_output=True)
        out = None
        if r.returncode == 0:
            out = []
            for ln in r.stdout.split(b"\n")[:-1]:
                name, seq, qual, sd = ln.rsplit(b"\t", 3)
                out.append((name, seq.decode(), qual, int(sd)))
        if len(_host) > 64:
            _host.clear()
        _host[key] = out
    return _host[key]


def host_parse(text, fmt, seed=0):
    """-> None, or (readID, bases, seed) per read"""
    recs = host_records(text, fmt, seed)
    return None if recs is None else [(read_id(name), seq, sd) for name, seq, _qual, sd in recs]
