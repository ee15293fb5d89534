"""Reads for the index builder's corner cases (tests/buildcases.py, groups A - F): what the classifier's kernels are asked at the
index shapes where they change behaviour - texts shorter than the ftab, than 64 bases (no text tables), '$' on side and word
edges, -o 0 ... 20, -t 1 ... 12, sequences shorter than the 11-base overlap, 65,535 / 65,536 sequences.

A read case is a build case plus a deterministic recipe of at most 150 reads of at most 300 bases, all made from the case's own
joined text with seeded generators, and a claim about what the oracle finds for them (tests/test_classify_cases.py checks it, so a
recipe that has drifted fails instead of quietly testing nothing).  tests/golden/make_classify_golden.py runs the unmodified
reference over every case and records digests in tests/golden/classify_edges.json; tests/test_gpu_classify_edges.py classifies the
same reads on the GPU.

The kinds of reads (the prefix of a read's name says which): whole (the text, its reverse complement, the text between 40 random
bases, the text twice), piece (starts / ends at position 0, the last base, each sequence start and one base to either side, in the
lengths PIECE_LENGTHS around the ftab width, the 22-base minimum hit and the word sizes), span (across a sequence boundary 1 : many,
half : half, many : 1, and across three sequences where they are short), row (the prefix of the text, whose match ends in the '$'
row's suffix, and the suffixes of row 0, z - 1, z + 1, n - 1), sub / subn (one substitution / one N at base 0, 9, 10, 11, 21, 22,
the middle, the last base of a 60- and a 100-base piece), mark (starts on a boundary mark, 11 bases before a
sequence start, and one base to either side), chim (a piece + the reverse complement of another), rand, cls (one
length per strand-record class), sw (216 ... 256 bases around the search kernel's 8-bit hit count, -t 1 / -t 2 only), unit (the
repeated unit of the d_all_* / d_acgt_* texts: ranges larger than ihits), homo, deg (empty, all-N, one base, homopolymers)."""
import hashlib
import json
import os

import numpy as np

import buildcases as B
from buildcases import REF_OVERLAP

GROUPS = "ABCDEF"
MAX_READS, MAX_LEN = 150, 300
SHORT_SEQ_CASES = ("a_2x5", "a_3x5", "c_3x5_rate0", "c_short_tail_rate0", "e_marks_collide", "e_all_n_between")
MATE_CASES = ("a_3x5", "b_rows384", "c_rate0", "c_short_tail_rate0", "d_ftab1", "d_all_a_rounds1", "e_marks_collide", "f_seqs65536")
SUB_PLACES = (0, 9, 10, 11, 21, 22)
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
# the strand-record classes of sizeBatch: <= 128 (4 words), <= 192 (6), <= 256 (8), beyond (the byte-window kernel)
CLASS_EDGES = (128, 192, 256, MAX_LEN)


def piece_lengths(ftab_chars):
    return sorted({max(1, ftab_chars - 1), ftab_chars, ftab_chars + 1, 15, 21, 22, 23, 31, 32, 33, 64, 65})


def rc(x):
    y = x[::-1].copy()
    y[y < 4] = 3 - y[y < 4]
    return y


def length_class(n):
    return next(i for i, e in enumerate(CLASS_EDGES) if n <= e)


def _thin(cands, budget):
    """every stride-th candidate, so that the (length, position, side) grid is sampled along its diagonals"""
    if len(cands) <= budget:
        return cands
    stride = -(-len(cands) // budget)
    return [c for c in cands if c[0] % stride == 0]


def make_reads(c):
    """[(name bytes, codes u8)] of build case c"""
    t = c.codes
    n, ftc = len(t), c.ftab_chars
    starts = c.starts()
    rng = np.random.default_rng(7000 + B.NAMES.index(c.name))
    rnd = lambda k: rng.integers(0, 4, k, dtype=np.uint8)                    # noqa: E731
    out, seen = [], set()

    def add(kind, r):
        r = np.ascontiguousarray(r, dtype=np.uint8)[:MAX_LEN]
        key = r.tobytes()
        if key in seen and kind != "deg":
            return
        seen.add(key)
        out.append((kind, r))

    def cut(L, at=None):
        """L bases from the text where it is long enough, else the text and random bases"""
        if n >= L:
            s = int(rng.integers(0, n - L + 1)) if at is None else at
            return t[s:s + L].copy()
        return np.concatenate([t, rnd(L - n)])

    # the whole text
    if n <= MAX_LEN:
        add("whole", t); add("whole", rc(t))
    if n + 80 <= MAX_LEN:
        add("whole", np.concatenate([rnd(40), t, rnd(40)]))
    if 2 * n <= MAX_LEN:
        add("whole", np.concatenate([t, t]))
    # boundaries (the first three and the last of a case with many)
    bounds = starts[1:4] + (starts[-1:] if len(starts) > 4 else [])
    for s in bounds:
        L = min(60, n)
        add("span", t[max(0, s - 1):s - 1 + L])
        add("span", t[max(0, s - L // 2):s + L // 2])
        add("span", t[max(0, s + 1 - L):s + 1])
    if c.name in SHORT_SEQ_CASES and len(starts) >= 3:
        add("span", t[max(0, starts[1] - 2):starts[2] + 2])
    # a hit that starts on a boundary mark (11 bases before a sequence start, or position 0) and one base to either side: its row
    # is a row of the boundary table, for one of the marks the LAST one - the equality case of `row <= lastBoundary` in the walks
    for s in bounds:
        for d in (-1, 0, 1):
            p = max(0, s - REF_OVERLAP) + d
            if 0 <= p < n:
                add("mark", t[p:p + 40])
    # rows of the suffix array
    if n <= 20000:
        sa = B.suffix_array(t)
        z = int(np.nonzero(sa == 0)[0][0])
        add("row", t[:min(n, 60)])
        for r in (0, z - 1, z + 1, n - 1):
            if 0 <= r <= n and sa[r] < n:
                add("row", t[sa[r]:sa[r] + 60])
    # one substitution / one N
    if n >= 60:
        for L in (60, min(n, 100)):
            p = cut(L)
            for at in SUB_PLACES + (L // 2, L - 1):
                q = p.copy(); q[at] = (q[at] + 1 + rng.integers(0, 3)) & 3
                add("sub", q)
                q = p.copy(); q[at] = 4
                add("subn", q)
    # chimeras, as common.edge_reads makes them
    if n >= 30:
        for la, lb in ((45, 45), (50, 50), (30, 60), (24, 70), (40, 23)):
            a, b_ = cut(min(n, 100)), cut(min(n, 100))
            add("chim", np.concatenate([a[:la], rc(b_[10:10 + lb])]))
    for _ in range(10):
        add("rand", rnd(100))
    for _ in range(2):
        add("rand", rnd(250))
    for L in (128, 129, 192, 193, 256, 257, 300):
        add("cls", cut(L))
    if ftc <= 2:
        for L in (216, 217, 218, 219, 220, 256):
            add("sw", cut(L))
        add("homo", np.zeros(200, dtype=np.uint8)); add("homo", np.full(200, 3, dtype=np.uint8))
        # as many hits on a strand as a read that is still searched can have: an N in every 7th place (under the 15 % at which
        # a read is dropped) between text pieces of 6 bases, which a ftab this short lets end early
        for L in (217, 256):
            r = cut(L); r[3::7] = 4
            add("nrich", r)
            r = rnd(L); r[5::7] = 4
            add("nrich", r)
    if c.name.startswith(("d_all_a", "d_all_t", "d_acgt")):
        for L in (21, 22, 50, 100):
            add("unit", t[:L])
        add("unit", rc(t[:50])); add("unit", t[1:51]); add("unit", t[2:42])
    # the degenerate reads of common.edge_reads
    for r in (np.zeros(0, dtype=np.uint8), np.full(50, 4, dtype=np.uint8), np.full(1, 2, dtype=np.uint8), np.zeros(40, dtype=np.uint8),
              np.full(33, 3, dtype=np.uint8)):
        add("deg", r)
    if n >= 90:
        r = cut(90); r[40:46] = 4
        add("deg", r)
    # pieces on position 0, the last base, the sequence starts and one base to either side: what is left of the 150
    spots = sorted({0, n} | {p for s in starts[:3] + starts[-1:] for p in (s - 1, s, s + 1) if 0 <= p <= n})
    cands = []
    for li, L in enumerate(piece_lengths(ftc)):
        for pi, p in enumerate(spots):
            if p < n:
                cands.append((li + 2 * pi, t[p:p + L]))
            if p > 0:
                cands.append((li + 2 * pi + 1, t[max(0, p - L):p]))
    uniq, pieces = set(seen), []
    for d, r in cands:
        if r.tobytes() not in uniq:
            uniq.add(r.tobytes()); pieces.append((d, r))
    for _, r in _thin(pieces, MAX_READS - len(out)):
        add("piece", r)
    assert len(out) <= MAX_READS and all(len(r) <= MAX_LEN for _, r in out), (c.name, len(out))
    return [(b"%s_%d" % (k.encode(), i), r) for i, (k, r) in enumerate(out)]


def make_mates(rs, seed):
    """the reads as mate 1, a shuffled selection as mate 2 with one mate the reference filters (all N)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(rs))
    m2 = [(b"%s" % rs[i][0], rs[int(perm[i])][1]) for i in range(len(rs))]
    m2[len(rs) // 2] = (m2[len(rs) // 2][0], np.full(30, 4, dtype=np.uint8))
    return m2


def fasta_bytes(rs):
    return b"".join(b">" + nm + b"\n" + LETTERS[r].tobytes() + b"\n" for nm, r in rs)


# ------------------------------------------------------------------ claims, over the oracle's view of a case
class View:
    """what a claim may look at: the reads, and the oracle's hit lists and rows of each (made by test_classify_cases.py)"""

    def __init__(self, case, reads, hits, n_rows, starts, n):
        self.case, self.reads, self.hits, self.n_rows, self.starts, self.n = case, reads, hits, n_rows, starts, n

    def kinds(self, k):
        return [i for i, (nm, _) in enumerate(self.reads) if nm.startswith(k.encode())]

    def classified(self, kind=None):
        return sum(1 for i in (self.kinds(kind) if kind else range(len(self.reads))) if self.n_rows[i] > 0)

    def max_strand_hits(self):
        return max((max(len(f), len(r)) for f, r in self.hits), default=0)

    def straddling(self, resolve):
        """reads with a one-row hit of >= 22 bases whose text interval crosses a sequence start"""
        inner = np.array(self.starts[1:], dtype=np.int64)
        cnt = 0
        for f, r in self.hits:
            ok = False
            for h in list(f) + list(r):
                if int(h["bot"]) - int(h["top"]) == 1 and int(h["len"]) >= 22:
                    p = int(resolve[int(h["top"])])
                    ok = ok or bool(np.any((inner > p) & (inner < p + int(h["len"]))))
            cnt += ok
        return cnt

    def last_boundary_row(self, sa):
        """the largest row of a boundary mark, and whether a walk can meet it: not the '$' row, not a row of the SA sample"""
        inv = np.empty(len(sa), dtype=np.int64)
        inv[sa] = np.arange(len(sa))
        row = max(int(inv[max(0, s - REF_OVERLAP)]) for s in self.starts)
        return row, row != int(inv[0]) and row % (1 << self.case.build.off_rate) != 0

    def on_last_boundary(self, sa):
        """reads with a one-row hit of >= 22 bases on the last boundary row"""
        row, _ = self.last_boundary_row(sa)
        return sum(1 for f, r in self.hits if any(int(h["top"]) == row and int(h["bot"]) == row + 1 and int(h["len"]) >= 22 for h in list(f) + list(r)))

    def big_ranges(self, size):
        return sum(1 for f, r in self.hits if any(int(h["len"]) > 0 and int(h["bot"]) - int(h["top"]) > size for h in list(f) + list(r)))


def _claim(c):
    """(text, predicate over a View [and a row resolver]) of build case c"""
    name, n = c.name, c.n
    if name in ("c_3x5_rate0", "a_3x5", "a_2x5") or (c.group == "A" and n < 22):
        return "every read is searched and none classified: no 22-base hit fits the text", lambda v, rs: v.classified() == 0 and len(v.reads) >= 20
    if c.group == "A" or name.startswith("b_len"):
        return "the whole text, its reverse complement and the text inside a longer read are classified", lambda v, rs: v.classified("whole") >= 3
    if name in ("c_short_tail_rate0", "e_marks_collide") or name.startswith("e_start") or name in ("e_leading_n", "e_all_n_between_long"):
        return ">= 3 reads whose oracle hit straddles a sequence boundary; where a walk can meet the last boundary row (not '$', not sampled), a read's hit is on it", \
            lambda v, rs: v.straddling(rs) >= 3 and (v.on_last_boundary(rs) >= 1 or not v.last_boundary_row(rs)[1])
    if name == "e_all_n_between":
        return "every read is searched and none classified (13 bases)", lambda v, rs: v.classified() == 0
    if name.startswith(("d_all_a", "d_all_t")):
        return ">= 4 reads with a range larger than ihits (200 rows), skipped: nothing is classified", lambda v, rs: v.big_ranges(200) >= 4 and v.classified() == 0
    if name.startswith("d_acgt"):
        return ">= 4 reads with a range of more than 100 rows (125 copies of the unit: under ihits, resolved)", lambda v, rs: v.big_ranges(100) >= 4 and v.classified("cls") >= 5
    if c.ftab_chars <= 2:
        return ">= 1 read with more than 64 hits on a strand; the pieces are classified", lambda v, rs: v.max_strand_hits() > 64 and v.classified("cls") >= 5
    if c.group == "F":
        return ">= 9 reads across the first and the last sequence boundaries are classified (40-base sequences)", lambda v, rs: v.classified("span") >= 9
    if c.group == "B":
        return "the suffixes of row 0, z +- 1 and n - 1 (where '$' leaves them) and the text's prefix are classified", \
            lambda v, rs: v.classified("row") >= 3 and v.classified("cls") >= 6
    return "the pieces, the substituted pieces and the chimeras are classified", \
        lambda v, rs: v.classified("cls") >= 6 and v.classified("sub") >= 12 and v.classified("chim") >= 3


class ReadCase:
    def __init__(self, build):
        self.build, self.name, self.group = build, build.name, build.group
        self.mates = build.name in MATE_CASES
        self.k50 = build.group == "D"
        self.claim_text, self.claim = _claim(build)
        self._reads = None

    @property
    def reads(self):
        if self._reads is None:
            self._reads = make_reads(self.build)
        return self._reads

    @property
    def mate2(self):
        return make_mates(self.reads, 9000 + B.NAMES.index(self.name))

    def fasta_sha256(self):
        return hashlib.sha256(fasta_bytes(self.reads)).hexdigest()

    def runs(self):
        """[(run id, reference options, paired)] the record holds of the case"""
        out = [("k5", ["-k", "5"], False), ("k1", ["-k", "1"], False)]
        if self.k50:
            out.append(("k50_min15", ["-k", "50", "--min-hitlen", "15"], False))
        if self.mates:
            out.append(("pe_k5", ["-k", "5"], True))
        return out


RUN_KW = {"k5": dict(k=5), "k1": dict(k=1), "k50_min15": dict(k=50, min_hitlen=15), "pe_k5": dict(k=5)}
CASES = [ReadCase(c) for c in B.CASES if c.group in GROUPS]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
assert set(MATE_CASES) <= set(NAMES) and {BY_NAME[m].group for m in MATE_CASES} == set(GROUPS)

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classify_edges.json")


def load_golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)["cases"]


def kept_names():
    """the cases the reference binary ran: the others have no truth and leave the comparisons"""
    g = load_golden()
    return [n for n in NAMES if "refused" not in g[n]]


def by_group(names):
    return {g: [n for n in names if BY_NAME[n].group == g] for g in GROUPS}


def load_arrays(rs, mate2=None, gen_seed=None):
    """the reads as the classifier's arrays, seeds as reads.load makes them from a FASTA -> names, qlens, seq, off, seeds, paired"""
    from centrifuge_amd import capi
    L = capi.lib()
    lst, names, qlens, seeds = [], [], [], []
    for i, (nm, r) in enumerate(rs):
        ql = 0
        for nm_, r_ in ((nm, r),) + (((mate2[i]),) if mate2 else ()):
            r_ = np.ascontiguousarray(r_, dtype=np.uint8)
            q = np.full(len(r_), ord("I"), dtype=np.uint8)
            lst.append(r_)
            ql += len(r_)
            seeds.append(L.cf_gen_rand_seed(r_.ctypes.data if len(r_) else None, q.ctypes.data if len(r_) else None, len(r_), nm_, len(nm_), 0))
        names.append(nm); qlens.append(ql)
    off = np.zeros(len(lst) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in lst])
    seq = np.concatenate(lst).astype(np.uint8) if off[-1] else np.zeros(1, dtype=np.uint8)
    return names, qlens, np.ascontiguousarray(seq), off, np.array(seeds, dtype=np.uint32), bool(mate2)
