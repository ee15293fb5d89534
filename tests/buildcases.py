"""The index builder's corner cases (centrifuge_amd/csrc/cf_build.hip, cf_prims.hpp): tiny texts, side / word / sample / ftab /
boundary-mark / chunk / scan edges.  tests/golden/make_build_golden.py runs the unmodified reference builder over every case and
records what it writes in tests/golden/build_edges.json; tests/test_build_cases.py checks, without a device, that every case still
sits on the edge it claims; tests/test_gpu_build_edges.py builds each accepted case on the GPU and compares with the record.

A case is a name and a deterministic recipe: FASTA records out of seeded numpy generators or literal bytes, the build options
(off_rate, ftab_chars, chunk_suffixes, CF_BUILD_ROUNDS) and a claim about the joined text (`claim`).  Seeds that were
searched for (a '$' row on a side edge, say) are literals here, found with find_seed(); the claim fails when they drift."""
import hashlib
import os

import numpy as np

import synth

LUT = np.full(256, 4, dtype=np.uint8)
for _ch, _v in zip(b"ACGT", range(4)):
    LUT[_ch] = _v

SIDE_ROWS, WORD_ROWS = 384, 32          # rows per side / per packed word (kb_side_words)
REF_OVERLAP = 11                        # kRefOverlap
BIN_CHARS, KEY_CHARS = 12, 29           # kBinChars, kKeyChars
SCAN_TILE, SCAN_CARRY = 2048, 256 * 2048  # cf_prims.hpp: items per tile, items per carry step of kp_scan_tiles


# ------------------------------------------------------------------ helpers
def rand(seed, n):
    """n random bases as bytes"""
    return synth.ACGT[np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)].tobytes()


def joined(records):
    """the joined text the builder sorts: the A/C/G/T of all records, as codes 0..3"""
    c = LUT[np.frombuffer(b"".join(s for _, s in records), dtype=np.uint8)]
    return np.ascontiguousarray(c[c < 4])


def suffix_array(codes):
    """brute force, for texts of a few thousand bases: the starts of the n + 1 suffixes in the builder's row order — the
    terminator sorts AFTER every base (sortKey in cf_build.hip), so the empty suffix is the last row"""
    t = np.append(np.asarray(codes, dtype=np.uint8), np.uint8(4)).tobytes()
    assert len(t) <= 20001, "brute force only"
    return np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.int64)


def z_off(codes):
    """the row of the whole text: where the BWT holds '$'"""
    return int(np.nonzero(suffix_array(codes) == 0)[0][0])


def find_seed(n, pred, start=0, limit=200000):
    """first seed >= start whose n random bases satisfy pred(codes): how the literal seeds below were chosen"""
    for s in range(start, start + limit):
        if pred(joined([(b"", rand(s, n))])):
            return s
    raise ValueError("no seed found")


def padded_kmers(codes, k):
    """the k-mer at every position 0 .. n of the text padded with T, as integers: kb_hist's bins for k = 12"""
    c = np.concatenate([np.asarray(codes, dtype=np.uint64), np.full(k, 3, dtype=np.uint64)])
    n = len(codes)
    v = np.zeros(n + 1, dtype=np.uint64)
    for j in range(k):
        v = (v << np.uint64(2)) | c[j:j + n + 1]
    return v


def max_bin12(codes):
    """the largest count of a 12-mer prefix bin (kb_hist over positions 0 .. n)"""
    return int(np.unique(padded_kmers(codes, BIN_CHARS), return_counts=True)[1].max())


def tied_slots(codes):
    """how many suffixes share their first sort key (29 bases + end mark) with another one: m of the first refinement round"""
    n = len(codes)
    rem = np.minimum(n - np.arange(n + 1), KEY_CHARS).astype(np.uint64)
    key = (padded_kmers(codes, KEY_CHARS) << np.uint64(6)) | (np.uint64(KEY_CHARS) - rem)
    cnt = np.unique(key, return_counts=True)[1]
    return int(cnt[cnt > 1].sum())


# ------------------------------------------------------------------ the case
class Case:
    def __init__(self, name, make, claim, n=None, off_rate=4, ftab_chars=10, chunk=0, rounds=None, vias=("fasta", "memory"), may_refuse=False):
        """make() -> [sequence bytes, ...]; claim(case) -> bool, what the case is here for; n: the joined length it must have;
        chunk: suffixes per pass, or "max_bin" = the largest 12-mer bin count of the text; rounds: CF_BUILD_ROUNDS or None;
        may_refuse: the reference builder may refuse the input (the record says whether it did)"""
        self.name, self.group, self._make, self.claim, self.n = name, name[0].upper(), make, claim, n
        self.off_rate, self.ftab_chars, self._chunk, self.rounds, self.may_refuse = off_rate, ftab_chars, chunk, rounds, may_refuse
        self.vias = vias
        self._rec = self._codes = None

    @property
    def records(self):
        if self._rec is None:
            self._rec = [(b"seq%d synthetic genome %d" % (i, i), s) for i, s in enumerate(self._make())]
        return self._rec

    @property
    def codes(self):
        if self._codes is None:
            self._codes = joined(self.records)
        return self._codes

    @property
    def has_gaps(self):
        return any(LUT[np.frombuffer(s, dtype=np.uint8)].max(initial=0) > 3 for _, s in self.records)

    @property
    def chunk_suffixes(self):
        return max_bin12(self.codes) if self._chunk == "max_bin" else self._chunk

    @property
    def env(self):
        return {} if self.rounds is None else {"CF_BUILD_ROUNDS": self.rounds}

    @property
    def ref_args(self):
        """the reference builder's options of the case"""
        return ["-o", str(self.off_rate), "-t", str(self.ftab_chars)]

    def build_kwargs(self):
        return dict(off_rate=self.off_rate, ftab_chars=self.ftab_chars, chunk_suffixes=self.chunk_suffixes)

    def fasta_bytes(self):
        out = []
        for nm, s in self.records:
            out.append(b">" + nm + b"\n")
            out += [s[p:p + 70] + b"\n" for p in range(0, len(s), 70)]
        return b"".join(out)

    def fasta_sha256(self):
        return hashlib.sha256(self.fasta_bytes()).hexdigest()

    def write(self, d):
        """genomes.fa, conv.tsv, nodes.dmp, names.dmp into d -> keyword arguments of the taxonomy files for capi.build_index"""
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "genomes.fa"), "wb") as f:
            f.write(self.fasta_bytes())
        synth.write_taxonomy(d, len(self.records), genus_size=3)
        return dict(conversion_table=os.path.join(d, "conv.tsv"), taxonomy_tree=os.path.join(d, "nodes.dmp"), name_table=os.path.join(d, "names.dmp"))

    def memory(self):
        """codes / seq_off / seq_names of the records for capi.build_index (gap-free cases)"""
        seqs = [LUT[np.frombuffer(s, dtype=np.uint8)] for _, s in self.records]
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        return dict(codes=np.concatenate(seqs), seq_off=off, seq_names=[nm for nm, _ in self.records])

    def starts(self):
        """joined start of every record that holds a base"""
        out, tot = [], 0
        for _, s in self.records:
            b = int((LUT[np.frombuffer(s, dtype=np.uint8)] < 4).sum())
            if b:
                out.append(tot)
            tot += b
        return out


CASES = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _z(c):
    return z_off(c.codes)


# ---- A. tiny texts: shorter than the ftab width (nShort = min(ftabChars, n + 1)), than the 11 bases of the sample's overlap
# (the adj >= n fix-ups of emitRow), than a 12-mer bin and a 29-mer key (end marks), than one packed word (window())
for _i, _L in enumerate((1, 2, 9, 10, 11, 12, 28, 29, 30, 31, 32, 33)):
    _add("a_len%d" % _L, lambda L=_L, i=_i: [rand(100 + i, L)], lambda c: True, n=_L, may_refuse=True)
_add("a_2x5", lambda: [rand(120, 5), rand(121, 5)], lambda c: c.starts() == [0, 5], n=10, may_refuse=True)
_add("a_3x5", lambda: [rand(122, 5), rand(123, 5), rand(124, 5)], lambda c: c.starts() == [0, 5, 10], n=15, may_refuse=True)

# ---- B. side and word edges: numSides = ((n/4 + 1) + 95) / 96, 384 rows a side, 32 a word; kb_side_words leaves the '$' row
# out of its count.  The seeds of the b_z* cases were found with find_seed(1000, ...) on the claim.  Row n always holds the
# empty suffix (the terminator sorts last), so the last row '$' can stand on is n - 1: b_z_last.
for _i, _n1 in enumerate((383, 384, 385, 767, 768, 769)):
    _add("b_rows%d" % _n1, lambda L=_n1 - 1, i=_i: [rand(200 + i, L)], lambda c: True, n=_n1 - 1)
for _i, _L in enumerate((31, 32, 33)):
    _add("b_len%d" % _L, lambda L=_L, i=_i: [rand(210 + i, L)], lambda c: True, n=_L)
B_SEEDS = {"b_z_side_first": 1074, "b_z_side_last": 1120, "b_z_word_first": 1006, "b_z_word_last": 1062, "b_z_row0": 3806, "b_z_last": 1637}
B_CLAIMS = {
    "b_z_side_first": lambda z, n: z > 0 and z % SIDE_ROWS == 0,
    "b_z_side_last": lambda z, n: z % SIDE_ROWS == SIDE_ROWS - 1,
    "b_z_word_first": lambda z, n: z % WORD_ROWS == 0 and z % SIDE_ROWS != 0,
    "b_z_word_last": lambda z, n: z % WORD_ROWS == WORD_ROWS - 1 and z % SIDE_ROWS != SIDE_ROWS - 1,
    "b_z_row0": lambda z, n: z == 0,
    "b_z_last": lambda z, n: z == n - 1,
}
for _nm in B_SEEDS:
    _add(_nm, lambda nm=_nm: [rand(B_SEEDS[nm], 1000)], lambda c, nm=_nm: B_CLAIMS[nm](_z(c), len(c.codes)), n=1000)

# ---- C. SA sample: row & ((1 << offRate) - 1), offsLen = ceil((n + 1) / 2^offRate).  3,000 bases: 2^12 and 2^20 exceed the
# row count, so row 0 alone is sampled
for _o in (0, 1, 3, 7, 12, 20):
    _add("c_rate%d" % _o, lambda: [rand(300, 3000)], lambda c: (len(c.codes) + 1 < (1 << c.off_rate)) == (c.off_rate >= 12), n=3000, off_rate=_o)
C_Z_SEED = 2005                          # find_seed(3000, z % 32 == 0 and z > 0)
_add("c_z_sampled", lambda: [rand(C_Z_SEED, 3000)], lambda c: _z(c) > 0 and _z(c) % (1 << c.off_rate) == 0, n=3000, off_rate=5)
_add("c_rows_multiple", lambda: [rand(301, 3007)], lambda c: (len(c.codes) + 1) % (1 << c.off_rate) == 0, n=3007, off_rate=6)

# every row sampled, on texts whose last sequences are shorter than the 11 bases of the sample's overlap: each `adj >= n` fix-up of
# emitRow then decides between two sequences (at the default rate a tiny text has one or two sampled rows, and they rarely do)
_add("c_3x5_rate0", lambda: [rand(122, 5), rand(123, 5), rand(124, 5)], lambda c: c.starts() == [0, 5, 10], n=15, off_rate=0)
_add("c_short_tail_rate0", lambda: [rand(310, 200), rand(311, 4), rand(312, 3)],
     lambda c: c.starts() == [0, 200, 204] and len(c.codes) - c.starts()[1] < REF_OVERLAP, n=207, off_rate=0)

# ---- D. ftab width: sh = 2 * (12 - ftabChars); short suffixes leave their T-padded bin again and are absorbed into the next
# populated transition (eftab)
for _t in (1, 2, 5, 11, 12):
    _add("d_ftab%d" % _t, lambda: [rand(400, 3000)], lambda c: True, n=3000, ftab_chars=_t)


def _t_run(seed, run):
    """1,000 bases that end in exactly `run` T"""
    body = bytearray(rand(seed, 1000 - run))
    if body[-1:] == b"T":
        body[-1:] = b"G"
    return bytes(body) + b"T" * run


def _ends_in_t(c, run):
    t = c.codes
    return bool((t[len(t) - run:] == 3).all()) and t[len(t) - run - 1] != 3


for _t in (2, 10):
    for _run in sorted({1, _t - 1, _t, _t + 1}):
        _add("d_ftab%d_trun%d" % (_t, _run), lambda r=_run: [_t_run(410 + r, r)], lambda c, r=_run: _ends_in_t(c, r), n=1000, ftab_chars=_t)
for _r in (1, 24):
    _add("d_all_t_rounds%d" % _r, lambda: [b"T" * 500], lambda c: bool((c.codes == 3).all()), n=500, rounds=_r)
    _add("d_all_a_rounds%d" % _r, lambda: [b"A" * 500], lambda c: bool((c.codes == 0).all()), n=500, rounds=_r)
    _add("d_acgt_rounds%d" % _r, lambda: [b"ACGT" * 125], lambda c: bool((c.codes == np.arange(500) % 4).all()), n=500, rounds=_r)

# ---- E. boundary marks: marks[start < 11 ? 0 : start - 11] = sequence, later sequences overwrite
_add("e_marks_collide", lambda: [rand(500, 3), rand(501, 4), rand(502, 4), rand(503, 200)],
     lambda c: c.starts() == [0, 3, 7, 11] and all(max(0, s - REF_OVERLAP) == 0 for s in c.starts()), n=211)
for _s in (10, 11, 12):
    _add("e_start%d" % _s, lambda s=_s: [rand(510 + s, s), rand(530 + s, 200)], lambda c, s=_s: c.starts() == [0, s], n=_s + 200)
_add("e_leading_n", lambda: [b"N" * 17 + rand(540, 150), rand(541, 60)], lambda c: c.records[0][1].startswith(b"N") and c.starts() == [0, 150],
     n=210, vias=("fasta",))
_add("e_all_n_between", lambda: [rand(550, 6), b"N" * 25, rand(551, 7)], lambda c: c.starts() == [0, 6] and len(c.records) == 3,
     n=13, vias=("fasta",), may_refuse=True)
# the same all-N record between sequences long enough for the reference builder
_add("e_all_n_between_long", lambda: [rand(552, 120), b"N" * 25, rand(553, 130)], lambda c: c.starts() == [0, 120] and len(c.records) == 3,
     n=250, vias=("fasta",))

# ---- F. sequence count: the SA sample is u16 up to 65,535 sequences and u32 beyond (nPat > 65535)
for _k in (65535, 65536):
    _add("f_seqs%d" % _k, lambda k=_k: [bytes(r) for r in synth.make_genomes(k, 40, genus_size=8, seed=600)],
         lambda c, k=_k: len(c.records) == k, n=40 * _k, vias=("memory",))


# ---- G. chunk plan: `cnt > 0 && cnt + bins[b] > chunkMax` with one suffix per pass, and with a pass that a bin fills exactly.
# The text repeats a 60-base piece five times, so that the fullest 12-mer bin holds 5 suffixes
def _g_text():
    r = rand(700, 2700)
    piece = rand(701, 60)
    return [b"".join(r[540 * k:540 * (k + 1)] + piece for k in range(5))]


_add("g_chunk1", _g_text, lambda c: max_bin12(c.codes) >= 5, n=3000, chunk=1)
_add("g_chunk_max_bin", _g_text, lambda c: c.chunk_suffixes == max_bin12(c.codes) >= 5, n=3000, chunk="max_bin")

# ---- H. scan edges through the builder.  A text of one chunk holds n + 1 suffixes; the builder's first device_scan runs over
# cnt + 1 = n + 2 items (the tie flags and one trailing zero), so that call meets a full tile (2,048 items) at n + 1 = 2,047 and
# the carry step of kp_scan_tiles (256 tiles = 524,288 items) at n + 1 = 524,287: the rows below hold n + 1 = 2,046 ... 2,049 and
# 524,286 ... 524,289, one to either side of the edge for n + 2 as well as for n + 1.
for _n1 in (2046, 2047, 2048, 2049, 524286, 524287, 524288, 524289):
    _add("h_rows%d" % _n1, lambda L=_n1 - 1: [rand(800, L)], lambda c: True, n=_n1 - 1)
# The tie scans (group ids over m slots inclusive, compaction over m + 1 exclusive) see the number of tied suffixes: a
# 300,000-base exact duplicate ties about 600,000 of them, beyond the carry step ...
_add("h_dup300k", lambda: [rand(810, 300000) + rand(811, 100000) + rand(810, 300000) + rand(812, 1000)], lambda c: tied_slots(c.codes) > SCAN_CARRY, n=701000)
# ... and a duplicate of H_DUP bases (chosen with tied_slots) ties 524,288 exactly: the inclusive scan ends on the carry edge, the
# exclusive one a single item beyond it
H_DUP = 262172


def _h_dup_text():
    x = rand(820, H_DUP)
    return [x + rand(821, 1000) + x + rand(822, 1000)]


_add("h_dup_ties524288", _h_dup_text, lambda c: tied_slots(c.codes) == SCAN_CARRY, n=2 * H_DUP + 2000)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]


# ------------------------------------------------------------------ the reference's record (tests/golden/build_edges.json)
GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_edges.json")


def file_digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 22), b""):
            h.update(blk)
    return {"size": os.path.getsize(path), "sha256": h.hexdigest()}


def index_digest(base):
    """size and sha256 of <base>.{1,2,3,4}.cf"""
    return {ext: file_digest("%s.%s.cf" % (base, ext)) for ext in "1234"}


def run_reference(case, d, threads=4):
    """the case's inputs into d and the compiled reference builder over them -> what build_edges.json holds of the case"""
    import subprocess
    from oracle import oracle as O
    case.write(d)
    try:
        O.ref_build(d, threads=threads, extra=case.ref_args)
        status = 0
    except subprocess.CalledProcessError as e:
        status = e.returncode
    rec = {"fasta_sha256": case.fasta_sha256(), "args": case.ref_args, "exit": status}
    if status == 0:
        rec["files"] = index_digest(os.path.join(d, "idx"))
    return rec


def load_golden():
    import json
    with open(GOLDEN_JSON) as f:
        return json.load(f)["cases"]


def accepted_names():
    g = load_golden()
    return [n for n in NAMES if g[n]["exit"] == 0]


def sections_1cf(path):
    """[(name, first offset)] of the sections of a .1.cf as writeIndexFiles lays them out (cf_build.hip)"""
    raw = open(path, "rb").read(64)
    n = int(np.frombuffer(raw, dtype="<u8", count=1, offset=4)[0])
    ftab_chars = int(np.frombuffer(raw, dtype="<i4", count=1, offset=24)[0])
    npat = int(np.frombuffer(raw, dtype="<u8", count=1, offset=32)[0])
    o = 40
    out = [("header", 0), ("plen", o)]
    o += 8 * npat
    with open(path, "rb") as f:
        f.seek(o)
        nfrag = int(np.frombuffer(f.read(8), dtype="<u8")[0])
    out.append(("rstarts", o))
    o += 8 + 24 * nfrag
    out.append(("sides", o))
    o += ((n // 4 + 1 + 95) // 96) * 128
    out.append(("zOff/fchr", o))
    o += 48
    out.append(("ftab", o))
    o += 8 * ((1 << (2 * ftab_chars)) + 1)
    out.append(("eftab", o))
    o += 16 * ftab_chars
    out.append(("names", o))
    return out


def first_difference(ref_base, our_base):
    """where the first differing file of two indexes differs, with the section of .1.cf it falls in"""
    for ext in "1234":
        a, b = np.fromfile("%s.%s.cf" % (ref_base, ext), dtype=np.uint8), np.fromfile("%s.%s.cf" % (our_base, ext), dtype=np.uint8)
        m = min(len(a), len(b))
        bad = np.nonzero(a[:m] != b[:m])[0]
        if len(bad) == 0 and len(a) == len(b):
            continue
        at = int(bad[0]) if len(bad) else m
        msg = ".%s.cf: reference %d bytes, ours %d, first difference at offset %d" % (ext, len(a), len(b), at)
        if ext == "1":
            sec = [nm for nm, o in sections_1cf("%s.1.cf" % ref_base) if o <= at][-1]
            first = dict(sections_1cf("%s.1.cf" % ref_base))[sec]
            msg += " (section %s, byte %d of it)" % (sec, at - first)
        return msg
    return "no difference"
