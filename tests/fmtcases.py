"""The formatter of the device text path (fmt_size_body / fmt_write_body and fmt_cols_size_body / fmt_cols_write_body,
centrifuge_amd/csrc/cf_textio.hpp): ONE table of synthetic batches and what they print, read by the CPU harness
(tests/test_textcols_emu.py: the one-lane build and wavefronts of 64 lanes) and by the device (tests/test_gpu_fmtcases.py, through
the tap cf_debug_format).  What a batch prints is stated in plain Python — expected(), the host's general formatter formatRange
(cf_cli.cpp; the reference: aln_sink.h:2279-2337, readID aln_sink.h:2203-2217), and tally(), SpeciesMetrics::addSpeciesCounts
(aln_sink.h:142-172) — and never taken from a run of the code under test.

A runner is a callable (world, batch, cols, default_bodies, out_cap, tuples_cap) -> (the room's out_cap bytes with UNWRITTEN where
nothing was written, bytes per query, the bytes the size pass summed, single, the tuple words that fit, the words all tuples need):
emu_cols.format_full and capi.debug_format behind a two-line adapter."""
import numpy as np

(READ_ID, SEQ_ID, TAX_ID, TAX_RANK, TAX_NAME, SCORE, SCORE2, HIT_LEN, QUERY_LEN, NUM_MATCHES,
 SEQ, QUAL, SEQ1, QUAL1, SEQ2, QUAL2, PLACEHOLDER, ZERO) = range(18)
NAMES = {"readID": READ_ID, "seqID": SEQ_ID, "taxID": TAX_ID, "taxRank": TAX_RANK, "taxLevel": TAX_RANK, "taxName": TAX_NAME, "score": SCORE,
         "2ndBestScore": SCORE2, "hitLength": HIT_LEN, "queryLength": QUERY_LEN, "numMatches": NUM_MATCHES, "readSeq": SEQ, "readQual": QUAL,
         "readSeq1": SEQ1, "readQual1": QUAL1, "readSeq2": SEQ2, "readQual2": QUAL2, "SEQ1": SEQ1, "QUAL1": QUAL1, "SEQ2": SEQ2, "QUAL2": QUAL2,
         "QNAME": READ_ID, "FLAG": ZERO, "RNAME": TAX_ID, "POS": ZERO, "MAPQ": ZERO, "CIGAR": PLACEHOLDER, "RNEXT": SEQ_ID, "PNEXT": ZERO,
         "TLEN": QUERY_LEN, "SEQ": SEQ, "QUAL": QUAL}
DEFAULT = [READ_ID, SEQ_ID, TAX_ID, SCORE, SCORE2, HIT_LEN, QUERY_LEN, NUM_MATCHES]
LIST_A = [NAMES[n] for n in "readID,taxID,taxRank,taxName,numMatches,readSeq,readQual".split(",")]                    # tests/test_gpu_cli.py:46
LIST_B = [NAMES[n] for n in "QNAME,CIGAR,FLAG,RNAME,RNEXT,TLEN,SEQ1,QUAL2,readSeq2,taxLevel".split(",")]             # tests/test_gpu_cli.py:48
SAM = [NAMES[n] for n in "QNAME,FLAG,RNAME,POS,MAPQ,CIGAR,RNEXT,PNEXT,TLEN,SEQ,QUAL".split(",")]
WIDE32 = (DEFAULT + [TAX_RANK, TAX_NAME, SEQ, QUAL, SEQ1, QUAL1, SEQ2, QUAL2, PLACEHOLDER, ZERO]) * 2
WIDE32 = WIDE32[:32]
PROGRAMS = [[c] for c in range(18)] + [[SEQ, SEQ, TAX_ID, TAX_ID, QUAL1, QUAL1], LIST_A, LIST_B, SAM, WIDE32, DEFAULT]
LONG = [READ_ID, SEQ, QUAL, SCORE]          # a program with long fields, for the groups that run "the default bodies and a program with long fields"
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 250]
NEVER = 0xffffffff
UNWRITTEN = 0x5A
BODIES = "the default bodies"               # in place of a column list: fmt_size_body / fmt_write_body
# the parameters of the tests both files run
TAIL_COUNTS = [1, 63, 64, 65, 130, 255, 256, 257, 256 + 65]                         # a wavefront's tail; a block of four wavefronts and its tail
TAIL_ROWS = [0, 1, 5]


def make_world(uids=None, taxa=None, seqid_rank=None, leaf=None, ranks=None, names=None, idx_zero=1):
    """a classifier's string tables: four references, six dense taxa (tax ID 0 among them: the reads without rows are counted there)"""
    uids = uids or [b"gi|4", b"NC_000913.3", b"r2", b"chr"]
    taxa = taxa or [9646, 0, 562, (7 << 32) | 12, 40674, 2]
    seqid_rank = seqid_rank or [b"species", b"no rank", b"species", b"leaf", b"class", b"superkingdom"]
    leaf = leaf or [1, 0, 1, 1, 0, 0]
    ranks = ranks or [b"species", b"no rank", b"species", b"subspecies", b"class", b"superkingdom"]
    names = names or [b"Ailuropoda melanoleuca", b"", b"Escherichia coli", b"a strain of it", b"Mammalia", b"Bacteria"]

    def table(items):
        off, s = [0], b""
        for x in items:
            s += x
            off.append(len(s))
        return s, off
    s1, uid_off = table(uids)
    s2, rank_off = table(seqid_rank)
    tax_txt = [(b"%d" % (t & 0xffffffff)) + ((b".%d" % (t >> 32)) if t >> 32 else b"") for t in taxa]
    s3, tax_off = table(tax_txt)
    # (behind the last taxon: tax ID 0's rank and name, what an unclassified row prints)
    t1, trank_off = table(ranks + [b"no rank"])
    t2, tname_off = table(names + [b"root-less"])
    w = dict(strs=s1 + s2 + s3, uidOff=uid_off, rankOff=[o + len(s1) for o in rank_off], taxOff=[o + len(s1) + len(s2) for o in tax_off],
             taxLeaf=leaf, nRefs=len(uids), nTaxa=len(taxa), idxZero=idx_zero, taxStrs=t1 + t2, trankOff=trank_off, tnameOff=[o + len(t1) for o in tname_off])
    w.update(uids=uids, taxTxt=tax_txt, seqidRank=seqid_rank, ranks=ranks + [b"no rank"], names=names + [b"root-less"])
    return w


WORLD = make_world()
# ... with an empty uid, a tax ID whose two fields are both at full width, an empty rank string
WORLD_EDGE = make_world(uids=[b"gi|4", b"", b"r2", b"chr", b"u" * 70], taxa=[9646, 0, (0xffffffff << 32) | 0xffffffff, (7 << 32) | 12, 40674, 4294967295],
                        seqid_rank=[b"species", b"no rank", b"", b"leaf", b"class", b"superkingdom"])
# ... with 70 taxa: every query of a wavefront can name another one
WORLD_WIDE = make_world(uids=[b"ref%d" % i for i in range(70)], taxa=[0] + [1000 + 7 * i for i in range(1, 70)], seqid_rank=[b"rank%d" % (i % 5) for i in range(70)],
                        leaf=[i % 2 for i in range(70)], ranks=[b"r%d" % (i % 3) for i in range(70)], names=[b"taxon %d" % i for i in range(70)], idx_zero=0)


def read_id(name):
    """aln_sink.h:2203-2217: a trailing /1 /2 /3 goes, then the name up to the first white space"""
    if len(name) >= 2 and name[-2:-1] == b"/" and name[-1:] in (b"1", b"2", b"3"):
        name = name[:-2]
    for i, ch in enumerate(name):
        if ch in b" \t\n\v\f\r":
            return name[:i]
    return name


def make_block(names, seqs, quals, fastq, wrap_lower):
    """the text of a block and, per record, what the record pass leaves: places of the readID and the quality line, the length"""
    text, id_off, id_len, qual_off = b"", [], [], []
    for i, (nm, sq) in enumerate(zip(names, seqs)):
        text += b"@" if fastq else b">"
        id_off.append(len(text)); id_len.append(len(read_id(nm)))
        text += nm + b"\n"
        if fastq:
            text += sq + b"\n+" + (nm if i % 3 == 0 else b"") + b"\n"
            qual_off.append(len(text))
            text += quals[i] + b"\n"
        else:
            s = sq.lower() if wrap_lower and i % 2 else sq
            if wrap_lower:
                s = b"\n".join(s[k:k + 60] for k in range(0, len(s), 60))
            text += s + b"\n"
    return text, id_off, id_len, qual_off


def pack(seqs):
    """2-bit words and N masks, ceil(len / 32) per read (an N: code 0, its mask bit set)"""
    words, masks = [], []
    for s in seqs:
        for k in range(0, len(s), 32):
            w = m = 0
            for j, ch in enumerate(s[k:k + 32]):
                if ch == ord("N"):
                    m |= 1 << j
                else:
                    w |= b"ACGT".index(bytes([ch])) << (2 * j)
            words.append(w); masks.append(m)
    return np.array(words, dtype=np.uint64), np.array(masks, dtype=np.uint32)


def assemble(names, seqs, quals, paired, fastq, wrap_lower, rows, score2, max_score):
    """a batch from its reads (names, bases, qualities or None) and its queries (rows: per query a list of (uniqueID, dense taxon, score,
    hitLength); score2 and maxScore per query)"""
    n_reads = len(seqs)
    if paired:
        # two blocks in one buffer, the second at a 4096-byte boundary behind the first (the places count from the buffer's start)
        a = make_block(names[0::2], seqs[0::2], quals[0::2] if fastq else None, fastq, wrap_lower)
        b = make_block(names[1::2], seqs[1::2], quals[1::2] if fastq else None, fastq, wrap_lower)
        at2 = (len(a[0]) + 128 + 4095) & ~4095
        text = a[0] + bytes(at2 - len(a[0])) + b[0]
        def mates(x, y):
            m = [None] * n_reads
            m[0::2], m[1::2] = x, y
            return m
        id_off, id_len = mates(a[1], [v + at2 for v in b[1]]), mates(a[2], b[2])
        qual_off = mates(a[3], [v + at2 for v in b[3]]) if fastq else []
    else:
        text, id_off, id_len, qual_off = make_block(names, seqs, quals, fastq, wrap_lower)
    rlen = [len(s) for s in seqs]
    bases, nmask = pack(seqs)
    flat = [r for rs in rows for r in rs]
    b = dict(text=text, idOff=id_off, idLen=id_len, rlen=rlen, qualOff=qual_off if fastq else None, bases=bases, nmask=nmask,
             rows=np.array(flat, dtype=np.uint32).reshape(-1, 4), qinfo=[len(rs) | 0x40 for rs in rows], score2=list(score2), maxScore=list(max_score), paired=paired)
    b.update(names=names, seqs=seqs, quals=quals)
    return b


def make_batch(nq, rows_per_query, paired, fastq, seed, wrap_lower=False, id_extra=0, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    per = 2 if paired else 1
    n_reads = nq * per
    seqs = []
    for r in range(n_reads):
        n = lengths[(r + seed) % len(lengths)]
        s = bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)))
        # an N at the first base, at the two sides of a word boundary, at the last base — and a read of nothing else now and then
        for p in ((0,), (31, 32), (n - 1,), (), ())[r % 5]:
            if p < n:
                s[p] = ord("N")
        if r % 37 == 11:
            s = bytearray(b"N" * n)
        seqs.append(bytes(s))
    names = []
    for r in range(n_reads):
        base = b"r%d" % (r // per) + (b"x" * id_extra if r == 0 else b"") + b"y" * (r % 3)
        names.append(base + ((b"/%d" % (r % per + 1)) if paired else (b"/3" if r % 11 == 5 else b"")) + (b" a comment/2" if r % 7 == 3 else b""))
    quals = [bytes(rng.integers(33, 127, len(s), dtype=np.uint8)) for s in seqs] if fastq else None
    # rows: rows_per_query of them (0: unclassified), or a mix
    rows, score2, max_score = [], [], []
    for q in range(nq):
        n = rows_per_query if rows_per_query >= 0 else (0, 1, 5, 2)[q % 4]
        ms = int(rng.integers(1, 40000)) if q % 9 else NEVER
        perfect = q % 2 == 0
        mine = []
        for i in range(n):
            t = int(rng.integers(0, WORLD["nTaxa"]))
            mine.append((int(rng.integers(0, WORLD["nRefs"] + 2)), t, ms if perfect and ms != NEVER else int(rng.integers(0, max(1, min(ms, 99999)))), int(rng.integers(0, 500))))
        rows.append(mine)
        score2.append(int(rng.integers(0, 3)) * int(rng.integers(0, 100000)))
        max_score.append(ms)
    return assemble(names, seqs, quals, paired, fastq, wrap_lower, rows, score2, max_score)


def expected_rows(b, cols, world=None):
    """formatRange (cf_cli.cpp) in plain Python: per query the bytes of its rows"""
    W, out, per, first = world or WORLD, [], 2 if b["paired"] else 1, 0
    for q in range(len(b["qinfo"])):
        n = b["qinfo"][q] & 0x3f
        ra, rb = q * per, q * per + 1
        seq = lambda r: b["seqs"][r]
        qual = lambda r: b["quals"][r] if b["quals"] is not None else b"I" * len(b["seqs"][r])
        qlen = len(seq(ra)) + (len(seq(rb)) if b["paired"] else 0)
        mine = []
        for i in range(max(1, n)):
            uncl = n == 0
            uid, t, score, hit = (0, W["nTaxa"], 0, 0) if uncl else [int(v) for v in b["rows"][first + i]]
            if not uncl and t >= W["nTaxa"]:
                t = 0       # the kernels print dense taxon 0 for a taxon index the index does not have; the reference has no such row
            fields = []
            for c in cols:
                if c == READ_ID: v = read_id(b["names"][ra])
                elif c == SEQ_ID: v = b"unclassified" if uncl else (W["uids"][uid] if W["taxLeaf"][t] and uid < W["nRefs"] else W["seqidRank"][t])
                elif c == TAX_ID: v = b"0" if uncl else W["taxTxt"][t]
                elif c == TAX_RANK: v = W["ranks"][t]
                elif c == TAX_NAME: v = W["names"][t]
                elif c == SCORE: v = b"%d" % score
                elif c == SCORE2: v = b"%d" % b["score2"][q]
                elif c == HIT_LEN: v = b"%d" % hit
                elif c == QUERY_LEN: v = b"%d" % qlen
                elif c == NUM_MATCHES: v = b"%d" % max(1, n)
                elif c == SEQ: v = seq(ra) + (b"_" + seq(rb) if b["paired"] else b"")
                elif c == QUAL: v = qual(ra) + (b"_" + qual(rb) if b["paired"] else b"")
                elif c == SEQ1: v = seq(ra)
                elif c == QUAL1: v = qual(ra)
                elif c == SEQ2: v = seq(rb) if b["paired"] else b""
                elif c == QUAL2: v = qual(rb) if b["paired"] else b""
                elif c == PLACEHOLDER: v = b"*0"
                elif c == ZERO: v = b"0"
                fields.append(v)
            mine.append(b"\t".join(fields) + b"\n")
        out.append(b"".join(mine))
        first += n
    return out


def expected(b, cols, world=None):
    return b"".join(expected_rows(b, cols, world))


def tally(b, world=None):
    """SpeciesMetrics::addSpeciesCounts (aln_sink.h:142-172), the part that is not in the per-taxon counters, in plain Python: a
    query without rows counts under tax ID 0's dense taxon; a query all of whose rows score the read's best possible score is a
    perfect assignment — one row: counted under its taxon, several: a tuple of their taxa.  -> single (nTaxa + 1 words), the tuples sorted"""
    W, first = world or WORLD, 0
    single, tuples = np.zeros(W["nTaxa"] + 1, dtype=np.uint64), []
    for q in range(len(b["qinfo"])):
        n, ms = b["qinfo"][q] & 0x3f, b["maxScore"][q]
        rows = [[int(v) for v in r] for r in b["rows"][first:first + n]]
        first += n
        if n == 0:
            single[W["idxZero"]] += 1
        elif ms != NEVER and all(score >= ms and t < W["nTaxa"] for _, t, score, _ in rows):
            if n == 1:
                single[rows[0][1]] += 1
            else:
                tuples.append(tuple(t for _, t, _, _ in rows))
    return single, sorted(tuples)


def first_diff(a, b):
    for i in range(min(len(a), len(b))):
        if a[i] != b[i]:
            return "byte %d: got %r, want %r" % (i, a[max(0, i - 30):i + 30], b[max(0, i - 30):i + 30])
    return "lengths %d / %d; got ends %r, want ends %r" % (len(a), len(b), a[-40:], b[-40:])


def split_tuples(t, whole=True):
    """the tuples of a list of tuple words; not whole: the list may end in words nothing wrote (a tuple that did not fit leaves none)"""
    out, i = [], 0
    while i < len(t):
        if not whole and int(t[i]) == 0x5A5A5A5A:
            assert all(int(v) == 0x5A5A5A5A for v in t[i:]), "a tuple word behind the last whole tuple"
            return out
        out.append(tuple(int(v) for v in t[i + 1:i + 1 + t[i]]))
        i += 1 + int(t[i])
    assert i == len(t)
    return out


def check(run, b, cols, world=None, out_cap=None, tuples_cap=None):
    """one batch through one runner, everything it returns against the Python statements.  cols: a column list, or BODIES.
    out_cap: the room (None: exactly the text); rows that fit are there, every other byte of the room is UNWRITTEN.  -> the text"""
    W = world or WORLD
    prog = DEFAULT if cols is BODIES else cols
    per_query = expected_rows(b, prog, W)
    want = b"".join(per_query)
    cap = len(want) if out_cap is None else out_cap
    text, sizes, total, single, tuples, tuple_words = run(W, b, [] if cols is BODIES else cols, cols is BODIES, cap, tuples_cap)
    assert total == len(want), "the size pass summed %d bytes, the rows take %d" % (total, len(want))
    assert [int(s) for s in sizes] == [len(r) for r in per_query]
    assert len(text) == cap
    room, at = bytearray([UNWRITTEN]) * cap, 0
    for r in per_query:
        if at + len(r) <= cap:
            room[at:at + len(r)] = r
        at += len(r)
    assert text == bytes(room), first_diff(text, bytes(room))
    want_single, want_tuples = tally(b, W)
    assert np.array_equal(single, want_single), "single: %r, want %r" % (list(single), list(want_single))
    need = sum(len(t) + 1 for t in want_tuples)
    assert tuple_words == need
    if tuples_cap is None or tuples_cap >= need:
        assert sorted(split_tuples(tuples)) == want_tuples
    else:
        # the tuples that fit are whole and are tuples of the batch; the first one left out would not have fitted
        assert len(tuples) == tuples_cap
        got, left = split_tuples(tuples, whole=False), list(want_tuples)
        for t in got:
            assert t in left, "tuple %r is none of the batch's (or there twice)" % (t,)
            left.remove(t)
        used = sum(len(t) + 1 for t in got)
        assert left and used <= tuples_cap < used + max(len(t) + 1 for t in left)
    return want


def check_case(run, case):
    return check(run, case[1], case[3], case[2], case[4], case[5])


# ---- the groups of cases beyond the random batches: each case is (id, batch, world, cols, out_cap or None, tuples_cap or None)
DIGITS = [0] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [4294967295]


def _reads(rng, lens, fastq):
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n)) for n in lens]
    return seqs, ([bytes(rng.integers(33, 127, n, dtype=np.uint8)) for n in lens] if fastq else None)


def digits_cases():
    """score, 2ndBestScore and hitLength at every count of digits; queryLength on both sides of 9 / 10, 99 / 100, 999 / 1000, unpaired
    and as the sum of two mates; numMatches 9, 10 and 63"""
    out = []
    nd = len(DIGITS)
    rng = np.random.default_rng(101)
    # one row, no row and two rows per query, every value in each of the three places
    rows = [[(q % 4, q % 6, DIGITS[q], DIGITS[(q + 7) % nd])] for q in range(nd)] + [[] for q in range(nd)] + \
           [[(1, 2, DIGITS[(q + 3) % nd], DIGITS[q]), (0, 3, DIGITS[q], DIGITS[(q + 11) % nd])] for q in range(nd)]
    score2 = [DIGITS[(q + 13) % nd] for q in range(nd)] + DIGITS + [DIGITS[(q + 5) % nd] for q in range(nd)]
    seqs, quals = _reads(rng, [20 + q % 9 for q in range(3 * nd)], True)
    b = assemble([b"d%d" % q for q in range(3 * nd)], seqs, quals, False, True, False, rows, score2, [NEVER] * (3 * nd))
    for q, r in enumerate(expected_rows(b, [SCORE, SCORE2, HIT_LEN])):
        if q < nd:
            assert r == b"%d\t%d\t%d\n" % (DIGITS[q], DIGITS[(q + 13) % nd], DIGITS[(q + 7) % nd])
    for name, cols in (("bodies", BODIES), ("default", DEFAULT), ("wide32", WIDE32), ("numbers", [SCORE, SCORE2, HIT_LEN])):
        out.append(("values-" + name, b, WORLD, cols, None, None))
    lens = [9, 10, 99, 100, 999, 1000]
    seqs, quals = _reads(rng, lens, True)
    b = assemble([b"L%d" % n for n in lens], seqs, quals, False, True, False, [[(0, 0, 5, 5)], [], [(1, 2, 6, 6)], [], [(2, 3, 7, 7)], []], [0] * 6, [NEVER] * 6)
    assert [r.split(b"\t")[1] for r in expected_rows(b, [READ_ID, QUERY_LEN, ZERO])] == [b"%d" % n for n in lens]
    for name, cols in (("bodies", BODIES), ("sam", SAM)):
        out.append(("querylen-unpaired-" + name, b, WORLD, cols, None, None))
    pairs = [(4, 5), (5, 5), (1, 8), (1, 9), (49, 50), (50, 50), (499, 500), (500, 500), (1, 998), (250, 750)]
    seqs, _ = _reads(rng, [n for p in pairs for n in p], False)
    b = assemble([b"P%d/%d" % (i // 2, i % 2 + 1) for i in range(2 * len(pairs))], seqs, None, True, False, False,
                 [[(0, 0, 5, 5)] if i % 2 else [] for i in range(len(pairs))], [0] * len(pairs), [NEVER] * len(pairs))
    assert [r.split(b"\t")[1] for r in expected_rows(b, [READ_ID, QUERY_LEN, ZERO])] == [b"%d" % (x + y) for x, y in pairs]
    for name, cols in (("bodies", BODIES), ("sam", SAM)):
        out.append(("querylen-mates-" + name, b, WORLD, cols, None, None))
    counts = [9, 10, 63, 1, 63, 10]
    seqs, quals = _reads(rng, [17] * len(counts), True)
    b = assemble([b"M%d" % n for n in counts], seqs, quals, False, True, False,
                 [[(i % 5, (i + q) % 6, 40 + i, 17) for i in range(n)] for q, n in enumerate(counts)], [3] * len(counts), [40, NEVER, 40, 41, NEVER, 49])
    assert [r.count(b"\n") for r in expected_rows(b, DEFAULT)] == counts
    for name, cols in (("bodies", BODIES), ("list-a", LIST_A)):
        out.append(("nummatches-" + name, b, WORLD, cols, None, None))
    return out


def lds_cases(lds_bytes):
    """a wavefront's stretch of exactly lds_bytes - phase bytes (the last that goes through the LDS stage) and one byte more, at each
    phase the stretch can start on: the very first wavefront (phase 0 only: it starts at byte 0), the first wavefront of the second
    block of 256 threads (256 queries in front), and a wavefront that is not a block's first (64 queries in front).  The readIDs are
    padded until expected_rows gives the sizes; every case carries (front, phase, stretch) for the test to assert them once more."""
    out = []
    for front in (0, 256, 64):
        for phase in range(4) if front else (0,):
            for over in (0, 1):
                for name, cols in (("bodies", BODIES), ("long", LONG)):
                    prog = DEFAULT if cols is BODIES else cols
                    nq = front + 64 + 1
                    rng = np.random.default_rng(1000 + front + 10 * phase + over)
                    seqs, quals = _reads(rng, [15 + (q * 7) % 19 for q in range(nq)], True)
                    rows = [[((q * 3) % 5, q % 6, 100 + q, 20 + q % 9)] if q % 5 else [] for q in range(nq)]
                    pad = [0] * nq

                    def build():
                        return assemble([b"q%d" % q + b"x" * pad[q] for q in range(nq)], seqs, quals, False, True, False, rows, [q % 3 for q in range(nq)],
                                        [100 + q if q % 2 else NEVER for q in range(nq)])
                    sizes = [len(r) for r in expected_rows(build(), prog)]
                    if front:
                        pad[0] = (phase - sum(sizes[:front])) % 4               # the stretch's first byte on the phase
                    more = lds_bytes - phase + over - sum(sizes[front:front + 64])
                    assert more >= 0
                    for q in range(front, front + 64):                          # one byte of readID is one byte of the query's one row
                        pad[q] = more // 64 + (q - front < more % 64)
                    b = build()
                    sizes = [len(r) for r in expected_rows(b, prog)]
                    assert sum(sizes[:front]) % 4 == phase and sum(sizes[front:front + 64]) == lds_bytes - phase + over
                    out.append(("front%d-phase%d-%s-%s" % (front, phase, "beyond" if over else "fits", name), b, WORLD, cols, None, None, (front, phase, lds_bytes - phase + over)))
    return out


def room_points(sizes):
    """the rooms a text of these per-query sizes is given: all of it, a byte less, a cut inside a row and on a row boundary, a cut
    inside the last wavefront's stretch (only that wavefront then finds its stretch's end beyond the room), none"""
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    nq, total = len(sizes), off[-1]
    last = (nq - 1) // 64 * 64
    assert last > 0 and nq - last >= 2 and off[last] < off[last + 1] + 2 < total
    return [("all", total), ("less1", total - 1), ("in-row", off[nq // 3] + 3), ("row-boundary", off[nq // 2]), ("last-wave", off[last + 1] + 2), ("none", 0)]


def room_cases():
    out = []
    for paired, fastq, seed in ((False, True, 21), (True, False, 22)):
        b = make_batch(130, -1, paired, fastq, seed=seed)
        for name, cols in (("bodies", BODIES), ("long", LONG), ("sam", SAM)):
            sizes = [len(r) for r in expected_rows(b, DEFAULT if cols is BODIES else cols)]
            for what, cap in room_points(sizes):
                out.append(("%s-%s-%s" % ("mates" if paired else "unpaired", name, what), b, WORLD, cols, cap, None))
    return out


def tuple_cases():
    """more tuple words than the room for them; a wavefront whose 64 queries all name one taxon, and one whose 64 all differ"""
    out = []
    rng = np.random.default_rng(303)
    nq = 130
    seqs, quals = _reads(rng, [16 + q % 5 for q in range(nq)], True)
    rows = [[((q + i) % 4, (q + 2 * i) % 6, 77, 16) for i in range((2, 5, 3)[q % 3])] for q in range(nq)]
    b = assemble([b"t%d" % q for q in range(nq)], seqs, quals, False, True, False, rows, [0] * nq, [77 if q % 10 else 78 for q in range(nq)])
    need = sum(len(t) + 1 for t in tally(b)[1])
    assert need == sum((3, 6, 4)[q % 3] for q in range(nq) if q % 10)
    for name, cols in (("bodies", BODIES), ("long", LONG)):
        for cap in (need, need - 1, 101, 2, 0):
            out.append(("cap%d-of-%d-%s" % (cap, need, name), b, WORLD, cols, None, cap))
    nq = 192
    seqs, quals = _reads(rng, [16] * nq, True)
    # wavefront 0: one taxon; wavefront 1: 64 taxa; wavefront 2: no rows at all (tax ID 0's dense taxon, 64 times)
    rows = [[(q % 70, 5, 50, 16)] if q < 64 else [(q % 70, 3 + q - 64, 50, 16)] if q < 128 else [] for q in range(nq)]
    b = assemble([b"s%d" % q for q in range(nq)], seqs, quals, False, True, False, rows, [0] * nq, [50] * nq)
    single = tally(b, WORLD_WIDE)[0]
    assert single[5] == 65 and single[0] == 64 and all(single[3 + i] == 1 for i in range(64) if i != 2) and single.sum() == 192
    for name, cols in (("bodies", BODIES), ("long", LONG)):
        out.append(("ballot-ends-" + name, b, WORLD_WIDE, cols, None, None))
    return out


def name_cases():
    """an empty readID (the name starts with white space), one of 255 bytes and longer ones, /1 /2 /3 behind a comment"""
    names = [b" starts with a blank", b"\tx", b"n" * 255, b"m" * 256, b"k" * 300 + b" c", b"a comment/1", b"b c/2", b"c\tc/3", b"d/1 c", b"e/3", b"f/4", b"g c/4",
             b"h" * 254 + b"/1", b"i" * 255 + b"/2"]
    ids = [b"", b"", b"n" * 255, b"m" * 256, b"k" * 300, b"a", b"b", b"c", b"d/1", b"e", b"f/4", b"g", b"h" * 254, b"i" * 255]
    assert [read_id(n) for n in names] == ids
    rng = np.random.default_rng(404)
    out = []
    for fastq in (True, False):
        seqs, quals = _reads(rng, [15 + q for q in range(len(names))], fastq)
        b = assemble(names, seqs, quals, False, fastq, False, [[(q % 4, q % 6, 9, 9)] * (q % 3) for q in range(len(names))], [0] * len(names), [NEVER] * len(names))
        assert b["idLen"] == [len(i) for i in ids]
        for name, cols in (("bodies", BODIES), ("long", LONG), ("id", [READ_ID])):
            out.append(("%s-%s" % ("fastq" if fastq else "fasta", name), b, WORLD, cols, None, None))
    return out


def table_cases():
    """an empty uid, an empty rank string, a tax ID at full width in both fields; rows whose uniqueID is nRefs and far beyond it
    (they print the taxon's rank); rows whose taxon index is nTaxa or larger: the kernels print dense taxon 0 for them, never count
    them as perfect — the reference has no such row, this pins what the kernels do"""
    W = WORLD_EDGE
    rows = [[(1, 0, 5, 5)], [(1, 2, 5, 5), (4, 2, 5, 5)], [(W["nRefs"], 0, 5, 5)], [(0xffffffff, 3, 5, 5), (W["nRefs"] - 1, 3, 5, 5)],
            [(0, W["nTaxa"], 5, 5)], [(2, 0xffffffff, 5, 5), (2, W["nTaxa"] + 1, 5, 5)], [(2, 5, 5, 5), (0, W["nTaxa"], 5, 5)], [(1, 2, 5, 5)], []]
    rng = np.random.default_rng(505)
    seqs, quals = _reads(rng, [18] * len(rows), True)
    b = assemble([b"w%d" % q for q in range(len(rows))], seqs, quals, False, True, False, rows, [0] * len(rows), [5] * len(rows))
    want = expected_rows(b, [SEQ_ID, TAX_ID], W)
    assert want[0] == b"\t9646\n" and want[1] == b"\t4294967295.4294967295\n" + b"u" * 70 + b"\t4294967295.4294967295\n"
    assert want[2] == b"species\t9646\n" and want[3] == b"leaf\t12.7\n" + b"u" * 70 + b"\t12.7\n" and want[4] == b"gi|4\t9646\n" and want[7] == b"\t4294967295.4294967295\n"
    single, tuples = tally(b, W)
    assert tuples == [(2, 2), (3, 3)] and single[0] == 2 and single[2] == 1 and single[1] == 1 and single.sum() == 4
    return [("edge-" + name, b, W, cols, None, None) for name, cols in (("bodies", BODIES), ("default", DEFAULT), ("list-a", LIST_A), ("list-b", LIST_B), ("wide32", WIDE32))]


GROUPS = {"digits": digits_cases, "rooms": room_cases, "tuples": tuple_cases, "names": name_cases, "tables": table_cases}


def group_ids(group, *args):
    return [c[0] for c in cases(group, *args)]


_cache = {}


def cases(group, *args):
    """the cases of a group, built once (the batches are shared: no test changes one)"""
    key = (group,) + args
    if key not in _cache:
        _cache[key] = (lds_cases if group == "lds" else GROUPS[group])(*args)
    return _cache[key]
