"""Any list of columns on the device text path (fmt_cols_size_body / fmt_cols_write_body, centrifuge_amd/csrc/cf_textio.hpp) in the CPU
harness of tests/emu/emu_cols.cpp — the one-lane build and wavefronts of 64 lanes — against a plain Python statement of the host's
general formatter (formatRange, cf_cli.cpp; the reference: aln_sink.h:2279-2337, readID aln_sink.h:2203-2217), byte for byte:
synthetic blocks of FASTA (wrapped at 60 columns, lower case) and FASTQ text, unpaired and mates, with the sizes at which the
cooperative copy of the long fields changes its way (word and dword boundaries of the 2-bit expansion, the four byte phases of
a field's first byte, a wavefront's tail and a second wavefront, stretches inside and beyond the LDS stage)."""
import numpy as np
import pytest

from centrifuge_amd import capi
from emu import emu_cols

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
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 250]
NEVER = 0xffffffff


def make_world():
    """a classifier's string tables: four references, six dense taxa (tax ID 0 among them: the reads without rows are counted there)"""
    uids = [b"gi|4", b"NC_000913.3", b"r2", b"chr"]
    taxa = [9646, 0, 562, (7 << 32) | 12, 40674, 2]
    seqid_rank = [b"species", b"no rank", b"species", b"leaf", b"class", b"superkingdom"]
    leaf = [1, 0, 1, 1, 0, 0]
    ranks = [b"species", b"no rank", b"species", b"subspecies", b"class", b"superkingdom"]
    names = [b"Ailuropoda melanoleuca", b"", b"Escherichia coli", b"a strain of it", b"Mammalia", b"Bacteria"]

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
             taxLeaf=leaf, nRefs=len(uids), nTaxa=len(taxa), idxZero=1, taxStrs=t1 + t2, trankOff=trank_off, tnameOff=[o + len(t1) for o in tname_off])
    w.update(uids=uids, taxTxt=tax_txt, seqidRank=seqid_rank, ranks=ranks + [b"no rank"], names=names + [b"root-less"])
    return w


WORLD = make_world()


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
    # rows: rows_per_query of them (0: unclassified), or a mix
    rows, qinfo, score2, max_score = [], [], [], []
    for q in range(nq):
        n = rows_per_query if rows_per_query >= 0 else (0, 1, 5, 2)[q % 4]
        ms = int(rng.integers(1, 40000)) if q % 9 else NEVER
        perfect = q % 2 == 0
        for i in range(n):
            t = int(rng.integers(0, WORLD["nTaxa"]))
            rows.append((int(rng.integers(0, WORLD["nRefs"] + 2)), t, ms if perfect and ms != NEVER else int(rng.integers(0, max(1, min(ms, 99999)))), int(rng.integers(0, 500))))
        qinfo.append(n | 0x40)
        score2.append(int(rng.integers(0, 3)) * int(rng.integers(0, 100000)))
        max_score.append(ms)
    bases, nmask = pack(seqs)
    b = dict(text=text, idOff=id_off, idLen=id_len, rlen=rlen, qualOff=qual_off if fastq else None, bases=bases, nmask=nmask,
             rows=np.array(rows, dtype=np.uint32).reshape(-1, 4), qinfo=qinfo, score2=score2, maxScore=max_score, paired=paired)
    b.update(names=names, seqs=seqs, quals=quals)
    return b


def expected(b, cols):
    """formatRange (cf_cli.cpp) in plain Python"""
    W, out, per, first = WORLD, [], 2 if b["paired"] else 1, 0
    for q in range(len(b["qinfo"])):
        n = b["qinfo"][q] & 0x3f
        ra, rb = q * per, q * per + 1
        seq = lambda r: b["seqs"][r]
        qual = lambda r: b["quals"][r] if b["quals"] is not None else b"I" * len(b["seqs"][r])
        qlen = len(seq(ra)) + (len(seq(rb)) if b["paired"] else 0)
        for i in range(max(1, n)):
            uncl = n == 0
            uid, t, score, hit = (0, W["nTaxa"], 0, 0) if uncl else [int(v) for v in b["rows"][first + i]]
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
            out.append(b"\t".join(fields) + b"\n")
        first += n
    return b"".join(out)


def first_diff(a, b):
    for i in range(min(len(a), len(b))):
        if a[i] != b[i]:
            return "byte %d: got %r, want %r" % (i, a[max(0, i - 30):i + 30], b[max(0, i - 30):i + 30])
    return "lengths %d / %d; got ends %r, want ends %r" % (len(a), len(b), a[-40:], b[-40:])


@pytest.fixture(params=[False, True], ids=["lane1", "wave64"])
def wave64(request):
    return request.param


def check(b, cols, wave64, tally=None):
    want = expected(b, cols)
    got, single, tuples = emu_cols.format_rows(WORLD, b, cols, wave64=wave64, out_cap=len(want))
    assert got == want, first_diff(got, want)
    if tally is not None:
        # the tally does not depend on the columns: what the default bodies leave on the same rows (the tuples in any order)
        assert np.array_equal(single, tally[0])
        assert sorted(split_tuples(tuples)) == sorted(split_tuples(tally[1]))
    return want


def split_tuples(t):
    out, i = [], 0
    while i < len(t):
        out.append(tuple(int(v) for v in t[i + 1:i + 1 + t[i]]))
        i += 1 + int(t[i])
    assert i == len(t)
    return out


def default_tally(b, wave64):
    text, single, tuples = emu_cols.format_rows(WORLD, b, DEFAULT, wave64=wave64, default_bodies=True, out_cap=len(expected(b, DEFAULT)))
    return text, single, tuples


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_every_program_prints_what_the_host_formatter_prints(wave64, paired, fastq):
    # 130 queries with 0 / 1 / 5 / 2 rows in turn: two wavefronts and the tail of a third; a FASTA block wrapped at 60 columns, every
    # other record lower case
    b = make_batch(130, -1, paired, fastq, seed=5 + paired, wrap_lower=not fastq)
    text0, single, tuples = default_tally(b, wave64)
    assert len(split_tuples(tuples)) > 3 and single.sum() > 10
    for cols in PROGRAMS:
        want = check(b, cols, wave64, tally=(single, tuples))
        if cols == DEFAULT:
            assert want == text0                                       # the default eight through the new bodies: the old bodies' bytes


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("rows", [0, 1, 5])
def test_wavefront_tails_and_row_counts(wave64, nq, rows):
    for paired, fastq in ((False, True), (True, False)):
        b = make_batch(nq, rows, paired, fastq, seed=nq + rows)
        tally = default_tally(b, wave64)[1:]
        for cols in (LIST_A, LIST_B, SAM):
            check(b, cols, wave64, tally=tally)


def test_byte_phases_and_the_lds_stage(wave64):
    """the first byte of a wavefront's stretch, and with it of every long field, on each of the four places in a dword; stretches that
    fit the LDS stage (short reads, one row each) and stretches beyond it (five rows of up to 250 bases)"""
    lds = emu_cols.lib(wave64).emu_cols_lds_bytes()
    fits = beyond = 0
    for extra in range(4):
        for rows, lengths in ((1, [1, 15, 16, 17, 31, 32, 33]), (5, LENGTHS)):
            for cols in ([SEQ], [QUAL], LIST_A, SAM):
                b = make_batch(65, rows, False, True, seed=3, id_extra=extra, lengths=lengths)
                want = check(b, [READ_ID] + cols, wave64)
                # the bytes of the first wavefront's 64 queries
                stretch = len(expected(dict(b, qinfo=b["qinfo"][:64]), [READ_ID] + cols))
                fits += stretch + 3 <= lds
                beyond += stretch > lds
                assert len(want) > stretch
    assert fits >= 8 and beyond >= 8


def test_rows_that_do_not_fit_the_buffer_are_left_out(wave64):
    """the bounds of the write pass: with room for fewer bytes than the rows take, the rows that fit are printed and nothing is
    written past the room (the harness keeps marked bytes behind it)"""
    b = make_batch(65, 1, False, True, seed=9)
    want = expected(b, SAM)
    cut = len(want) // 2
    sizes = [len(expected(dict(b, qinfo=b["qinfo"][:q + 1]), SAM)) for q in range(65)]
    whole = max(s for s in sizes if s <= cut)
    part, _, _ = emu_cols.format_rows(WORLD, b, SAM, wave64=wave64, out_cap=cut)
    assert len(part) == cut and part[:whole] == want[:whole]


def test_column_names_are_the_reference_s():
    """cf_text_column_of: the one table of names (no device needed); the codes are those of this file"""
    assert (capi.COL_READ_ID, capi.COL_QUAL2, capi.COL_PLACEHOLDER, capi.COL_ZERO, capi.TEXT_MAX_COLS) == (READ_ID, QUAL2, PLACEHOLDER, ZERO, 32)
    for n, c in NAMES.items():
        assert capi.text_column_of(n) == c, n
    assert capi.text_column_of("readID") == capi.COL_READ_ID and capi.text_column_of("QNAME") == capi.COL_READ_ID
    assert capi.text_column_of("taxLevel") == capi.COL_TAX_RANK and capi.text_column_of("taxRank") == capi.COL_TAX_RANK
    assert capi.text_column_of("CIGAR") == capi.COL_PLACEHOLDER and capi.text_column_of("MAPQ") == capi.COL_ZERO
    assert capi.text_column_of("QUAL2") == capi.COL_QUAL2 and capi.text_column_of("SEQ") == capi.COL_SEQ
    assert capi.text_column_of("readid") == -1 and capi.text_column_of("") == -1
