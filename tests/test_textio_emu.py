"""The front end's ingest and egress on the device (centrifuge_amd/csrc/cf_textio.hpp) in the CPU harness: the bodies of
cf_batch_upload_text's kernels, of the plan stage's k_text_pack and of cf_batch_wait_text's formatter, one call per thread — in
the one-lane build and as wavefronts of 64 lanes (their cross-lane sums) — against

* the HOST parser (`centrifuge-class --dump-reads`, itself checked against the reference's parsers: tests/test_ingest.py,
  tests/fuzz/fuzz_ingest.py): a block the device takes for plain must give the very reads, names and seeds the host parser
  gives, and everything the host parser treats specially must be flagged as not plain;
* a plain Python statement of the default columns (aln_sink.h:2279-2337, readID aln_sink.h:2203-2217) and of the tally
  (aln_sink.h:142-172) for the formatter."""
import ctypes as C

import numpy as np
import pytest

import textcases as T
from emu import emu
from emu import emu_textio as E
from textcases import FASTA, FASTQ, host_parse, make_records, read_id

padded, vp = E.padded, E.vp
PLAIN = T.plain_cases()
IRREGULAR = T.irregular_cases()
CAPACITY = T.capacity_cases()


@pytest.fixture(params=[False, True], ids=["lane1", "wave64"])
def L(request):
    was = emu.use_wave64(request.param)
    lib = E.lib(request.param)
    lib.emu_text_format.restype = C.c_uint64
    # arrays as cf_batch_upload_text sizes them (recCap = total / 32 + 1024) in the one-lane build; the 64-lane build, which runs
    # every thread of a launch as a fiber, gets arrays for the block's own records, as before
    lib.upload_caps = not request.param
    yield lib
    emu.use_wave64(was)


def parse(L, text, fmt, seed=0, rec_cap=None, pos_cap=None):
    return E.parse(L, text, fmt, seed, rec_cap, pos_cap)


def check_plain(L, c, seed, upload_caps):
    """the block (or the two blocks of mates) is taken and gives the host parser's reads; upload_caps: arrays as cf_batch_upload_text sizes them"""
    if c.text2 is not None:
        flags, got = E.parse_mates(L, c.text, c.text2, c.fmt, seed)
        w1, w2 = host_parse(c.text, c.fmt, seed), host_parse(c.text2, c.fmt, seed)
        assert w1 is not None and w2 is not None and len(w1) == len(w2)
        want = [w[q] for q in range(len(w1)) for w in (w1, w2)]
    else:
        caps = (T.rec_cap(len(c.text)), T.pos_cap(len(c.text), c.fmt)) if upload_caps else (None, None)
        flags, got = parse(L, c.text, c.fmt, seed, *caps)
        want = host_parse(c.text, c.fmt, seed)
    assert flags == 0, (c.name, flags)
    assert want is not None and got == want, c.name


@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_plain_blocks_parse_as_the_host_parser_does(L, fmt):
    for c in PLAIN:
        if c.fmt == fmt and c.group == "trials":
            for seed in T.SEEDS:
                check_plain(L, c, seed, False)
    assert parse(L, b"", fmt) == (0, [])


@pytest.mark.parametrize("group", sorted(set(c.group for c in PLAIN) - {"trials"}))
def test_the_table_of_plain_blocks_parses_as_the_host_parser_does(L, group):
    """the table's plain cases (tests/textcases.py), arrays sized as the upload sizes them: reads, bases, longest read, every readID,
    every base, every seed"""
    for c in PLAIN:
        if c.group == group:
            for seed in T.SEEDS:
                check_plain(L, c, seed, L.upload_caps)


@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_two_blocks_of_mates_in_one_buffer(L, fmt):
    """cf_batch_upload_text with text2: the blocks lie one behind the other, record r of block m is read 2 r + m of the batch, the
    places the later passes use count from the buffer's start"""
    rng = np.random.default_rng(31 + fmt)
    n = 97
    t1, t2 = make_records(rng, n, fmt, lower=True), make_records(rng, n, fmt, wrap=9 if fmt == FASTA else 0)
    flags, got = E.parse_mates(L, t1, t2, fmt, 7)
    assert flags == 0 and len(got) == 2 * n
    want = [host_parse(t1, fmt, 7), host_parse(t2, fmt, 7)]
    for r in range(2 * n):
        assert got[r] == want[r % 2][r // 2], r


@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_everything_the_host_parser_treats_specially_is_flagged(L, fmt):
    """every irregular block of the table — alone, behind 70 records, and as record 0, 63, 64, 255, 256 and 300 of 300 — carries its bit"""
    seen = 0
    for c in IRREGULAR:
        if c.fmt == fmt:
            caps = (T.rec_cap(len(c.text)), T.pos_cap(len(c.text), fmt)) if L.upload_caps else (None, None)
            flags, _ = parse(L, c.text, fmt, 0, *caps)
            assert T.carries(flags, c.bit), (c.name, flags, c.bit)
            seen |= flags
    # every reason bit of the format is reached
    assert seen & 0x7ff == (0x3f if fmt == FASTA else 0x3ff), hex(seen)
    # too many records / markers for the arrays: left to the host as well
    text = make_records(np.random.default_rng(6), 50, fmt)
    assert parse(L, text, fmt, rec_cap=49)[0] & 1024
    assert parse(L, text, fmt, rec_cap=50)[0] == 0


def test_the_capacity_table_is_the_formula():
    """CAPACITY's counts against recCap = total / 32 + 1024 (tests/textcases.py's docstring); the library is not called"""
    for fmt in (FASTA, FASTQ):
        for unit, n, fits in T.CAPACITY[fmt]:
            total = len(unit) * n
            records = unit.count(b">") * n if fmt == FASTA else unit.count(b"\n") * n // 4
            markers = (unit.count(b">") if fmt == FASTA else unit.count(b"\n")) * n
            cap = total // 32 + 1024
            assert (records <= cap and markers <= (cap if fmt == FASTA else 4 * cap)) == fits, (unit, n)
        # the edge itself: each unit's largest fitting count is followed by its smallest refused one
        for unit in set(u for u, _, _ in T.CAPACITY[fmt]):
            ok = max(n for u, n, f in T.CAPACITY[fmt] if u == unit and f)
            assert (unit, ok + 1, False) in T.CAPACITY[fmt]
        assert T.FLOOD > 4 * (T.FLOOD // 32 + 1024)


@pytest.mark.parametrize("c", CAPACITY, ids=[c.name for c in CAPACITY])
def test_a_block_beyond_the_upload_capacity_is_too_many_and_nothing_else(L, c):
    """arrays sized by the upload's formula, a filled margin behind each (E.parse checks the margins): text_mark_body's guard and
    text_counts leave a block with more markers than posCap alone"""
    total = len(c.text)
    assert parse(L, c.text, c.fmt, 0, T.rec_cap(total), T.pos_cap(total, c.fmt))[0] == T.TOO_MANY


@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_mutated_blocks_are_either_flagged_or_parsed_as_the_host_parser_does(L, fmt):
    """the safety property of the plain form: whatever a block looks like, if the device takes it, its reads are the host parser's"""
    taken = 0
    for trial, text in enumerate(T.mutated(fmt)):
        flags, got = parse(L, text, fmt)
        if flags:
            continue
        taken += 1
        want = host_parse(text, fmt)
        assert want is not None and got == want, (trial, text)
    assert taken >= 10                                         # (some mutations leave a plain block: the comparison did run)


# ---------------------------------------------------------------------------------------------- the formatter
def format_reference(names, qlens, rows_of, score2, uid, rank_name, tax_col, leaf):
    out = []
    for q, name in enumerate(names):
        rid = read_id(name)
        rows = rows_of[q]
        if not rows:
            out.append(rid + b"\tunclassified\t0\t0\t%d\t0\t%d\t1\n" % (score2[q], qlens[q]))
        for (u, t, score, hit) in rows:
            sid = uid[u] if leaf[t] and u < len(uid) else rank_name[t]
            out.append(rid + b"\t" + sid + b"\t" + tax_col[t] + b"\t%d\t%d\t%d\t%d\t%d\n" % (score, score2[q], hit, qlens[q], len(rows)))
    return b"".join(out)


@pytest.mark.parametrize("paired", [0, 1])
def test_default_columns_and_the_tally_from_narrow_rows(L, paired):
    rng = np.random.default_rng(77 + paired)
    n_taxa, n_refs, nq = 37, 19, 333
    uid = [("NC_%06d.%d" % (rng.integers(0, 999999), rng.integers(1, 9))).encode() for _ in range(n_refs)]
    rank_name = [rng.choice([b"species", b"genus", b"no rank", b"superkingdom"]) for _ in range(n_taxa)]
    tax_col = [(b"%d" % rng.integers(0, 2 ** 32)) + ((b".%d" % rng.integers(1, 2 ** 32)) if rng.random() < 0.2 else b"") for _ in range(n_taxa)]
    leaf = [int(rng.random() < 0.6) for _ in range(n_taxa)]
    strs, uid_off, rank_off, tax_off = bytearray(), [], [], []
    for table, offs in ((uid, uid_off), (rank_name, rank_off), (tax_col, tax_off)):
        for x in table:
            offs.append(len(strs))
            strs += x
        offs.append(len(strs))
    per = 2 if paired else 1
    text = make_records(rng, nq * per, FASTA)
    flags_, parsed = 0, None
    buf = padded(text)
    rec_cap = nq * per + 16
    arr = [np.zeros(rec_cap + 80, dtype=np.uint32) for _ in range(5)]
    status = np.zeros(4, dtype=np.uint64)
    assert L.emu_text_parse(vp(buf), len(text), FASTA, 0, rec_cap, rec_cap, *[vp(a) for a in arr], vp(status)) == nq * per and not status[3]
    rlen, _seeds, _seq_off, id_off, id_len = arr
    names = [text[int(id_off[r * per]) - 0:].split(b"\n", 1)[0] for r in range(nq)]
    qlens = [int(rlen[q * per]) + (int(rlen[q * per + 1]) if paired else 0) for q in range(nq)]
    rows_of, score2, max_score = [], [], []
    for q in range(nq):
        n = int(rng.choice([0, 1, 1, 1, 2, 3, 5]))
        ms = int(rng.choice([50, 7225, 0xffffffff]))
        rows = [(int(rng.integers(0, n_refs + 3)) if rng.random() < 0.8 else 0xffffffff, int(rng.integers(0, n_taxa)),
                 int(rng.choice([ms if ms != 0xffffffff else 9, 7225, 49, 0, 4000000000])), int(rng.integers(0, 100000))) for _ in range(n)]
        rows_of.append(rows); score2.append(int(rng.choice([0, 49, 12345678]))); max_score.append(ms)
    rows = np.array([r for rs in rows_of for r in rs] + [(0, 0, 0, 0)], dtype=np.uint32).reshape(-1, 4)
    qinfo = np.array([len(rs) | 0x40 for rs in rows_of], dtype=np.uint8)
    s2, ms_a = np.array(score2, dtype=np.uint32), np.array(max_score, dtype=np.uint32)
    want = format_reference(names, qlens, rows_of, score2, uid, rank_name, tax_col, leaf)
    out = np.zeros(len(want) + 64, dtype=np.uint8)
    idx_zero = 3
    single = np.zeros(n_taxa, dtype=np.uint64)
    tuples = np.zeros(6 * nq + 16, dtype=np.uint32)
    tw = C.c_uint32(0)
    sb = np.frombuffer(bytes(strs) + bytes(16), dtype=np.uint8)
    mk = lambda x: np.array(x, dtype=np.uint32)
    uo, ro, to, lf = mk(uid_off), mk(rank_off), mk(tax_off), np.array(leaf, dtype=np.uint8)
    L.emu_text_format.argtypes = None
    got_n = L.emu_text_format(vp(buf), vp(id_off), vp(id_len), vp(rlen), vp(rows), vp(qinfo), vp(s2), vp(ms_a), C.c_uint32(nq), C.c_int(paired),
                              vp(sb), vp(uo), vp(ro), vp(to), vp(lf), C.c_uint32(n_refs), C.c_uint32(n_taxa), C.c_uint32(idx_zero),
                              vp(out), C.c_uint64(len(want)), vp(single), vp(tuples), C.c_uint32(len(tuples)), C.byref(tw))
    assert got_n == len(want)
    assert bytes(out[:got_n]) == want
    # the tally (aln_sink.h:142-172): perfect single assignments per taxon (unclassified under taxon 0), perfect tuples
    want_single = np.zeros(n_taxa, dtype=np.uint64)
    want_tuples = []
    for q in range(nq):
        rs, ms = rows_of[q], max_score[q]
        if not rs:
            want_single[idx_zero] += 1
        elif len(rs) == 1:
            if ms != 0xffffffff and rs[0][2] >= ms:
                want_single[rs[0][1]] += 1
        elif ms != 0xffffffff and all(r[2] >= ms for r in rs):
            want_tuples.append(tuple(r[1] for r in rs))
    assert (single == want_single).all()
    got_tuples, i = [], 0
    while i < tw.value:
        n = int(tuples[i])
        got_tuples.append(tuple(int(x) for x in tuples[i + 1:i + 1 + n]))
        i += 1 + n
    assert sorted(got_tuples) == sorted(want_tuples) and want_tuples
