"""The reads of tests/classifycases.py without a device: every case's claim holds for what the oracle finds, the record of the
reference's output (tests/golden/classify_edges.json) is what the generator and the compiled reference give today, the oracle and
capi.Report reproduce every recorded TSV and report digest, and the kernels' CPU build (tests/emu) gives the oracle's rows, n_rows,
2ndBest and counters under every table combination, both search versions and - groups A, B, E - as a wavefront of 64 lanes.
This leg tells a wrong kernel body from a device-only fault of tests/test_gpu_classify_edges.py.

The indexes come from the unmodified reference builder (oracle/_ref), so everything that needs one is skipped without it.

Table combinations of the emu leg: the hooks build what they are asked for at any size, the device layer does not - planTablesIn
makes text tables only for n >= 64 -, so the combinations with text tables are run where the device could run them (n >= 64);
the wide ftab of ftabChars + 1 is left out at -t 12 (4^13 entries: half a gigabyte on the CPU)."""
import ctypes as C
import hashlib
import os
import shutil
import tempfile

import numpy as np
import pytest

import buildcases as B
import classifycases as K
from centrifuge_amd import capi, reads
from oracle import oracle as O

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the compiled reference) is not built")

_tmp = None
_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _workdir():
    global _tmp
    _tmp = tempfile.mkdtemp(prefix="cf_classify_cases_")
    yield
    for c in _ctx.values():
        c["orc"].close(); c["hix"].close()
    _ctx.clear()
    shutil.rmtree(_tmp, ignore_errors=True)


def ctx(name):
    """the case's index (reference builder), its reads as arrays and the oracle's answer per run: made once, left unchanged"""
    if name not in _ctx:
        c = K.BY_NAME[name]
        d = os.path.join(_tmp, name)
        assert B.run_reference(c.build, d)["exit"] == 0
        base = os.path.join(d, "idx")
        orc, hix = O.Oracle(base), capi.Index(base, host_only=True)
        x = dict(case=c, base=base, orc=orc, hix=hix, runs={})
        for rid, _args, paired in c.runs():
            names, qlens, seq, off, seeds, pr = K.load_arrays(c.reads, c.mate2 if paired else None)
            want = orc.classify(seq, off, seeds, len(names), pr, orc.params(**K.RUN_KW[rid]))
            x["runs"][rid] = dict(names=names, qlens=qlens, seq=seq, off=off, seeds=seeds, paired=pr, want=want, kw=K.RUN_KW[rid])
        _ctx[name] = x
    return _ctx[name]


def sha(text):
    return hashlib.sha256(text.encode("latin1") if isinstance(text, str) else text).hexdigest()


def oracle_tally(hix, want, n_taxa):
    """the per-taxon counters of the oracle's rows (as test_gpu_variants.tally, taxa by their id)"""
    rows, n_rows, _ = want
    idx = {int(t): i for i, t in enumerate(hix.taxon_ids())}
    a, u = np.zeros(n_taxa, dtype=np.uint64), np.zeros(n_taxa, dtype=np.uint64)
    for q in range(len(n_rows)):
        if n_rows[q] == 0:
            a[0] += 1; u[0] += 1
        for r in range(int(n_rows[q])):
            a[idx[int(rows[q, r]["tax_id"])]] += 1
        if n_rows[q] == 1:
            u[idx[int(rows[q, 0]["tax_id"])]] += 1
    return a, u


def assert_rows(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "n_rows", np.nonzero(got[1] != want[1])[0][:10])
    assert np.array_equal(got[2], want[2]), (what, "score2", np.nonzero(got[2] != want[2])[0][:10])
    live = np.arange(want[0].shape[1])[None, :] < want[1][:, None]
    for f in ("tax_id", "unique_id", "score", "hit_len"):
        assert np.array_equal(got[0][f][live], want[0][f][live]), (what, f)


# ------------------------------------------------------------------ the recipes and the record
def test_every_group_is_there_and_the_recipes_stay_small():
    assert {c.group for c in K.CASES} == set(K.GROUPS) and len(K.CASES) == len([c for c in B.CASES if c.group in K.GROUPS])
    for c in K.CASES:
        if c.group == "F" and not O.have_ref():
            continue                                        # (1.5 s each to generate: with the rest of their tests)
        assert 20 <= len(c.reads) <= K.MAX_READS and max(len(r) for _, r in c.reads) <= K.MAX_LEN, c.name
        assert len({nm for nm, _ in c.reads}) == len(c.reads)


def test_record_covers_every_case_and_keeps_the_cap():
    """one record per case; refused cases are a cap: at least half of every group and 85 % overall stay"""
    g = K.load_golden()
    assert sorted(g) == sorted(K.NAMES)
    kept = K.kept_names()
    for grp, names in K.by_group(K.NAMES).items():
        assert 2 * len([n for n in names if n in kept]) >= len(names), grp
    assert len(kept) >= 0.85 * len(K.NAMES)
    for n in kept:
        assert sorted(g[n]["runs"]) == sorted(rid for rid, _, _ in K.BY_NAME[n].runs()), n
        assert g[n]["build_args"] == K.BY_NAME[n].build.ref_args


@pytest.mark.parametrize("name", K.NAMES)
def test_reads_are_the_recorded_ones(name):
    assert K.BY_NAME[name].fasta_sha256() == K.load_golden()[name]["reads_sha256"], "the generator has changed, regenerate the record"


@needs_ref
@pytest.mark.parametrize("name", K.NAMES)
def test_reference_reproduces_the_record(name, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_classify_golden as M
    assert M.run_case(K.BY_NAME[name], str(tmp_path)) == K.load_golden()[name]


# ------------------------------------------------------------------ claims
@needs_ref
@pytest.mark.parametrize("name", K.kept_names())
def test_claim_holds(name):
    x = ctx(name)
    c, orc, run = x["case"], x["orc"], x["runs"]["k5"]
    p = orc.params(k=5)
    hits = []
    for _nm, r in c.reads:
        hf, hr = np.zeros(len(r) + 2, dtype=capi.HIT_DTYPE), np.zeros(len(r) + 2, dtype=capi.HIT_DTYPE)
        n = (C.c_uint32 * 2)()
        codes = np.ascontiguousarray(r if len(r) else np.zeros(1, dtype=np.uint8))
        assert orc.L.cfo_search(orc.h, C.byref(p), codes.ctypes.data, len(r), hf.ctypes.data, hr.ctypes.data, n) == 0
        hits.append((hf[:n[0]], hr[:n[1]]))
    t = c.build.codes
    sa = B.suffix_array(t) if len(t) <= 20000 else None
    v = K.View(c, c.reads, hits, run["want"][1], c.build.starts(), len(t))
    assert c.claim(v, sa), "%s: the recipe has drifted: %s" % (name, c.claim_text)


# ------------------------------------------------------------------ the oracle and the report module against the record
@needs_ref
@pytest.mark.parametrize("name", K.kept_names())
def test_oracle_and_report_reproduce_the_record(name):
    from test_report import max_scores
    x = ctx(name)
    rec = K.load_golden()[name]["runs"]
    for rid, run in x["runs"].items():
        rows, n_rows, s2 = run["want"]
        got = reads.format_tsv(x["hix"].seqid, run["names"], run["qlens"], rows, n_rows, s2)
        assert got.count("\n") == rec[rid]["tsv"]["rows"], (name, rid)
        assert sha(got) == rec[rid]["tsv"]["sha256"], (name, rid)
        k = run["kw"]["k"]
        full = np.zeros(rows.shape, dtype=capi.ROW_DTYPE)
        idx = {int(t): i for i, t in enumerate(x["hix"].taxon_ids())}
        for f in ("tax_id", "unique_id", "score", "hit_len"):
            full[f] = rows[f]
        live = np.arange(k)[None, :] < n_rows[:, None]
        full["taxon_idx"][live] = [idx[int(t)] for t in rows["tax_id"][live]]
        rep = capi.Report(x["hix"])
        rep.add(full, n_rows, max_scores(x["orc"], run["seq"], run["off"], run["paired"]), k)
        path = os.path.join(_tmp, "%s_%s.rep" % (name, rid))
        rep.write(path); rep.close()
        raw = open(path, "rb").read()
        assert raw.count(b"\n") == rec[rid]["report"]["rows"] and sha(raw) == rec[rid]["report"]["sha256"], (name, rid)


# ------------------------------------------------------------------ the kernels' CPU build
# (name, planes, pair planes, wide ftab: 0 / "+1" / "+6", text rate, resolve rate, position form, small-range rows, without sides)
COMBOS = [
    ("sides",       0, 0, 0,    -1, -1, 0, 0, 0),
    ("planes",      1, 0, 0,    -1, -1, 0, 0, 0),
    ("auto",        1, 1, "+1", 0,  0,  1, 0, 0),
    ("small4",      1, 0, 0,    0,  -1, 0, 4, 0),
    ("rate3",       1, 1, "+6", 3,  3,  1, 0, 0),
    ("no_sides",    1, 1, "+1", -1, 1,  0, 0, 1),
]


def set_tables(L, e, c, combo):
    """-> None when the combination cannot be made for the case, else the tables that stand"""
    _nm, pl, pp, wide, text, dense, pos, multi, nosides = combo
    n, ftc, off_rate = c.build.n, c.build.ftab_chars, c.build.off_rate
    if text >= 0 and n < 64:
        return None
    k = 0 if not wide else ftc + 1 if wide == "+1" else min(ftc + 6, 12)
    if k and (k <= ftc or k > 12):
        return None
    assert L.emu_planify(e.h, pl) == 1
    assert L.emu_planify2(e.h, pp) == (1 if pl or not pp else 0)
    assert L.emu_widen(e.h, k) == (1 if k else 0)
    made = dict(text=L.emu_textify(e.h, text), dense=L.emu_densify(e.h, dense))
    assert made["text"] == (1 if text >= 0 else 0) and made["dense"] == (1 if 0 <= dense < off_rate else 0)
    made["pos"] = L.emu_posify(e.h, pos)
    L.emu_set_multi_verify(multi, 0 if multi else 2)
    assert L.emu_drop_sides(e.h, nosides) == 1
    return made


EMU_LIMIT_S = 300       # the slowest case takes 12 s


def run_emu(name, combos, versions, wave64=False):
    """A kernel body that is wrong in its counts (a '$' row counted as a base, say) can make the BWT no permutation, and a
    walk-left over it goes round in circles inside the C++ call: the watchdog then ends the run with the traceback of this case
    rather than leaving the suite hanging without a word"""
    import faulthandler
    import sys
    from emu import emu
    was = emu.use_wave64(wave64)
    faulthandler.dump_traceback_later(EMU_LIMIT_S, exit=True, file=sys.__stderr__)
    try:
        L = emu.lib()
        assert L.emu_wave_lanes() == (64 if wave64 else 1)
        L.emu_set_multi_verify.argtypes = [C.c_uint32, C.c_uint32]
        x = ctx(name)
        e = emu.Emu(x["base"])
        n_taxa = int(x["hix"].num_taxa)
        ran = 0
        try:
            for combo in combos:
                if set_tables(L, e, x["case"], combo) is None:
                    continue
                for ver in versions:
                    L.emu_set_search_version(ver)
                    for rid, run in x["runs"].items():
                        rows, n_rows, s2, cnt = e.classify(run["seq"], run["off"], run["seeds"], paired=run["paired"], counts=True, **run["kw"])
                        what = (name, combo[0], "search v%d" % ver, rid)
                        assert_rows((rows, n_rows, s2), run["want"], what)
                        a, u = oracle_tally(x["hix"], run["want"], n_taxa)
                        assert np.array_equal(cnt[:n_taxa], a) and np.array_equal(cnt[n_taxa:], u), what
                        ran += 1
        finally:
            L.emu_set_multi_verify(0, 2); L.emu_set_search_version(2)
            e.close()
        assert ran >= 2 * len(versions)                     # (the sides and the planes can always be made)
    finally:
        faulthandler.cancel_dump_traceback_later()
        emu.use_wave64(was)


@needs_ref
@pytest.mark.parametrize("name", K.kept_names())
def test_emulated_kernels_match_the_oracle(name):
    run_emu(name, COMBOS, (2, 1))


@needs_ref
@pytest.mark.parametrize("name", [n for n in K.kept_names() if K.BY_NAME[n].group in "ABE"])
def test_emulated_wavefront_of_64_lanes_matches_the_oracle(name):
    run_emu(name, [COMBOS[1], COMBOS[2]], (2,), wave64=True)


@needs_ref
@pytest.mark.parametrize("name", [n for n in K.kept_names() if K.BY_NAME[n].build.n <= 5000])
def test_every_row_resolves_as_in_the_oracle(name):
    """try_offset + single LF steps (the emu's resolve tap, the only caller of try_offset) at every row of the index, the rows of the
    boundary table and the last of them included, against the oracle's walk"""
    from emu import emu
    x = ctx(name)
    e = emu.Emu(x["base"])
    try:
        n = x["case"].build.n
        got = [int(e.L.emu_resolve(e.h, r)) for r in range(n + 1)]
        want = [int(x["orc"].L.cfo_resolve_row(x["orc"].h, r)) for r in range(n + 1)]
        assert got == want, (name, [r for r in range(n + 1) if got[r] != want[r]][:10])
    finally:
        e.close()


@pytest.mark.parametrize("tables", ["A", "B", "C", "D", "W1", "W6"])
def test_planner_realises_what_the_gpu_test_expects(tables):
    """the table planner on its own (cf_debug_plan_tables: no device, room to spare) against expected_tables(), the pure function
    of n, ftabChars and offRate that tests/test_gpu_classify_edges.py holds cf_index_describe to: text tables only for n >= 64"""
    import classify_edge_worker as W
    for c in K.CASES:
        b = c.build
        want = W.expected_tables(tables, b.n, b.ftab_chars, b.off_rate)
        p = capi.plan_tables(b.n, 1 << 36, b.ftab_chars, b.off_rate, 4 if c.group == "F" and b.n > 40 * 65535 else 2, **W.index_opts(tables, b.ftab_chars))
        got = dict(wide_ftab_chars=p["K"], text_verify_rate=p["text_rate"], occ_planes=p["planes"], pair_planes=p["pair"], resolve_rate=p["resolve_rate"])
        assert got == {k: want[k] for k in got}, (c.name, tables, got, want)
