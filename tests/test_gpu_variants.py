"""Every kernel variant and fallback of the hot path, forced on the GPU, against the goldens and the oracle.

cf_device.hip picks its kernels from knobs that are read once per process (centrifuge_amd/csrc/cf_knobs.hpp), so ONE pytest item
here is ONE child process (tests/variant_worker.py) started with the variant's CF_* variables, over one table setup:

    A  every table automatic: planes, pair planes, text and resolve table at every row, hits in the position form (small_range_rows
       = -1: the repeat probe would turn the golden index's small ranges on by itself, and the plain planes kernels would never run)
    B  the file's own tables only: the two-lane search kernel over the sides, real walks
    C  small_range_rows = 4: the search kernels that finish small ranges against the text
    D  text and resolve table sampled (rate 3): sampled text, forced steps of the walk

Every child classifies the golden cases k5 / k1 / pe_k1 / r250_k5 / minhit15 of synth_small and example/default (compared byte for
byte with the reference's TSV, counters with its report) and the five common.EDGE_CASES batches (compared with the oracle, computed
here on the CPU), each of them twice (plan + classify again: the same rows; the packed egress against the k-slot one), and the
device's per-taxon counters are compared with a tally of the rows made here.  No item passes on equal rows alone: each proves
from the launch record (cf_batch_debug_launch), the op counters or the `info` of cf_batch_wait that its variant really ran — a
mistyped knob would otherwise test the default once more.

A child's environment is the parent's WITHOUT its CF_* variables (CF_AMD_LIB apart), plus CF_DEBUG_KNOBS=1, the setup's and the
variant's knobs: a stray knob or a suite-wide switch such as CF_TEST_SMALL_RANGE_ROWS would turn a row into another variant than
the one it proves, so this module, unlike the rest of the suite, does not run under such a switch.

Process hygiene: one child at a time, each under a time limit; a child that ends by a signal, with status 134 / 139, at its time
limit or with an illegal memory access in its stderr stops the module — every later item fails at once and starts nothing.

The time limit: the slowest child of the default variant (no kernel knob; default-A, which also classifies the 8x and 40x
replicated batches) took 1.5 s on an MI355X, process start to result (MEASURED_DEFAULT_S); T is ten times that, at least 60 s:
T = 60 s.  Measured on the same run, seconds per item (50.2 s for the module's 47 items):
    default A 1.48 B 1.20 C 0.85 D 0.82; post_general A 0.88 B 0.94 C 0.92; score_general A 0.86 B 0.98 C 0.91;
    both_general A 0.84 B 0.92 C 0.94 D 0.89; direct_refs0 A 0.86; walk2_emitted A 0.86; walk2 B 0.91 D 1.00; search_v1 A 0.92 B 1.09;
    lazy_hits0 A 0.89 D 0.81; lazy_n1 A 0.88; lazy_n2 A 0.91; self_records0 A 0.89; rev_words0 A 0.88; pos_hits0 A 0.91 D 0.93;
    pos_shift5 A 0.92 D 0.89; count_bits1 / 2 / 4 A 0.95 / 0.88 / 0.82; post_lds A 0.75 C 0.90; post_lds_general A 0.86;
    score_lds16 A 1.10 C 1.09; score_lds4 A 1.10 C 1.10; rows_per_query1 B 1.94 C 1.82; early_score A 1.51;
    tail_stream1 A 1.46; tail_stream2 A 1.48; blocks_per_cu1 A 0.96 B 1.13
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import variant_worker as W
from centrifuge_amd import capi, reads

pytestmark = pytest.mark.gpu

MEASURED_DEFAULT_S = 1.5          # slowest default item (default-A, with the 8x and 40x replicated batches): the child's whole wall clock on an MI355X
T = max(60.0, 10 * MEASURED_DEFAULT_S)

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "variant_worker.py")

# ---- table setups: (environment, cf_index_options)
SETUPS = {
    "A": ({}, {"small_range_rows": -1}),
    "B": ({"CF_WIDE_FTAB": "0", "CF_DENSE_SA_RATE": "4", "CF_TEXT_VERIFY_RATE": "-1", "CF_OCC_PLANES": "0"}, {}),
    "C": ({}, {"small_range_rows": 4}),
    "D": ({"CF_TEXT_VERIFY_RATE": "3", "CF_DENSE_SA_RATE": "3"}, {}),
}

GOLDEN = [dict(kind="golden", arch="synth_small", name=n) for n in ("k5", "k1", "pe_k1", "r250_k5", "minhit15")] + \
         [dict(kind="golden", arch="example", name="default")]
EDGES = [dict(kind="edge", idx=i) for i in range(len(common.EDGE_CASES))]
STANDARD = GOLDEN + EDGES
REP8, REP40 = dict(kind="replicated", copies=8), dict(kind="replicated", copies=40)
K50 = dict(kind="golden", arch="synth_small", name="k50")


def V(env, setups, proof, **spec):
    return dict(env=env, setups=setups, proof=proof, spec=spec)


# ---- the matrix: variant -> knobs, table setups, what must be proved beyond equal rows, extras of the child's spec
MATRIX = {
    "default":         V({}, "ABCD", "default", kreport=True, extra=[REP8], extra_by_setup={"A": [REP40], "B": [REP40]}),
    "post_general":    V({"CF_POST_FAST": "0"}, "ABC", "post_general"),
    "score_general":   V({"CF_SCORE_FAST": "0"}, "ABC", "score_general"),
    "both_general":    V({"CF_POST_FAST": "0", "CF_SCORE_FAST": "0"}, "ABCD", "both_general"),
    "direct_refs0":    V({"CF_DIRECT_REFS": "0"}, "A", "direct_refs0"),
    "walk2_emitted":   V({"CF_DIRECT_REFS": "0", "CF_WALK_V": "2"}, "A", "walk2", walk3_from="direct_refs0"),
    "walk2":           V({"CF_WALK_V": "2"}, "BD", "walk2", walk3_from="default"),
    "search_v1":       V({"CF_SEARCH_V": "1"}, "AB", "search_v1"),
    "lazy_hits0":      V({"CF_LAZY_HITS": "0"}, "AD", "lazy_hits0"),
    "lazy_n1":         V({"CF_LAZY_N": "1"}, "A", "lazy_n1"),
    "lazy_n2":         V({"CF_LAZY_N": "2"}, "A", "lazy_n2"),
    "self_records0":   V({"CF_SELF_RECORDS": "0"}, "A", "self_records0"),
    "rev_words0":      V({"CF_REV_WORDS": "0"}, "A", "rev_words0"),
    "pos_hits0":       V({"CF_POS_HITS": "0"}, "AD", "pos_hits0"),
    "pos_shift5":      V({"CF_POS_SHIFT": "5"}, "AD", "pos_shift5"),
    "count_bits1":     V({"CF_COUNT_SLOT_BITS": "1"}, "A", "count_bits", kreport=True, extra=[REP8]),
    "count_bits2":     V({"CF_COUNT_SLOT_BITS": "2"}, "A", "count_bits", kreport=True, extra=[REP8]),
    "count_bits4":     V({"CF_COUNT_SLOT_BITS": "4"}, "A", "count_bits", kreport=True, extra=[REP8]),
    "post_lds":        V({"CF_POST_LDS": "1"}, "AC", "post_lds"),
    "post_lds_general": V({"CF_POST_LDS": "1", "CF_POST_FAST": "0"}, "A", "post_lds"),
    "score_lds16":     V({"CF_SCORE_LDS_ROWS": "16", "CF_SCORE_FAST": "0"}, "AC", "score_lds", extra=[K50], planned_per_query=["synth_small/k5"]),
    "score_lds4":      V({"CF_SCORE_LDS_ROWS": "4", "CF_SCORE_LDS_SPARSE": "4", "CF_SCORE_FAST": "0"}, "AC", "score_lds", extra=[K50], planned_per_query=["synth_small/k5"]),
    "rows_per_query1": V({"CF_ROWS_PER_QUERY": "1"}, "BC", "rows_per_query", rows_per_pass_div=5, extra=[REP8]),
    "early_score":     V({"CF_EARLY_SCORE": "1"}, "A", "early_score", in_flight=True),
    "tail_stream1":    V({"CF_TAIL_STREAM": "1"}, "A", "tail_stream", in_flight=True),
    "tail_stream2":    V({"CF_TAIL_STREAM": "2"}, "A", "tail_stream", in_flight=True),
    "blocks_per_cu1":  V({"CF_BLOCKS_PER_CU": "1"}, "AB", "blocks_per_cu", extra=[REP40]),
}
ITEMS = [(v, s) for v, row in MATRIX.items() for s in row["setups"]]


def matrix_knobs():
    """every CF_* variable a row or a setup of the matrix sets (tests/test_variant_matrix.py)"""
    names = set()
    for row in MATRIX.values():
        names |= set(row["env"])
    for env, _ in SETUPS.values():
        names |= set(env)
    return names


# ---- running the children
_outdir = None       # the session's directory for specs and results (the fixture below)
_done = {}            # (variant, setup) -> (meta, arrays) or an Exception
_faulted = None       # id of the child that faulted: nothing is started after it


@pytest.fixture(scope="module", autouse=True)
def _workdir(tmp_path_factory):
    global _outdir
    _outdir = str(tmp_path_factory.mktemp("cf_variants"))
    yield
    _outdir = None


def child_spec(variant, setup, out):
    row = MATRIX[variant]
    sp = row["spec"]
    inputs = STANDARD + list(sp.get("extra", [])) + list(sp.get("extra_by_setup", {}).get(setup, []))
    spec = dict(id="%s-%s" % (variant, setup), out=out, index_opts=SETUPS[setup][1], inputs=inputs)
    for k in ("kreport", "in_flight", "rows_per_pass_div", "planned_per_query"):
        if k in sp:
            spec[k] = sp[k]
    return spec


def child_env(variant, setup):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CF_") or k in ("CF_AMD_LIB",)}      # no stray knob, no suite-wide switch
    env["CF_DEBUG_KNOBS"] = "1"
    env.update(SETUPS[setup][0])
    env.update(MATRIX[variant]["env"])
    return env


def run_child(variant, setup):
    """the child's (meta, arrays): run once per session, whoever asks first"""
    global _faulted
    key = (variant, setup)
    if key in _done:
        if isinstance(_done[key], Exception):
            raise _done[key]
        return _done[key]
    cid = "%s-%s" % key
    if _faulted:
        pytest.fail("not run: an earlier variant faulted (%s)" % _faulted)
    out = os.path.join(_outdir, cid + ".npz")
    spec_path = os.path.join(_outdir, cid + ".json")
    with open(spec_path, "w") as f:
        json.dump(child_spec(variant, setup, out), f)
    try:
        r = subprocess.run([sys.executable, WORKER, spec_path], env=child_env(variant, setup), timeout=T, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _faulted = cid
        pytest.fail("%s: no result within %.0f s: counted as hung, nothing more is started" % (cid, T))
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr:
        _faulted = cid
        pytest.fail("%s: the child faulted (status %d), nothing more is started\n%s" % (cid, r.returncode, r.stderr[-4000:]))
    if r.returncode != 0:
        _done[key] = AssertionError("%s: the child failed (status %d)\n%s" % (cid, r.returncode, r.stderr[-4000:]))
        raise _done[key]
    _done[key] = W.load_result(out)
    os.remove(out); os.remove(spec_path)
    print("%s: child %.2f s (%s)" % (cid, _done[key][0]["seconds"], ", ".join("%s %.2f" % (m["id"], m["seconds"]) for m in _done[key][0]["inputs"])))
    return _done[key]


# ---- what the children are compared with (made once, on the CPU)
_inputs, _oracle_rows, _host_ix = {}, {}, {}


def the_input(inp):
    k = W.input_id(inp)
    if k not in _inputs:
        _inputs[k] = W.build_input(inp)
    return _inputs[k]


def host_index(arch):
    if arch not in _host_ix:
        d, _ = common.golden(arch)
        _host_ix[arch] = capi.Index(os.path.join(d, "idx"), host_only=True)
    return _host_ix[arch]


def oracle_rows(inp):
    from oracle import oracle as O
    k = W.input_id(inp)
    if k not in _oracle_rows:
        x = the_input(inp)
        d, _ = common.golden(x["arch"])
        orc = O.Oracle(os.path.join(d, "idx"))
        _oracle_rows[k] = orc.classify(x["seq"], x["off"], x["seeds"], x["nq"], x["paired"], orc.params(**x["kw"]))
        orc.close()
    return _oracle_rows[k]


def tally(rows, n_rows, n_taxa):
    """SpeciesMetrics::addSpeciesCounts over the rows: every printed row a read of its taxon (no row: of taxon 0), the row of a
    query that prints at most one also a unique read"""
    a, u = np.zeros(n_taxa, dtype=np.uint64), np.zeros(n_taxa, dtype=np.uint64)
    k = rows.shape[1]
    live = np.arange(k)[None, :] < n_rows[:, None]
    np.add.at(a, rows["taxon_idx"][live], 1)
    a[0] += int(np.count_nonzero(n_rows == 0))
    one = n_rows == 1
    np.add.at(u, rows["taxon_idx"][one, 0], 1)
    u[0] += int(np.count_nonzero(n_rows == 0))
    return a, u


def same_rows(ra, na, rb, nb):
    """the used slots of two [nq, k] row arrays"""
    if not np.array_equal(na, nb):
        return False
    live = np.arange(ra.shape[1])[None, :] < na[:, None]
    return bool(np.array_equal(ra[live], rb[live]))


def check_input(cid, i, inp, m, A, by_id):
    """rows, order, 2ndBest, counters of one input of one child against the reference / the oracle; the second pass; the packed egress"""
    x = the_input(inp)
    pre = "in%d." % i
    rows, n_rows, score2 = A[pre + "rows"], A[pre + "n_rows"], A[pre + "score2"]
    what = "%s %s" % (cid, m["id"])
    assert m["nq"] == x["nq"] == len(n_rows), what
    hix = host_index(x["arch"])
    if inp["kind"] == "golden":
        got = reads.format_tsv(hix.seqid, x["names"], x["qlens"], rows, n_rows, score2)
        ref = open(os.path.join(x["dir"], x["case"]["tsv"])).read()
        assert got == ref, what + "\n" + common.first_diff(got, ref)
        taxa = hix.taxon_ids()
        mine = {int(t): (int(a), int(u)) for t, a, u in zip(taxa, A[pre + "counts_reads"], A[pre + "counts_uniq"]) if t != 0 and a}
        rep = {}
        for ln in open(os.path.join(x["dir"], x["case"]["report"])).read().splitlines()[1:]:
            f = ln.split("\t")
            rep[int(f[1])] = (int(f[4]), int(f[5]))
        assert mine == rep, what
    elif inp["kind"] == "edge":
        want = oracle_rows(inp)
        assert np.array_equal(n_rows, want[1]) and np.array_equal(score2, want[2]), what
        for q in range(x["nq"]):
            for r in range(int(want[1][q])):
                g, w = rows[q, r], want[0][q, r]
                assert (int(g["tax_id"]), int(g["unique_id"]), int(g["score"]), int(g["hit_len"])) == \
                       (int(w["tax_id"]), int(w["unique_id"]), int(w["score"]), int(w["hit_len"])), (what, q, r)
    else:                                   # every copy of a read prints the rows of the original, checked against the TSV above
        j = by_id[W.input_id(x["base"])]
        r0, n0, s0 = A["in%d.rows" % j], A["in%d.n_rows" % j], A["in%d.score2" % j]
        perm = x["perm"]
        assert np.array_equal(score2, s0[perm]) and same_rows(rows, n_rows, r0[perm], n0[perm]), what
    # the device's counters are the tally of the rows, whichever kernel counted them (LDS slots, far atomics, the score kernel)
    a, u = tally(rows, n_rows, hix.num_taxa)
    assert np.array_equal(A[pre + "counts_reads"], a) and np.array_equal(A[pre + "counts_uniq"], u), what
    # the second pass over the resident batch: the same rows, counted once more; the packed egress holds exactly the used slots
    assert np.array_equal(A[pre + "score22"], score2) and same_rows(A[pre + "rows2"], A[pre + "n_rows2"], rows, n_rows), what
    assert np.array_equal(A[pre + "counts2_reads"], 2 * a) and np.array_equal(A[pre + "counts2_uniq"], 2 * u), what
    assert np.array_equal(A[pre + "cn_rows"], n_rows) and np.array_equal(A[pre + "cscore2"], score2), what
    live = np.arange(rows.shape[1])[None, :] < n_rows[:, None]
    assert np.array_equal(A[pre + "crows"], rows[live]), what
    assert m["launch"] == m["launch2"] and m["info"]["slow_post"] == m["info2"]["slow_post"] and m["info"]["slow_score"] == m["info2"]["slow_score"], what
    if pre + "kreport" in A:
        assert m["kreport_reads"] == x["nq"] and int(A[pre + "kreport"].sum()) == x["nq"], what
    if pre + "lim_rows" in A:               # a row workspace of a fifth of the planned rows: further passes, the same rows, counted once
        packed = capi.unpack_rows(A[pre + "lim_rows"], np.concatenate([[0], np.cumsum(A[pre + "lim_n_rows"])]).astype(np.uint64), A[pre + "lim_n_rows"], rows.shape[1])
        assert np.array_equal(A[pre + "lim_score2"], score2) and same_rows(packed, A[pre + "lim_n_rows"], rows, n_rows), what
        assert np.array_equal(A[pre + "lim_counts_reads"], a) and np.array_equal(A[pre + "lim_counts_uniq"], u), what
        if m["info"]["planned_sa_rows"] >= 10:
            assert m["lim_info"]["row_passes"] > 1 and m["lim_launch"]["passes"] == m["lim_info"]["row_passes"], (what, m["lim_info"])
    if "fl_runs" in m:                      # two slots, three batches each, always one in flight behind the other
        assert m["fl_runs"] == 6, what
        for r in range(6):
            packed = capi.unpack_rows(A[pre + "fl%d_rows" % r], np.concatenate([[0], np.cumsum(A[pre + "fl%d_n_rows" % r])]).astype(np.uint64), A[pre + "fl%d_n_rows" % r], rows.shape[1])
            assert np.array_equal(A[pre + "fl%d_score2" % r], score2) and same_rows(packed, A[pre + "fl%d_n_rows" % r], rows, n_rows), (what, r)
            assert m["fl_launch"][r] == dict(m["launch"], passes=m["fl_launch"][r]["passes"]), (what, r)
        assert np.array_equal(A[pre + "fl_counts_reads"], 6 * a) and np.array_equal(A[pre + "fl_counts_uniq"], 6 * u), what


# ---- the table setups, proved from cf_index_describe and the launch record (synth_small; the worked example's index is too small for some tables)
def check_setup(cid, setup, variant, meta):
    cfg = meta["index"]["synth_small"]
    env = MATRIX[variant]["env"]
    if setup == "A":
        assert cfg["occ_planes"] == 1 and cfg["pair_planes"] == 1 and cfg["text_verify_rate"] == 0 and cfg["resolve_rate"] == 0 and cfg["small_range_rows"] == 0, (cid, cfg)
        assert (cfg["walk_bound"] > 0) == (env.get("CF_POS_HITS") != "0"), (cid, cfg)
    elif setup == "B":
        assert cfg["occ_planes"] == 0 and cfg["pair_planes"] == 0 and cfg["text_verify_rate"] == -1 and cfg["resolve_rate"] == 4 and cfg["wide_ftab_chars"] == 0, (cid, cfg)
    elif setup == "C":
        assert cfg["small_range_rows"] == 4 and cfg["occ_planes"] == 1 and cfg["text_verify_rate"] >= 0, (cid, cfg)
    else:
        assert cfg["occ_planes"] == 1 and cfg["text_verify_rate"] == 3 and cfg["resolve_rate"] == 3, (cid, cfg)
    for m in meta["inputs"]:
        if m["id"].startswith("example/") or env.get("CF_SEARCH_V") == "1":
            continue
        rec = m["launch"]
        if rec["rec_words"] == 0:
            assert rec["search_form"] == "words", (cid, m["id"], rec)          # reads beyond 256 bases: the byte-window kernel
        elif setup == "B":
            assert rec["search_form"] == "sides" and rec["walk_version"] in (2, 3) and rec["direct_refs"] == 0, (cid, m["id"], rec)
        elif setup == "C":
            assert rec["search_form"] == "multi", (cid, m["id"], rec)
        else:
            assert rec["search_form"].startswith("planes"), (cid, m["id"], rec)
        if setup == "D":
            assert rec["walk_version"] in (2, 3) and rec["direct_refs"] == 0, (cid, m["id"], rec)


def synth(meta):
    return [m for m in meta["inputs"] if not m["id"].startswith("example/")]


def searched_reads(inp):
    """N-free reads of 32 bases or more: both strands are searched, each search starts at the ftab"""
    x = the_input(inp)
    off = x["off"].astype(np.int64)
    return sum(1 for r in range(len(off) - 1) if off[r + 1] - off[r] >= 32 and not np.any(x["seq"][off[r]:off[r + 1]] > 3))


# ---- what each variant must prove beyond equal rows
def prove(cid, variant, setup, meta, inputs):
    row = MATRIX[variant]
    proof, env = row["proof"], row["env"]
    ms = meta["inputs"]
    for k, v in env.items():
        assert meta["knobs"].get(k) == v, (cid, k)
    L = lambda m: m["launch"]      # noqa: E731
    # what holds whatever the variant: the general kernels took every query exactly when their common-case kernel is off
    for m in ms:
        pf, sf = env.get("CF_POST_FAST", "1") != "0", env.get("CF_SCORE_FAST", "1") != "0"
        assert L(m)["post_fast"] == int(pf) and L(m)["score_fast"] == int(sf), (cid, m["id"], L(m))
        if not pf:
            assert m["info"]["slow_post"] == m["nq"], (cid, m["id"], m["info"])
        elif m["nq"] >= 100:
            assert m["info"]["slow_post"] < m["nq"], (cid, m["id"], m["info"])
        if not sf:
            assert m["info"]["slow_score"] == m["nq"] and L(m)["direct_refs"] == 0, (cid, m["id"], m["info"])
        elif m["nq"] >= 100:
            assert m["info"]["slow_score"] < m["nq"], (cid, m["id"], m["info"])
        assert L(m)["passes"] == m["info"]["row_passes"] >= 1, (cid, m["id"])
    if proof == "default":
        for m in synth(meta):
            assert L(m)["lazy_hits"] == 1 and L(m)["early_score"] == 0 and L(m)["tail_stream"] == 0 and L(m)["post_cap_hits"] == 0 and L(m)["score_cap_rows"] == 0, (cid, m["id"], L(m))
            assert L(m)["count_direct"] == 1 and L(m)["pos_shift"] == 14, (cid, m["id"], L(m))
            if setup == "A":
                assert L(m)["direct_refs"] == 1 and L(m)["walk_version"] == 0 and L(m)["pos_form"] == 1, (cid, m["id"], L(m))
                if L(m)["rec_words"]:
                    assert L(m)["search_form"] == "planes" and L(m)["self_records"] == 1 and L(m)["rev_words"] == 1, (cid, m["id"], L(m))
            if setup in "BD":
                assert L(m)["walk_version"] == 3, (cid, m["id"], L(m))
        assert {L(m)["rec_words"] for m in synth(meta)} == {0, 4, 6, 8}, cid       # every strand-record size and the byte-window kernel
        if setup in "BD":
            assert sum(m["ops"]["n_walk"] for m in ms) > 0, cid
    elif proof in ("post_general", "both_general"):
        pass                                  # (slow_post == n_queries, above)
    elif proof == "score_general":
        for m in synth(meta):                 # no direct references then: rows are emitted and walked
            assert L(m)["walk_version"] == 3, (cid, m["id"], L(m))
        assert sum(m["ops"]["n_rows"] for m in ms) > 0, cid
    elif proof == "direct_refs0":
        for m in ms:
            assert L(m)["direct_refs"] == 0 and L(m)["walk_version"] == 3, (cid, m["id"], L(m))
        assert sum(m["ops"]["n_rows"] for m in ms) > 0, cid
    elif proof == "walk2":
        base = run_child(row["spec"]["walk3_from"], setup)[0]
        for m, m0 in zip(ms, base["inputs"]):
            assert m["id"] == m0["id"] and L(m)["walk_version"] == 2 and L(m0)["walk_version"] == 3, (cid, m["id"], L(m), L(m0))
            assert m["ops"]["n_walk"] == m0["ops"]["n_walk"] and m["ops"]["n_rows"] == m0["ops"]["n_rows"], (cid, m["id"], m["ops"], m0["ops"])
        if setup in "BD":
            assert sum(m["ops"]["n_walk"] for m in ms) > 0, cid
    elif proof == "search_v1":
        for m, inp in zip(ms, inputs):
            assert L(m)["search_form"] == "words" and L(m)["rec_words"] == 0, (cid, m["id"], L(m))
            assert m["ops"]["n_ftab_wide"] == 0 and m["ops"]["n_ftab"] >= searched_reads(inp), (cid, m["id"], m["ops"])
        assert sum(searched_reads(inp) for inp in inputs) > 1000
    elif proof == "lazy_hits0":
        for m in ms:
            assert L(m)["lazy_hits"] == 0, (cid, m["id"], L(m))
    elif proof in ("lazy_n1", "lazy_n2"):
        seen = set()
        for m in synth(meta):
            w = L(m)["rec_words"]
            want = "words" if w == 0 else "planes-lazy1" if (proof == "lazy_n1" and w == 4) else "planes-lazy2" if (proof == "lazy_n2" and w in (6, 8)) else "planes"
            assert L(m)["search_form"] == want, (cid, m["id"], L(m))
            seen.add((w, want))
        assert seen >= ({(4, "planes-lazy1")} if proof == "lazy_n1" else {(6, "planes-lazy2"), (8, "planes-lazy2")}), (cid, seen)
        assert {m["id"]: L(m)["rec_words"] for m in ms}["synth_small/r250_k5"] == 8
    elif proof == "self_records0":
        for m in ms:
            assert L(m)["self_records"] == 0 and L(m)["rev_words"] == 0, (cid, m["id"], L(m))
    elif proof == "rev_words0":
        for m in ms:
            assert L(m)["rev_words"] == 0 and L(m)["self_records"] == (1 if L(m)["rec_words"] else 0), (cid, m["id"], L(m))
    elif proof == "pos_hits0":
        base = run_child("default", setup)[0]
        some = 0
        for m, m0 in zip(ms, base["inputs"]):
            assert m["id"] == m0["id"] and L(m)["pos_form"] == 0 and m["ops"]["n_pos_hits"] == 0, (cid, m["id"], L(m), m["ops"])
            if m["id"].startswith("example/"):
                continue
            assert L(m0)["pos_form"] == 1, (cid, m["id"], L(m0))
            for f in ("n_pair", "n_pair2", "n_ftab", "n_ftab_wide", "n_verify"):
                assert m["ops"][f] == m0["ops"][f], (cid, m["id"], f, m["ops"], m0["ops"])
            assert m0["ops"]["n_single"] <= m["ops"]["n_single"], (cid, m["id"])
            if m["ops"]["n_verify"] > 20 and L(m)["rec_words"]:
                assert m0["ops"]["n_pos_hits"] > m["ops"]["n_verify"] // 4, (cid, m["id"], m0["ops"])
                some += 1
        assert some >= 3, cid
    elif proof == "pos_shift5":
        some = 0
        for m in synth(meta):
            assert L(m)["pos_form"] == 1 and L(m)["pos_shift"] == 5, (cid, m["id"], L(m))
            if m["ops"]["n_verify"] > 20 and L(m)["rec_words"]:
                assert m["ops"]["n_pos_hits"] > m["ops"]["n_verify"] // 4, (cid, m["id"], m["ops"])
                some += 1
        assert some >= 3, cid
    elif proof == "count_bits":
        bits = int(env["CF_COUNT_SLOT_BITS"])
        base_meta, base_arr = run_child("default", setup)
        A = _done[(variant, setup)][1]
        for i, (m, m0) in enumerate(zip(ms, base_meta["inputs"])):
            assert m["id"] == m0["id"], cid
            assert meta["index"]["synth_small"]["num_taxa"] > 1 << bits and meta["index"]["example"]["num_taxa"] > 1 << bits
            assert L(m)["count_slot_bits"] == bits and L(m)["count_direct"] == 0 and L(m0)["count_direct"] == 1, (cid, m["id"], L(m))
            for f in ("counts_reads", "counts_uniq", "counts_single", "kreport"):
                assert np.array_equal(A["in%d.%s" % (i, f)], base_arr["in%d.%s" % (i, f)]), (cid, m["id"], f)
            assert m["kreport_reads"] == m0["kreport_reads"], (cid, m["id"])
        a = A["in%d.counts_reads" % [m["id"] for m in ms].index("rep8")]
        assert int(np.count_nonzero(a)) > 1 << bits, (cid, a)       # more taxa in one chunk than slots: probing, overflow to the far atomics
    elif proof == "post_lds":
        ids = {m["id"]: L(m)["post_cap_hits"] for m in ms}
        assert all(v > 0 for v in ids.values()), (cid, ids)
        assert ids["synth_small/r250_k5"] > ids["synth_small/k5"], (cid, ids)                        # the scratch is sized by the batch's longest read
        # the general kernel did get queries with the scratch in place: the chimeras (a long hit on both strands) among the N-rich edge
        # reads of 100 bases (edge0: lists that fit) and of 255 / 256 bases (edge2); with CF_POST_FAST=0 every query, above
        sp = {m["id"]: m["info"]["slow_post"] for m in ms}
        assert sp["edge0"] > 0 and sp["edge2"] > 0, (cid, sp)
    elif proof == "score_lds":
        cap, sparse = int(env["CF_SCORE_LDS_ROWS"]), int(env.get("CF_SCORE_LDS_SPARSE", "2"))
        A = _done[(variant, setup)][1]
        for m in ms:
            assert L(m)["score_cap_rows"] == cap and L(m)["score_sparse"] == sparse, (cid, m["id"], L(m))
        # above the cap: a query plans at least the rows it prints
        i = [m["id"] for m in ms].index("synth_small/k50" if cap > 5 else "synth_small/k5")
        assert int(A["in%d.n_rows" % i].max()) > cap, (cid, int(A["in%d.n_rows" % i].max()))
        # below it (the scratch in LDS is used): the planned rows of k5's first queries, each classified once more as a batch of its own
        j = [m["id"] for m in ms].index("synth_small/k5")
        planned = A["in%d.planned" % j]
        assert len(planned) == 300 and np.all(planned >= A["in%d.n_rows" % j][:300]), cid          # (a query plans at least the rows it prints)
        below = int(np.count_nonzero((planned >= 1) & (planned <= cap)))
        assert below > 100, (cid, below, np.bincount(planned.astype(np.int64)).tolist())
    elif proof == "rows_per_query":
        over = [m for m in ms if m["info"]["planned_sa_rows"] > max(1024, m["nq"])]
        assert over and any(m["id"] == "rep8" for m in over), (cid, [(m["id"], m["info"]) for m in ms])
        for m in over:
            assert m["info"]["row_passes"] > 1, (cid, m["id"], m["info"])
        assert any("lim_info" in m and m["lim_info"]["row_passes"] > 1 for m in ms), cid
    elif proof == "early_score":
        for m in synth(meta):
            assert L(m)["early_score"] == 1 and L(m)["direct_refs"] == 1, (cid, m["id"], L(m))
    elif proof == "tail_stream":
        for m in ms:
            assert L(m)["tail_stream"] == int(env["CF_TAIL_STREAM"]), (cid, m["id"], L(m))
    elif proof == "blocks_per_cu":
        base = run_child("default", setup)[0]
        m = [x for x in ms if x["id"] == "rep40"][0]
        m0 = [x for x in base["inputs"] if x["id"] == "rep40"][0]
        lanes = 2 if L(m)["search_form"] == "sides" else 1
        assert L(m)["search_blocks"] < L(m0)["search_blocks"], (cid, L(m), L(m0))
        assert 2 * m["n_reads"] * lanes > 2 * L(m)["search_blocks"] * 256, (cid, m["n_reads"], L(m))     # the work queue wraps, more than once
    else:
        raise AssertionError("no proof named %r" % proof)


@pytest.mark.parametrize("variant,setup", ITEMS, ids=["%s-%s" % it for it in ITEMS])
def test_variant(variant, setup):
    cid = "%s-%s" % (variant, setup)
    meta, A = run_child(variant, setup)
    inputs = child_spec(variant, setup, "")["inputs"]
    assert meta["id"] == cid and [m["id"] for m in meta["inputs"]] == [W.input_id(x) for x in inputs]
    by_id = {m["id"]: i for i, m in enumerate(meta["inputs"])}
    for i, (inp, m) in enumerate(zip(inputs, meta["inputs"])):
        check_input(cid, i, inp, m, A, by_id)
    check_setup(cid, setup, variant, meta)
    prove(cid, variant, setup, meta, inputs)
