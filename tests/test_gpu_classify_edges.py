"""The classifier's kernels on the GPU at the index shapes where they change behaviour: the reads of tests/classifycases.py against
the indexes of the builder's corner cases (groups A - F of tests/buildcases.py), under every table configuration, the general
kernels and the first search version, compared bit for bit with the record of the unmodified reference
(tests/golden/classify_edges.json) and with the oracle, which says where a difference is.

One pytest item is one child process (tests/classify_edge_worker.py): a unit - a group, group F one case a child: its two
2.6-Mbase builds take most of a child's time - under a configuration:

    A          every table automatic, small_range_rows = -1          B          the file's tables only: the sides kernel, real walks
    C          small_range_rows = 4                                   D          text and resolve table at rate 3
    W1 / W6    the wide ftab forced to ftabChars + 1 / min(ftabChars + 6, 12)
    A_general / B_general   CF_POST_FAST=0 CF_SCORE_FAST=0           A_v1       CF_SEARCH_V=1

The tables are asked for through cf_index_options, so that a case's own ftab width and SA rate decide what each means.  The
parent never opens a device.  The child builds every index itself and stops unless its files are the reference builder's
(tests/golden/build_edges.json); it leaves them where the parent's oracle and host-side index read them.

Per case and run (-k 5, -k 1; -k 50 --min-hitlen 15 on group D; mates on eight cases) the parent asserts, with no tolerance: the
TSV's sha256 is the recorded one; rows, order, n_rows and 2ndBest are the oracle's; the device's counters are the tally of the
rows and double on the second pass; the byte form, the packed slot form and (configuration A, the 100-base reads) the dense form
give the same rows.  That the configuration really ran is proved from cf_index_describe against expected_tables(), a pure function
of n, ftabChars and offRate written from planTablesIn's thresholds, and from the op counters summed over the child.  At -t 1
sizeBatch's guard 0.15 L + L / ftabChars + 3 >= 255 falls between 219 and 220 bases (32 + 219 + 3 = 254, 33 + 220 + 3 = 256): the
193 ... 256 class, cut to 219 bases, must show rec_words == 8 in the launch record and, cut to 220, rec_words == 0 (a cut at 217
and the uncut batch, 256 bases, lie further out on either side).

Process hygiene as tests/test_gpu_variants.py: one child at a time, each under the time limit T; a child that ends by a signal,
with status 134 / 139, at T or with an illegal memory access in its stderr latches the module - every later item fails at once and
starts nothing.

The time limit: the slowest child (D-B: group D's 18 indexes, three or four runs each) took 4.4 s on an MI355X (MEASURED_SLOWEST_S
rounds that up for the process start); T is ten times that, at least 60 s: T = 60 s.  Measured on the same run, seconds per item
(165 s for the module's 63 items), units A B C D E F65535 F65536:
    A 2.79 2.81 1.94 3.95 1.39 1.27 1.25; B 2.83 3.11 2.27 4.44 1.53 1.50 1.35; C 2.74 2.53 1.74 3.95 1.24 1.34 1.32;
    D 2.75 2.91 2.04 4.17 1.36 1.29 1.31; W1 2.82 3.04 2.19 4.08 1.50 1.37 1.36; W6 2.90 3.20 2.12 4.32 1.48 1.29 1.43;
    A_general 2.84 3.22 2.17 4.11 1.31 1.32 1.36; B_general 2.63 3.38 1.91 3.82 1.37 1.32 1.31; A_v1 2.56 2.52 1.81 3.59 1.55 1.30 1.32
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import classify_edge_worker as W
import classifycases as K
from centrifuge_amd import capi, reads
from test_gpu_variants import same_rows, tally

pytestmark = pytest.mark.gpu

MEASURED_SLOWEST_S = 5.0
T = max(60.0, 10 * MEASURED_SLOWEST_S)
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "classify_edge_worker.py")

KEPT = K.kept_names()
UNITS = {g: [n for n in KEPT if K.BY_NAME[n].group == g] for g in "ABCDE"}
UNITS.update({n.upper(): [n] for n in KEPT if K.BY_NAME[n].group == "F"})
ITEMS = [(u, cfg) for cfg in W.CONFIGS for u in UNITS]

_outdir = None
_done = {}
_faulted = None
_oracle = {}
_host = {}


@pytest.fixture(scope="module", autouse=True)
def _workdir(tmp_path_factory):
    global _outdir
    _outdir = str(tmp_path_factory.mktemp("cf_classify_edges"))
    yield
    for h in _host.values():
        h.close()
    _host.clear(); _oracle.clear()
    _outdir = None


def child_env(cfg):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CF_") or k in ("CF_AMD_LIB",)}      # no stray knob, no suite-wide switch
    env["CF_DEBUG_KNOBS"] = "1"
    env.update(W.CONFIGS[cfg][1])
    return env


def run_child(unit, cfg):
    global _faulted
    key = (unit, cfg)
    if key in _done:
        if isinstance(_done[key], Exception):
            raise _done[key]
        return _done[key]
    cid = "%s-%s" % key
    if _faulted:
        pytest.fail("not run: an earlier child faulted (%s)" % _faulted)
    out, spec_path = os.path.join(_outdir, cid + ".npz"), os.path.join(_outdir, cid + ".json")
    with open(spec_path, "w") as f:
        json.dump(dict(id=cid, out=out, config=cfg, cases=UNITS[unit], index_dir=os.path.join(_outdir, "idx", cfg)), f)
    try:
        r = subprocess.run([sys.executable, WORKER, spec_path], env=child_env(cfg), timeout=T, capture_output=True, text=True)
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
    print("%s: child %.2f s" % (cid, _done[key][0]["seconds"]))
    return _done[key]


def truth(name, rid, paired, cfg):
    """the run's arrays and the oracle's answer over the index a child has built (the reference builder's own, by its digest).
    Every configuration's child builds into a directory of its own; the parent reads, and keeps open, the files of the first
    configuration that asks (A), which no later child writes to; the other configurations' files go when their item ends"""
    from oracle import oracle as O
    if (name, rid) not in _oracle:
        c = K.BY_NAME[name]
        base = os.path.join(_outdir, "idx", cfg, name, "idx")
        if name not in _host:
            _host[name] = capi.Index(base, host_only=True)
        names, qlens, seq, off, seeds, pr = W.run_arrays(c, paired)
        orc = O.Oracle(base)
        want = orc.classify(seq, off, seeds, len(names), pr, orc.params(**K.RUN_KW[rid]))
        cuts = {}
        if c.build.ftab_chars == 1 and rid == "k5":
            lens = (off[1:] - off[:-1]).astype(np.int64)
            idx = dict(W.class_batches(lens))[2]
            for cut in W.CUTS:
                s, o, sd = W.subset(seq, off, seeds, idx, cut=cut)
                cuts[cut] = orc.classify(s, o, sd, len(idx), False, orc.params(k=5))
        orc.close()
        _oracle[(name, rid)] = dict(names=names, qlens=qlens, want=want, cuts=cuts)
    return _oracle[(name, rid)]


def assert_oracle(got, want, what):
    rows, n_rows, score2 = got
    assert np.array_equal(n_rows, want[1]), (what, "n_rows differ at queries", np.nonzero(n_rows != want[1])[0][:10].tolist())
    assert np.array_equal(score2, want[2]), (what, "2ndBest differs at queries", np.nonzero(score2 != want[2])[0][:10].tolist())
    live = np.arange(want[0].shape[1])[None, :] < want[1][:, None]
    for f in ("tax_id", "unique_id", "score", "hit_len"):
        bad = np.nonzero((rows[f] != want[0][f]) & live)
        assert len(bad[0]) == 0, (what, f, "first at query %d row %d" % (bad[0][0], bad[1][0]))


def check_run(cid, cfg, name, rid, paired, m, A):
    what = "%s %s %s" % (cid, name, rid)
    pre = "%s.%s." % (name, rid)
    x = truth(name, rid, paired, cfg)
    hix = _host[name]
    rows, n_rows, score2 = A[pre + "rows"], A[pre + "n_rows"], A[pre + "score2"]
    assert m["nq"] == len(x["names"]) == len(n_rows), what
    assert_oracle((rows, n_rows, score2), x["want"], what)
    rec = K.load_golden()[name]["runs"][rid]["tsv"]
    got = reads.format_tsv(hix.seqid, x["names"], x["qlens"], rows, n_rows, score2)
    assert got.count("\n") == rec["rows"] and __import__("hashlib").sha256(got.encode("latin1")).hexdigest() == rec["sha256"], what
    # the device's counters are the tally of the rows, and double on the second pass
    a, u = tally(rows, n_rows, hix.num_taxa)
    assert np.array_equal(A[pre + "counts_reads"], a) and np.array_equal(A[pre + "counts_uniq"], u), what
    assert np.array_equal(A[pre + "counts2_reads"], 2 * a) and np.array_equal(A[pre + "counts2_uniq"], 2 * u), what
    # the second pass, the packed slot form, the dense form: the same rows
    assert np.array_equal(A[pre + "score22"], score2) and same_rows(A[pre + "rows2"], A[pre + "n_rows2"], rows, n_rows), what
    assert np.array_equal(A[pre + "score23"], score2) and same_rows(A[pre + "rows3"], A[pre + "n_rows3"], rows, n_rows), what
    if pre + "dense_idx" in A:
        idx = A[pre + "dense_idx"]
        assert len(idx) == 10 and np.array_equal(A[pre + "dense_score2"], score2[idx]), what
        assert same_rows(A[pre + "dense_rows"], A[pre + "dense_n_rows"], rows[idx], n_rows[idx]), what
    else:
        assert not (W.CONFIGS[cfg][0] == "A" and rid == "k5"), what
    env = W.CONFIGS[cfg][1]
    for b in m["batches"]:
        assert b["launch"] == b["launch2"] and b["info"]["slow_post"] == b["info2"]["slow_post"], (what, b)
        if env.get("CF_POST_FAST") == "0":
            assert b["info"]["slow_post"] == b["nq"] and b["info"]["slow_score"] == b["nq"], (what, b)
        want_words = 0 if env.get("CF_SEARCH_V") == "1" else (4, 6, 8, 0)[b["cls"]] if not paired else None
        if want_words is not None and not (K.BY_NAME[name].build.ftab_chars == 1 and b["max_len"] >= 220):
            assert b["launch"]["rec_words"] == want_words, (what, b["cls"], b["launch"])
    # the 8-bit hit count of the strand records, -t 1
    if "cuts" in m:
        full = [b for b in m["batches"] if b["cls"] == 2][0]
        names = [nm for nm, r in K.BY_NAME[name].reads if K.length_class(len(r)) == 2]
        assert any(nm.startswith(b"sw") for nm in names) and full["max_len"] == 256
        v2 = env.get("CF_SEARCH_V") != "1"
        assert full["launch"]["rec_words"] == 0, (what, full["launch"])                                   # (its longest read has 256 bases)
        assert m["cuts"]["217"]["rec_words"] == (8 if v2 else 0), (what, m["cuts"]["217"])
        assert m["cuts"]["219"]["rec_words"] == (8 if v2 else 0) and m["cuts"]["220"]["rec_words"] == 0, (what, m["cuts"])
        for cut in W.CUTS:
            assert_oracle((A[pre + "cut%d_rows" % cut], A[pre + "cut%d_n_rows" % cut], A[pre + "cut%d_score2" % cut]), x["cuts"][cut], (what, "cut", cut))


def check_tables(cid, cfg, name, m):
    b = K.BY_NAME[name].build
    tables = W.CONFIGS[cfg][0]
    want = W.expected_tables(tables, b.n, b.ftab_chars, b.off_rate)
    got = {k: m["describe"][k] for k in want}
    assert got == want, (cid, name, got, want)


@pytest.mark.parametrize("unit,cfg", ITEMS, ids=["%s-%s" % it for it in ITEMS])
def test_classify_edges(unit, cfg):
    cid = "%s-%s" % (unit, cfg)
    meta, A = run_child(unit, cfg)
    try:
        check_item(cid, unit, cfg, meta, A)
    finally:
        if cfg != ITEMS[0][1]:                              # (the first configuration's files are the ones the parent reads)
            for name in UNITS[unit]:
                shutil.rmtree(os.path.join(_outdir, "idx", cfg, name), ignore_errors=True)


def check_item(cid, unit, cfg, meta, A):
    assert meta["id"] == cid and list(meta["cases"]) == UNITS[unit]
    for k, v in W.CONFIGS[cfg][1].items():
        assert meta["knobs"].get(k) == v, (cid, k)
    ops = {f: 0 for f in ("n_ftab_wide", "n_pos_hits", "n_walk", "n_verify")}
    for name in UNITS[unit]:
        m = meta["cases"][name]
        c = K.BY_NAME[name]
        check_tables(cid, cfg, name, m)
        for rid, _args, paired in c.runs():
            check_run(cid, cfg, name, rid, paired, m["runs"][rid], A)
            for b in m["runs"][rid]["batches"]:
                for f in ops:
                    ops[f] += b["ops"][f]
    # the paths ran
    tables, env = W.CONFIGS[cfg]
    group = K.BY_NAME[UNITS[unit][0]].group
    builds = [K.BY_NAME[n].build for n in UNITS[unit]]
    if env.get("CF_SEARCH_V") != "1":
        if tables.startswith("W") or (tables == "A" and any(W.expected_tables("A", b.n, b.ftab_chars, b.off_rate)["wide_ftab_chars"] for b in builds)):
            # (automatic tables widen the ftab only where floor(log4 n) exceeds the file's width: the -t 1 / -t 2 / -t 5 cases of group D)
            assert ops["n_ftab_wide"] > 0, (cid, ops)
    if tables == "A" and group in "BCDEF" and env.get("CF_SEARCH_V") != "1":       # (the position form rests on the text tables, and on the second search version)
        assert ops["n_pos_hits"] > 0, (cid, ops)
    if tables in "BD":
        assert ops["n_walk"] > 0, (cid, ops)
    if tables == "C" and group in "BCDEF":             # (group A: texts under 64 bases have no text tables to finish a range against)
        assert ops["n_verify"] > 0, (cid, ops)
