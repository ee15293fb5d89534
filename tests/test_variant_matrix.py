"""Keeps the GPU variant matrix (tests/test_gpu_variants.py) honest, without a GPU: every CF_* knob cf_device.hip reads is forced
by a row of the matrix, by another GPU test, or is exempt for a stated reason — a knob added later without a GPU test fails here.
Also the worker's spec / result round trip, on made-up data."""
import json
import os
import re

import numpy as np

import common
import test_gpu_variants as G
import variant_worker as W
from centrifuge_amd import capi

CSRC = os.path.join(common.ROOT, "centrifuge_amd", "csrc")

# knobs other GPU tests force: knob -> the test file that must mention it
FORCED_ELSEWHERE = {
    "CF_DENSE_BY_POS": "test_gpu_parity.py",
    "CF_PAIR_PLANES": "test_gpu_scale.py",
    "CF_BGZF_OUT_MEMBER": "test_gpu_deflate.py",
    "CF_TEST_FAIL_COMM": "test_gpu_cli.py",
    "CF_RESTORE_SHIFT": "test_tools.py",
}
# knobs no GPU test forces, and why that is accepted
EXEMPT = {
    "CF_ISA_RATE": "spacing of the inverse sample: a table size, read by no kernel choice; the position-form rows run over both of its automatic values (setups A and D)",
    "CF_MULTI_VERIFY": "the knob form of cf_index_options::small_range_rows, which setup C sets through the option",
    "CF_DROP_SIDES": "the knob form of cf_index_options::sides, forced through the option by test_async_abi.py",
    "CF_RESTORE_VERBOSE": "prints the inverse-BWT phases, computes nothing",
    "CF_TEXT_VERIFY_MIN_RUN": "tuning threshold of the text comparison, measured by tools/gpu/run.sh only",
    "CF_MULTI_MIN_RUN": "tuning threshold of the small-range kernels, measured by tools/gpu/run.sh only",
    "CF_TABLE_PLANNER": "0 = the fixed table priorities of earlier rounds, kept for measurements; the planner itself is tested on the CPU (test_plan_emu.py)",
    "CF_INFLATE_LANES": "the one-lane-per-member inflater, kept as the comparison of the two forms for measurements",
}


def knobs_read_by_the_device_layer():
    src = open(os.path.join(CSRC, "cf_device.hip")).read()
    return set(re.findall(r'"(CF_[A-Z0-9_]+)"', src))


def test_every_knob_of_the_device_layer_is_forced_on_the_gpu_or_exempt():
    read = knobs_read_by_the_device_layer()
    assert len(read) > 30 and "CF_POST_FAST" in read and "CF_POS_SHIFT" in read
    matrix = G.matrix_knobs()
    assert matrix <= read, "the matrix sets knobs the device layer does not read (a mistyped name?): %s" % sorted(matrix - read)
    for knob, path in FORCED_ELSEWHERE.items():
        assert knob in open(os.path.join(common.ROOT, "tests", path)).read(), (knob, path)
    for knob, why in EXEMPT.items():
        assert knob in read and len(why) > 20, knob           # (an exemption of a knob that is gone is stale)
    claimed = [matrix, set(FORCED_ELSEWHERE), set(EXEMPT)]
    assert not (claimed[0] & claimed[1]) and not (claimed[0] & claimed[2]) and not (claimed[1] & claimed[2])
    missing = read - matrix - set(FORCED_ELSEWHERE) - set(EXEMPT)
    assert not missing, "knobs of cf_device.hip that no GPU test forces: %s (add a row to tests/test_gpu_variants.py)" % sorted(missing)
    # the header that documents the knobs names every kernel-variant knob of the matrix, and this module's sibling as their test
    doc = open(os.path.join(CSRC, "cf_knobs.hpp")).read()
    for knob in matrix:
        assert knob in doc, knob
    assert "tests/test_gpu_variants.py" in doc


def test_matrix_is_well_formed():
    ids = ["%s-%s" % it for it in G.ITEMS]
    assert len(ids) == len(set(ids)) and 40 <= len(ids) <= 60
    for variant, setup in G.ITEMS:
        row = G.MATRIX[variant]
        assert setup in G.SETUPS and row["env"].keys().isdisjoint(G.SETUPS[setup][0].keys())
        spec = G.child_spec(variant, setup, "x.npz")
        got = [W.input_id(i) for i in spec["inputs"]]
        assert len(got) == len(set(got)) and got[:len(G.STANDARD)] == [W.input_id(i) for i in G.STANDARD]
        json.dumps(spec)
        env = G.child_env(variant, setup)
        assert env["CF_DEBUG_KNOBS"] == "1" and all(env[k] == v for k, v in row["env"].items())
        if "walk3_from" in row["spec"]:
            assert setup in G.MATRIX[row["spec"]["walk3_from"]]["setups"]
    assert G.T >= 60 and G.T >= 10 * G.MEASURED_DEFAULT_S
    # a stray knob or the suite-wide switch in the parent's environment does not reach a child
    os.environ["CF_WALK_V"], os.environ["CF_TEST_SMALL_RANGE_ROWS"] = "2", "4"
    try:
        env = G.child_env("default", "A")
    finally:
        del os.environ["CF_WALK_V"], os.environ["CF_TEST_SMALL_RANGE_ROWS"]
    assert "CF_WALK_V" not in env and "CF_TEST_SMALL_RANGE_ROWS" not in env


def test_worker_inputs_are_those_of_the_parity_tests():
    x = W.build_input(dict(kind="golden", arch="synth_small", name="pe_k1"))
    assert x["paired"] and x["kw"] == {"k": 1} and x["nq"] == 400 and len(x["off"]) == 801
    for i, (lengths, paired, k) in enumerate(common.EDGE_CASES):
        e = W.build_input(dict(kind="edge", idx=i))
        n = len(e["off"]) - 1
        assert e["kw"] == {"k": k} and e["paired"] == paired and e["nq"] == (n // 2 if paired else n) and len(e["seeds"]) == n
        lens = (e["off"][1:] - e["off"][:-1]).astype(int).tolist()
        assert lens[:len(lengths)] == lengths and 0 in lens and int(e["seq"].max()) == 4       # the boundary lengths; an empty read; reads with N
    r = W.build_input(dict(kind="replicated", copies=3))
    b = W.build_input(r["base"])
    assert r["nq"] == 3 * b["nq"] and sorted(r["perm"].tolist()) == sorted(list(range(b["nq"])) * 3)
    j = 2 * b["nq"] + 5
    i = int(r["perm"][j])
    assert np.array_equal(r["seq"][int(r["off"][j]):int(r["off"][j + 1])], b["seq"][int(b["off"][i]):int(b["off"][i + 1])]) and r["seeds"][j] == b["seeds"][i]


def test_worker_result_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    rows = np.zeros((7, 5), dtype=capi.ROW_DTYPE)
    rows["tax_id"] = rng.integers(0, 2 ** 62, (7, 5)); rows["taxon_idx"] = rng.integers(0, 30, (7, 5)); rows["score"] = rng.integers(0, 2 ** 32, (7, 5))
    n_rows = rng.integers(0, 6, 7).astype(np.uint32)
    rec = capi.LaunchRecord(search_form=4, rec_words=4, walk_version=2, passes=3).as_dict()
    assert rec["search_form"] == "planes-lazy1" and rec["passes"] == 3 and set(rec) == {f for f, _ in capi.LaunchRecord._fields_}
    meta = {"id": "x-A", "inputs": [{"id": "edge0", "info": {"row_passes": 2, "slow_post": 7}, "launch": rec, "ops": {f: i for i, f in enumerate(W.OPS)}}]}
    path = str(tmp_path / "r.npz")
    W.save_result(path, meta, {"in0.rows": rows, "in0.n_rows": n_rows, "in0.counts_reads": np.arange(31, dtype=np.uint64)})
    m2, a2 = W.load_result(path)
    assert m2 == meta and set(a2) == {"in0.rows", "in0.n_rows", "in0.counts_reads"}
    assert a2["in0.rows"].dtype == capi.ROW_DTYPE and np.array_equal(a2["in0.rows"], rows) and np.array_equal(a2["in0.n_rows"], n_rows)
    assert os.listdir(str(tmp_path)) == ["r.npz"]
    # the parent's tally of rows: per printed row a read, the only row of a query also a unique read, no row = taxon 0
    r = np.zeros((4, 2), dtype=capi.ROW_DTYPE)
    r["taxon_idx"] = [[3, 4], [3, 0], [9, 9], [5, 6]]
    a, u = G.tally(r, np.array([2, 1, 0, 2], dtype=np.uint32), 10)
    assert a.tolist() == [1, 0, 0, 2, 1, 1, 1, 0, 0, 0] and u.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert G.same_rows(r, np.array([2, 1, 0, 2]), r.copy(), np.array([2, 1, 0, 2])) and not G.same_rows(r, np.array([2, 1, 0, 2]), r, np.array([2, 1, 1, 2]))
