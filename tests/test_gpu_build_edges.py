"""The GPU index builder (cf_build_index) at tiny, boundary and non-default shapes (tests/buildcases.py) against the record of
the unmodified reference builder's output (tests/golden/build_edges.json: sizes and sha256 of the four files), and the
builder's prefix sum on its own (cf_debug_prim_scan) against numpy.  Indexes of at most 5,000 bases are also opened and read
back: the text out of the BWT, and every row resolved against the CPU restatement."""
import os

import numpy as np
import pytest

import buildcases as B
from centrifuge_amd import capi
from oracle import oracle as O
from test_gpu_build import _env

pytestmark = pytest.mark.gpu

READ_BACK_MAX = 5000


def _explain(c, d, ours):
    """with the compiled reference at hand: where the files differ"""
    if not O.have_ref():
        return "(no oracle/_ref here to locate the difference)"
    rd = os.path.join(d, "ref")
    B.run_reference(c, rd)
    return B.first_difference(os.path.join(rd, "idx"), ours)


def _read_back(c, ours):
    ix = capi.Index(ours, device=0)
    try:
        n = len(c.codes)
        assert ix.text_len == n
        packed = ix.restore()
        text = (packed[np.arange(n) // 4] >> (2 * (np.arange(n) % 4)).astype(np.uint8)) & 3
        assert np.array_equal(text, c.codes), "the text restored from the index is not the input"
        rows = np.arange(n + 1, dtype=np.uint64)
        orc = O.Oracle(ours)
        want = np.array([orc.L.cfo_resolve_row(orc.h, int(r)) for r in rows], dtype=np.uint32)
        orc.close()
        assert np.array_equal(ix.debug_resolve(rows), want)
    finally:
        ix.close()


@pytest.mark.parametrize("name", B.accepted_names())
def test_build_matches_the_recorded_reference(name, tmp_path):
    c, want = B.BY_NAME[name], B.load_golden()[name]["files"]
    d = str(tmp_path)
    tax = c.write(d)
    for via in c.vias:
        ours = os.path.join(d, "ours_" + via)
        src = dict(fasta=[os.path.join(d, "genomes.fa")]) if via == "fasta" else c.memory()
        with _env(**c.env):
            capi.build_index(ours, **src, **tax, **c.build_kwargs())
        got = B.index_digest(ours)
        if got != want:
            bad = [e for e in "1234" if got[e] != want[e]]
            raise AssertionError("%s via %s: .%s.cf differ from the reference's; %s" % (name, via, ",".join(bad), _explain(c, d, ours)))
        if len(c.codes) <= READ_BACK_MAX:
            _read_back(c, ours)


SCAN_N = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 524287, 524288, 524289, 1048577]


@pytest.mark.parametrize("n", SCAN_N)
def test_prim_scan_matches_cumsum(n):
    """device_scan<T, INCL> of cf_prims.hpp in the three forms the builder runs, exact, sums wrapping in the element's width"""
    rng = np.random.default_rng(n)
    last = np.zeros(n, dtype=np.uint32); last[-1] = 1
    inputs = {"ones": np.ones(n, dtype=np.uint32), "all_ff": np.full(n, 0xffffffff, dtype=np.uint32),
              "random": rng.integers(0, 1 << 32, n, dtype=np.uint32), "last_one": last}
    for nm, x in inputs.items():
        inc = np.cumsum(x, dtype=np.uint32)                                    # wraps modulo 2^32
        assert np.array_equal(capi.prim_scan(x, inclusive=True), inc), "u32 inclusive, " + nm
        assert np.array_equal(capi.prim_scan(x, inclusive=False), inc - x), "u32 exclusive, " + nm
    big = {"ones": np.ones(n, dtype=np.uint64), "random": rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
           "last_one": last.astype(np.uint64)}
    for nm, x in big.items():
        assert np.array_equal(capi.prim_scan(x, inclusive=False), np.cumsum(x, dtype=np.uint64) - x), "u64 exclusive, " + nm


def test_prim_scan_has_only_the_builders_forms():
    with pytest.raises(capi.CfError):
        capi.prim_scan(np.ones(8, dtype=np.uint64), inclusive=True)
