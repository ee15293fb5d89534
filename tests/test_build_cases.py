"""The index builder's corner cases (tests/buildcases.py) without a device: every case still sits on the edge it is there for,
and the record of the reference builder's output (tests/golden/build_edges.json) is what the compiled reference writes."""
import numpy as np
import pytest

import buildcases as B
from centrifuge_amd import capi
from oracle import oracle as O


@pytest.mark.parametrize("name", B.NAMES)
def test_case_has_its_property(name, tmp_path):
    """lengths and text through the builder's own ingest (cf_build_describe), '$' rows through the brute-force suffix array"""
    c = B.BY_NAME[name]
    c.write(str(tmp_path))
    forms = []
    if "fasta" in c.vias:
        forms.append(capi.build_describe(fasta=[str(tmp_path / "genomes.fa")]))
    if "memory" in c.vias:
        assert not c.has_gaps
        forms.append(capi.build_describe(**c.memory()))
    for d in forms:
        assert d["len"] == c.n == len(c.codes)
        assert np.array_equal(d["text"], c.codes)
        assert list(d["rstarts"][:, 0][np.unique(d["rstarts"][:, 1], return_index=True)[1]]) == c.starts()
    assert c.claim(c), "the case has drifted off its edge"


def test_brute_force_suffix_array_orders_the_terminator_last():
    """ACA: the terminator sorts after T, so ACA$ < A$ < CA$ < $ and '$' stands in row 0 (with '$' first it would be row 2)"""
    assert list(B.suffix_array(np.array([0, 1, 0]))) == [0, 2, 1, 3] and B.z_off(np.array([0, 1, 0])) == 0
    assert list(B.suffix_array(np.array([3, 3]))) == [0, 1, 2]                  # TT$ < T$ < $
    assert B.max_bin12(np.zeros(20, dtype=np.uint8)) == 9                       # AAAAAAAAAAAA at positions 0 .. 8
    assert B.tied_slots(np.zeros(40, dtype=np.uint8)) == 12                     # 29 A: positions 0 .. 11


def test_record_covers_every_case():
    """one record per case, made from the inputs the table generates today; only the cases that may be refused are"""
    g = B.load_golden()
    assert sorted(g) == sorted(B.NAMES)
    for c in B.CASES:
        r = g[c.name]
        assert r["fasta_sha256"] == c.fasta_sha256(), "%s: the generator has changed, regenerate the record" % c.name
        assert r["args"] == c.ref_args
        assert r["exit"] == 0 or c.may_refuse, c.name
        assert (r["exit"] == 0) == ("files" in r)


@pytest.mark.skipif(not O.have_ref(), reason="needs oracle/_ref")
@pytest.mark.parametrize("name", B.NAMES)
def test_reference_reproduces_build_golden(name, tmp_path):
    assert B.run_reference(B.BY_NAME[name], str(tmp_path)) == B.load_golden()[name]
