"""cf_split_taxa_mask (include/centrifuge_amd.h) — the table --split-taxids looks a row's taxon up in — on the golden indexes, opened
on the host only, against the closure computed here from what the project's `centrifuge-inspect --taxonomy-tree` and
`--conversion-table` print: a dense taxon's byte is 1 when the taxon or a node of its parent chain is listed, a taxon the tree
lacks only when it is listed itself, and the byte behind the last taxon's is taxID 0's."""
import functools
import os
import subprocess

import numpy as np
import pytest

import common
from centrifuge_amd import capi

INSPECT = os.path.join(os.path.dirname(capi.LIB_PATH), "bin", "centrifuge-inspect-bin")
INDEXES = ("synth_small", "example")


@functools.lru_cache(maxsize=None)
def world(name):
    """the index (host only), its dense taxa, the tree as the inspector prints it (tid -> parent) and the references' taxIDs"""
    base = os.path.join(common.golden(name)[0], "idx")
    ix = capi.Index(base, host_only=True)
    parent = {}
    for ln in subprocess.run([INSPECT, "--taxonomy-tree", base], capture_output=True, text=True, check=True).stdout.splitlines():
        tid, par = ln.split("\t|\t")[:2]
        parent[int(tid)] = int(par)
    refs = {int(ln.split("\t")[1]) for ln in subprocess.run([INSPECT, "--conversion-table", base], capture_output=True, text=True, check=True).stdout.splitlines()}
    return ix, [int(t) for t in ix.taxon_ids()], parent, refs


def closure(taxa, parent, listed):
    """the rule, on the inspector's tree"""
    listed, out = set(listed), []
    for t in taxa:
        sel, steps = False, 0
        while True:
            if t in listed:
                sel = True
                break
            if t not in parent or parent[t] == t or parent[t] == 0 or t == 1:
                break
            t, steps = parent[t], steps + 1
            assert steps < 4096
        out.append(int(sel))
    return np.array(out + [int(0 in listed)], dtype=np.uint8)


def pick(name):
    """a leaf of the tree, an internal taxon with descendants, an ID the index does not know"""
    _, taxa, parent, _ = world(name)
    inner = {p for t, p in parent.items() if p != t}
    leaf = max(t for t in parent if t not in inner)
    internal = max((t for t in inner if t > 1), key=lambda t: (sum(1 for x in parent if parent[x] == t), t))
    unknown = max(taxa) + 12345
    return leaf, internal, unknown


@pytest.mark.parametrize("name", INDEXES)
@pytest.mark.parametrize("what", ["leaf", "internal", "root", "zero", "unknown", "duplicate", "leaf+zero", "nothing"])
def test_mask_is_the_closure_on_the_inspector_s_tree(name, what):
    ix, taxa, parent, _ = world(name)
    leaf, internal, unknown = pick(name)
    listed = {"leaf": [leaf], "internal": [internal], "root": [1], "zero": [0], "unknown": [unknown, leaf, unknown],
              "duplicate": [internal, leaf, internal, internal], "leaf+zero": [leaf, 0], "nothing": [unknown]}[what]
    mask, n_unknown = capi.split_taxa_mask(ix, listed)
    want = closure(taxa, parent, listed)
    assert mask.dtype == np.uint8 and len(mask) == ix.num_taxa + 1
    assert np.array_equal(mask, want), [(t, int(a), int(b)) for t, a, b in zip(taxa + [0], mask, want) if a != b]
    assert n_unknown == (1 if what in ("unknown", "nothing") else 0)        # (an ID counts once, and selects nothing)
    sel = {t for t, m in zip(taxa, mask[:-1]) if m}
    if what == "leaf":
        assert sel == {leaf} and not mask[-1]
    elif what == "internal":
        assert internal in sel and len(sel) > 1 and 1 not in sel and 0 not in sel
    elif what == "root":
        assert sel == set(parent) and not mask[-1] and not mask[taxa.index(0)]
    elif what == "zero":
        assert sel == {0} and mask[-1] == 1
    elif what == "unknown":
        assert np.array_equal(mask, capi.split_taxa_mask(ix, [leaf])[0])
    elif what == "duplicate":
        assert np.array_equal(mask, capi.split_taxa_mask(ix, [leaf, internal])[0])
    elif what == "nothing":
        assert not mask.any()


@pytest.mark.parametrize("name", INDEXES)
def test_every_taxon_on_its_own(name):
    ix, taxa, parent, _ = world(name)
    for t in taxa:
        mask, n_unknown = capi.split_taxa_mask(ix, [t])
        assert n_unknown == 0 and np.array_equal(mask, closure(taxa, parent, [t])), t
    mask, n_unknown = capi.split_taxa_mask(ix, [])
    assert n_unknown == 0 and not mask.any()


@pytest.mark.parametrize("name", INDEXES)
def test_a_reference_s_taxid_outside_the_tree_is_selected_only_by_itself(name):
    ix, taxa, parent, refs = world(name)
    outside = sorted(t for t in refs if t not in parent and t != 0)
    if not outside:
        pytest.skip("every reference of the golden index %s carries a taxID that is a node of its tree" % name)
    t = outside[0]
    assert t in taxa
    assert capi.split_taxa_mask(ix, [t])[0][taxa.index(t)] == 1
    assert capi.split_taxa_mask(ix, [1])[0][taxa.index(t)] == 0
