"""The Kraken-style report's tally in the CPU harness (tests/emu/emu_kreport.cpp), both widths: lca_body over the host's table
against a restatement of centrifuge-kreport's lca behind its inTree rule, for every pair of taxa of small trees — ill-formed ones
among them —, and kreport_body against a per-read fold: every row count and both places rows lie in, windows, direct slots, the
hash with probes that run out (far atomics), two chunks."""
import numpy as np
import pytest

from emu import emu_kreport as K

WIDTHS = [False, True]


# ---- centrifuge-kreport's own rules (inTree, lca), on taxon ids
class Tree:
    def __init__(self, nodes):
        self.parent = {}
        for t, p in nodes:
            self.parent[t] = 0 if t == 1 else p

    def in_tree(self, a):
        while a > 1:
            if a not in self.parent:
                return False
            p = self.parent[a]
            if a == p:
                break
            a = p
        return True

    def lca(self, a, b):
        if a == 0:
            return b
        if b == 0:
            return a
        if a == b:
            return a
        path = set()
        while a != 0:
            path.add(a)
            if a not in self.parent:
                break
            p = self.parent[a]
            if a == p:
                break
            a = p
        while b > 1:
            if b in path:
                return b
            if b not in self.parent:
                break
            p = self.parent[b]
            if b == p:
                break
            b = p
        return 1

    def fold(self, tids):
        acc = 0
        for t in tids:
            acc = self.lca(acc, t if self.in_tree(t) else 1)
        return acc


def dense(nodes, extra=()):
    return sorted({0, 1} | {t for t, _ in nodes} | set(extra))


def chain(n, first=2, root=1):
    """root <- first <- first+1 ..."""
    return [(first + i, root if i == 0 else first + i - 1) for i in range(n)]


BUSH = [(1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (6, 4), (7, 4), (8, 5), (9, 3), (10, 9), (11, 9), (12, 10)]
TREES = {
    "chain": ([(1, 1)] + chain(9), ()),
    "bush": (BUSH, ()),
    # depths that differ by more than 64: a chain of 150 under 2, a leaf under 3
    "deep": ([(1, 1), (2, 1), (3, 1), (500, 3)] + chain(150, first=10, root=2), ()),
    # a parent missing in mid-chain (23's parent 22 is no node): 23, 24 and 25 are outside the tree
    "gap": (BUSH + [(21, 2), (23, 22), (24, 23), (25, 24)], ()),
    # a second self-parented root with a subtree of its own, and a node whose parent is 0
    "two_roots": (BUSH + [(40, 40), (41, 40), (42, 40), (43, 41), (50, 0), (51, 50)], ()),
    # taxon 1 is no node; 30 is a taxon of the index (a sequence's) that the tree does not hold
    "no_one": ([(2, 1), (3, 1), (4, 2), (5, 2), (6, 4), (9, 3)], (30,)),
}


@pytest.mark.parametrize("wave64", WIDTHS)
@pytest.mark.parametrize("name", sorted(TREES))
def test_lca_of_every_pair(name, wave64):
    nodes, extra = TREES[name]
    taxa = dense(nodes, extra)
    tab = K.table(nodes, taxa, wave64)
    tree = Tree(nodes)
    idx = {t: i for i, t in enumerate(taxa)}
    outside = [t for t in taxa if not tree.in_tree(t)]
    if name == "gap":
        assert outside == [23, 24, 25]
    if name == "no_one":
        assert outside == [30]
    for a in taxa:
        for b in taxa:
            want = tree.lca(a if tree.in_tree(a) else 1, b if tree.in_tree(b) else 1)
            assert taxa[K.lca(tab, idx[a], idx[b], wave64)] == want, (name, a, b)
    if name == "two_roots":
        assert tree.lca(43, 42) == 40 and tree.lca(43, 6) == 1 and tree.lca(51, 50) == 50 and tree.lca(51, 43) == 1
    if name == "deep":
        assert tree.lca(159, 500) == 1 and tree.lca(159, 20) == 20


@pytest.mark.parametrize("wave64", WIDTHS)
def test_a_cycle_is_refused(wave64):
    for nodes in ([(1, 1), (2, 1), (5, 6), (6, 7), (7, 5)], [(1, 1)] + chain(4100)):
        with pytest.raises(K.Refused, match=r"taxonomy tree is deeper than 4096 levels \(a cycle\?\)"):
            K.table(nodes, dense(nodes), wave64)
    K.table([(1, 1)] + chain(4096), dense([(1, 1)] + chain(4096)), wave64)          # 4,096 levels are accepted


# ---- kreport_body
def case(nodes, extra, nq, k, seed, n_rows_of=None):
    """nq queries with every row count the issue names spread over them -> table, taxa, tree, n_out, rows"""
    L = K.lib()
    F = L.emu_kreport_field_rows()
    taxa = dense(nodes, extra)
    rng = np.random.default_rng(seed)
    pick = [0, 1, 2, F, F + 1, k] + list(range(3, k))
    n_out = np.array([pick[q % len(pick)] if n_rows_of is None else n_rows_of(q) for q in range(nq)], dtype=np.uint32)
    rows = rng.integers(0, len(taxa), size=(nq, k), dtype=np.uint32)
    rows[rng.random((nq, k)) < 0.05] = 0                      # rows of taxon 0 (lca(0, b) = b inside the fold)
    return taxa, n_out, rows


def want_counts(tree, taxa, n_out, rows, q_lo, q_hi):
    want = np.zeros(len(taxa) + 1, dtype=np.uint64)
    idx = {t: i for i, t in enumerate(taxa)}
    for q in range(q_lo, q_hi):
        want[idx[tree.fold([taxa[r] for r in rows[q, :n_out[q]]])]] += 1
        want[len(taxa)] += 1
    return want


@pytest.mark.parametrize("wave64", WIDTHS)
def test_tally_direct_slots_row_counts_and_windows(wave64):
    nodes, extra = TREES["gap"]
    F = K.lib().emu_kreport_field_rows()
    taxa, n_out, rows = case(nodes, extra, 700, 63, 1)
    assert {0, 1, 2, F, F + 1, 63} <= set(n_out.tolist())
    tab, tree = K.table(nodes, taxa, wave64), Tree(nodes)
    assert len(taxa) <= 1 << K.lib().emu_kreport_slot_bits()
    for q_lo, q_hi in ((0, 700), (37, 700), (0, 611), (129, 130), (300, 300)):
        got, lds, blocks = K.tally(tab, n_out, rows, q_lo, q_hi, wave64=wave64)
        want = want_counts(tree, taxa, n_out, rows, q_lo, q_hi)
        assert np.array_equal(got, want), (q_lo, q_hi)
        assert np.array_equal(lds, want[:-1]) and blocks == 1       # direct slots: nothing takes the far atomics
    # some LCA is none of its read's rows' taxa, some read counts under taxon 1 for a row outside the tree
    inner = sum(1 for q in range(700) if n_out[q] and tree.fold([taxa[r] for r in rows[q, :n_out[q]]]) not in {taxa[r] for r in rows[q, :n_out[q]]})
    assert inner > 50


@pytest.mark.parametrize("wave64", WIDTHS)
@pytest.mark.parametrize("chunk", [None, 256])
def test_tally_hash_slots_run_out_and_two_chunks(chunk, wave64):
    """four slots, 8 probes: at most four taxa of a block live in LDS, the others take the far atomics; chunk 256: two blocks"""
    nodes = [(1, 1)] + [(t, 1) for t in range(2, 12)] + [(100 + t, t) for t in range(2, 12)] + [(200 + t, 100 + t) for t in range(2, 12)]
    taxa, n_out, rows = case(nodes, (), 400, 7, 2, n_rows_of=lambda q: (1, 1, 2, 5, 0, 7, 1)[q % 7])
    tab, tree = K.table(nodes, taxa, wave64), Tree(nodes)
    assert len(taxa) > 4
    for q_lo, q_hi in ((0, 400), (100, 390)):
        got, lds, blocks = K.tally(tab, n_out, rows, q_lo, q_hi, chunk=chunk, slot_bits=2, wave64=wave64)
        want = want_counts(tree, taxa, n_out, rows, q_lo, q_hi)
        assert np.array_equal(got, want), (q_lo, q_hi)
        assert blocks == (1 if chunk is None else 2)
        far = want[:-1] - lds
        assert (lds <= want[:-1]).all()
        assert (far > 0).sum() >= 1 and (lds > 0).sum() >= 1, "one taxon at least through the far atomics, one through LDS"
        assert (lds > 0).sum() <= 4 * blocks


@pytest.mark.parametrize("wave64", WIDTHS)
def test_tally_hash_slots_that_suffice(wave64):
    nodes, extra = TREES["two_roots"]
    taxa, n_out, rows = case(nodes, extra, 300, 9, 3)
    tab, tree = K.table(nodes, taxa, wave64), Tree(nodes)
    got, lds, _ = K.tally(tab, n_out, rows, slot_bits=4, wave64=wave64)         # 16 slots for 20 taxa: the hash, mostly without overflow
    assert len(taxa) > 16
    want = want_counts(tree, taxa, n_out, rows, 0, 300)
    assert np.array_equal(got, want)
    # 20 taxa in 16 slots: four taxa at the least find no slot and take the far atomics, the others the LDS path
    far = want[:-1] - lds
    assert (lds <= want[:-1]).all() and (far > 0).sum() >= 1 and (lds > 0).sum() >= 1
