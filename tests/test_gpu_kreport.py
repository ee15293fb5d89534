"""The Kraken-style report's tally on the GPU (cf_kreport_enable / _get / _reset / _write through capi.py): the golden synth_small
reads through a slot of a classifier with the tally on — write_kreport against centrifuge-kreport on the same rows as a TSV,
kreport_counts against kreport_body in the CPU harness over the same rows; two batches of unequal size against one; the reset."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common
from centrifuge_amd import capi, reads
from emu import emu_kreport as K
from test_async_abi import dev_index, load_case

pytestmark = pytest.mark.gpu
KREPORT = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-kreport")
_tab = {}


def index_table(arch):
    if arch not in _tab:
        _tab[arch] = K.index_table(os.path.join(common.golden(arch)[0], "idx"))
    return _tab[arch]


def classify(slot, seq, off, seeds, paired, lo, hi):
    """queries [lo, hi) through the slot -> rows (k per query), n_rows, score2"""
    m = 2 if paired else 1
    o = off[lo * m:hi * m + 1]
    b, msk, ln = capi.pack_reads(seq[int(o[0]):int(o[-1])], o - o[0])
    slot.submit(b, msk, ln, np.ascontiguousarray(seeds[lo * m:hi * m], dtype=np.uint32), paired=paired)
    rows, first, n_rows, score2, _, _ = slot.wait()
    return capi.unpack_rows(rows, first, n_rows, slot.clf.params.khits), n_rows, score2


@pytest.mark.parametrize("name", ["k5", "pe_k5", "fastq"])
def test_kreport_of_the_golden_reads(name):
    d, c, kw, nm, ql, seq, off, seeds, paired = load_case("synth_small", name)
    ix = dev_index("synth_small")
    taxa, tab = index_table("synth_small")
    assert len(taxa) == ix.num_taxa
    clf = capi.Classifier(ix, **kw)
    with pytest.raises(capi.CfError):
        clf.kreport_counts()                                     # not enabled yet
    clf.enable_kreport()
    clf.enable_kreport()                                         # (a second call changes nothing)
    slot = capi.Slot(clf)
    nq = len(nm)
    rows, n_rows, score2 = classify(slot, seq, off, seeds, paired, 0, nq)
    got, n = clf.kreport_counts()
    # the CPU harness over the same rows
    k = clf.params.khits
    tidx = np.searchsorted(taxa, rows["tax_id"].astype(np.uint64)).astype(np.uint32).reshape(nq, k)
    want, _, _ = K.tally(tab, n_rows, tidx)
    assert n == nq == int(want[-1]) and np.array_equal(got, want[:-1])
    assert int(got.sum()) == nq
    # what the case shows beyond count_body's work: unclassified reads, and LCAs that are none of their rows' taxa
    inner = sum(1 for q in range(nq) if n_rows[q] > 1 and _fold(tab, tidx[q, :n_rows[q]]) not in set(tidx[q, :n_rows[q]].tolist()))
    assert inner >= 10 and int(got[0]) >= 1 and int((n_rows == 0).sum()) == int(got[0]), (inner, int(got[0]))
    # write_kreport against centrifuge-kreport on the rows as a TSV (readIDs r0, r1, ...)
    with tempfile.TemporaryDirectory() as t:
        tsv, out = os.path.join(t, "o.tsv"), os.path.join(t, "k.txt")
        open(tsv, "w").write(reads.format_tsv(ix.seqid, [b"r%d" % i for i in range(nq)], ql, rows, n_rows, score2))
        clf.write_kreport(out)
        ref = subprocess.run([KREPORT, "-x", os.path.join(d, "idx"), tsv], capture_output=True)
        assert ref.returncode == 0 and ref.stdout.count(b"\n") > 3
        assert open(out, "rb").read() == ref.stdout
    # the reset, then the same reads in two batches of unequal size
    clf.reset_kreport()
    z, n0 = clf.kreport_counts()
    assert n0 == 0 and not z.any()
    cut = nq // 3 + 1
    classify(slot, seq, off, seeds, paired, 0, cut)
    part, n1 = clf.kreport_counts()
    assert n1 == cut and int(part.sum()) == cut
    classify(slot, seq, off, seeds, paired, cut, nq)
    both, n2 = clf.kreport_counts()
    assert n2 == nq and np.array_equal(both, got)
    assert slot.kreport_ms() >= 0
    slot.close(); clf.close()


def _fold(tab, idx):
    acc = 0
    for t in idx.tolist():
        acc = K.lca(tab, acc, t)
    return acc


def test_a_classifier_without_the_tally_is_untouched():
    d, c, kw, nm, ql, seq, off, seeds, paired = load_case("synth_small", "k5")
    ix = dev_index("synth_small")
    clf = capi.Classifier(ix, **kw)
    slot = capi.Slot(clf)
    classify(slot, seq, off, seeds, paired, 0, len(nm))
    assert slot.kreport_ms() == 0
    with pytest.raises(capi.CfError):
        clf.reset_kreport()
    slot.close(); clf.close()
