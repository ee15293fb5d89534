"""The read splitter by a selection of taxa on the GPU (k_split_sel_size in front of the sums and k_split_write; --split-taxids).
The batches of tests/splitselcases.py — those of the CPU harness, tests/test_splitsel_emu.py — through the tap cf_debug_split_taxa,
which launches the kernels with the code cf_batch_wait_text_split launches them with, every buffer they write between filled margins
that are read back; and the slot ABI on synth_small: a block up as text, classified, cf_classifier_set_split_taxa, the four sinks
against the contract applied to the rows the batch itself printed.  Byte for byte against the rule's Python statement, never
against the CPU harness."""
import os

import numpy as np
import pytest

import common
import splitcases
import splitselcases
from centrifuge_amd import capi
from splitselcases import AL, MASKS, PATTERNS, UN, make_batch
from test_async_abi import dev_index
from test_gpu_split import inflate_members, parse_reads

pytestmark = pytest.mark.gpu


def check(batch, rows, rows16, printed, mask, sinks, cap=None):
    return splitselcases.check(lambda b, r, m, s, c: capi.debug_split_taxa(b, r, m, s, cap=c), batch, rows, rows16, printed, mask, sinks, cap)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_selection_matches_the_rule(paired, mask):
    for nq in splitcases.COUNTS:
        b = make_batch(nq, PATTERNS["rows0_1_2_5_63"], paired, nq % 2 == 1, seed=nq)
        check(*b, MASKS[mask], UN | AL)


@pytest.mark.parametrize("pattern", ["unclassified", "classified", "alternating", "rows0125"])
def test_selection_over_the_splitter_s_own_patterns(pattern):
    for paired in (False, True):
        for fastq in (False, True):
            b = make_batch(130, PATTERNS[pattern], paired, fastq, seed=7 + paired)
            for mask in ("every-other", "only-zero", "first-row-only"):
                check(*b, MASKS[mask], UN | AL)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("sinks", [0, UN, AL, UN | AL])
def test_selection_sink_subsets(paired, sinks):
    b = make_batch(256 + 65, PATTERNS["rows0125"], paired, True, seed=4)
    for mask in ("every-other", "last-row-only"):
        check(*b, MASKS[mask], sinks)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
def test_every_taxon_but_zero_is_today_s_split(paired):
    for nq in (65, 257):
        batch, rows, rows16, printed = make_batch(nq, PATTERNS["rows0_1_2_5_63"], paired, True, seed=nq)
        for sinks in (UN | AL, AL):
            assert capi.debug_split_taxa(batch, rows16, MASKS["all-but-zero"], sinks) == capi.debug_split(batch, sinks)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
def test_rooms_smaller_than_the_text(paired):
    b = make_batch(130, PATTERNS["rows0125"], paired, True, seed=31 + paired)
    full = check(*b, MASKS["every-other"], UN | AL)
    sizes = [full[s][1] for s in range(4)]
    for caps in ([1000] * 4, [n - 1 if n else 0 for n in sizes], [n // 2 for n in sizes], [0] * 4, [sizes[0], 0, 777, sizes[3]]):
        check(*b, MASKS["every-other"], UN | AL, cap=caps)


def test_mates_of_one_base_and_250():
    b = make_batch(67, PATTERNS["rows0125"], True, True, seed=8, length_of=lambda r: (1, 250, 250, 1)[r % 4])
    check(*b, MASKS["every-other"], UN | AL)


def test_the_tap_s_limits():
    batch, rows, rows16, printed = make_batch(3, PATTERNS["alternating"], False, True, seed=1)
    with pytest.raises(capi.CfError):
        capi.debug_split_taxa(batch, rows16, MASKS["all"], 4)
    empty = make_batch(0, PATTERNS["alternating"], True, True, seed=1)
    assert capi.debug_split_taxa(empty[0], empty[2], MASKS["all"], UN | AL) == [(b"", 0, 0, True)] * 4


# ---- the slot ABI
@pytest.fixture(scope="module")
def world():
    ix = dev_index("synth_small")
    clf = capi.Classifier(ix)
    yield ix, clf
    clf.close()


def rows_by_selection(text, reads, dense, mask):
    """the rows a batch printed (default columns, no header) and the input's reads -> what splitcases.contract reads, each row classed
    by the mask entry of its taxID column"""
    rows, q, left = [], 0, 0
    for ln in text.split(b"\n"):
        if not ln:
            continue
        f = ln.split(b"\t")
        if left == 0:
            left = int(f[-1])
        seq, qual = reads[0][q]
        if len(reads) == 2:
            seq, qual = seq + b"_" + reads[1][q][0], qual + b"_" + reads[1][q][1]
        unclassified = f[1] == b"unclassified"
        rows.append((f[0], seq, qual, bool(mask[-1] if unclassified else mask[dense[int(f[2])]])))
        left -= 1
        if left == 0:
            q += 1
    assert q == len(reads[0])
    return rows


@pytest.mark.parametrize("name,tfmt", [("k5", capi.TEXT_FASTA), ("fastq", capi.TEXT_FASTQ), ("pe_k5", capi.TEXT_FASTA)], ids=["k5", "fastq", "pe_k5"])
def test_slot_sinks_follow_the_selection_and_come_back_without_it(world, name, tfmt):
    ix, clf = world
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    texts = [open(os.path.join(d, f), "rb").read() for f in c["reads"]]
    paired = len(texts) == 2
    reads = [parse_reads(t, tfmt == capi.TEXT_FASTQ) for t in texts]
    golden = open(os.path.join(d, c["tsv"]), "rb").read().split(b"\n", 1)[1]
    taxa = [int(t) for t in ix.taxon_ids()]
    dense = {t: i for i, t in enumerate(taxa)}
    names = splitcases.SINKS_PAIRED if paired else splitcases.SINKS_UNPAIRED
    slot = capi.Slot(clf)
    slot.set_result_format(capi.RESULTS_NARROW)
    slot.set_text_split(capi.SPLIT_UN | capi.SPLIT_AL)

    def run(bgzf=False):
        slot.set_text_split(capi.SPLIT_UN | capi.SPLIT_AL, bgzf)
        assert not slot.submit_text(texts[0], tfmt, text2=texts[1] if paired else None).irregular
        text = slot.wait_text()[0]
        assert text == golden                                        # the rows never depend on the selection
        got = slot.wait_text_split()
        assert slot.launch_record()["split_sinks"] == sum(1 << s for s in names.values())
        return text, [(inflate_members(g[0]) if bgzf else g[0], g[1], g[2]) for g in got]

    _, today = run()
    assert not slot.split_by_taxa()
    # 100: a genus with species below it; 1008: a species; 0: the reads without an assignment; an ID no index knows
    for listed, n_unknown in (([100], 0), ([1008], 0), ([0], 0), ([0, 101, 1000], 0), ([100, 4000000000], 1), ([4000000000], 1)):
        assert clf.set_split_taxa(listed) == n_unknown
        mask = capi.split_taxa_mask(ix, listed)[0]
        for bgzf in (False, True):
            text, got = run(bgzf)
            assert slot.split_by_taxa()
            want = splitcases.contract(rows_by_selection(text, reads, dense, mask))
            for k, s in names.items():
                assert got[s][0] == want[k], (listed, k, bgzf)
                assert got[s][1] == len(want[k]) and got[s][2] == want[k].count(b"\n") // 4
            for s in range(4):
                if s not in names.values():
                    assert got[s] == (b"", 0, 0)
        if listed == [100]:
            assert all(want[k] for k in names), "the selection should feed every sink"
        if listed == [4000000000]:
            assert not any(want[k] for k in names if k.startswith("al"))
    # every taxon but 0: today's bytes; and the selection dropped: today's launches and bytes again
    assert clf.set_split_taxa([t for t in taxa if t != 0]) == 0
    assert run()[1] == today and slot.split_by_taxa()
    assert clf.set_split_taxa([]) == 0
    assert run()[1] == today and not slot.split_by_taxa()
    slot.close()


def test_the_getter_needs_a_split_wait(world):
    ix, clf = world
    slot = capi.Slot(clf)
    with pytest.raises(capi.CfError, match="cf_batch_wait_text_split"):
        slot.split_by_taxa()
    slot.close()
