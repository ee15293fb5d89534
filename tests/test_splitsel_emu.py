"""The read splitter's size pass by a selection of taxa (split_sel_size_body, centrifuge_amd/csrc/cf_textio.hpp) with the write pass
it leaves alone (split_write_body), in the CPU harness of tests/emu/emu_splitsel.cpp — the one-lane build and wavefronts of 64
lanes — against the rule's Python statement (tests/splitselcases.py), byte for byte: query counts around a wavefront and a block
of four (where the records' sums over the wavefront and the lanes past the end can go wrong), 0, 1, 2, 5 and 63 rows per query,
unpaired reads and mates of unequal lengths, FASTA and FASTQ, every subset of the sinks, rooms smaller than the text, and the
selection "every taxon but 0" against today's splitter (tests/emu/emu_split.cpp).  The device reads the same batches
(tests/test_gpu_splitsel.py)."""
import pytest

import splitcases
import splitselcases
from emu import emu_split, emu_splitsel
from splitselcases import AL, MASKS, PATTERNS, UN, make_batch


def check(wave64, batch, rows, rows16, printed, mask, sinks, cap=None):
    return splitselcases.check(lambda b, r, m, s, c: emu_splitsel.split_taxa(b, r, m, s, wave64, cap=c), batch, rows, rows16, printed, mask, sinks, cap)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_selection_matches_the_rule(wave64, paired, mask):
    for nq in splitcases.COUNTS:
        b = make_batch(nq, PATTERNS["rows0_1_2_5_63"], paired, nq % 2 == 1, seed=nq)
        check(wave64, *b, MASKS[mask], UN | AL)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("pattern", ["unclassified", "classified", "alternating", "rows0125"])
def test_selection_over_the_splitter_s_own_patterns(wave64, pattern):
    for paired in (False, True):
        for fastq in (False, True):
            b = make_batch(130, PATTERNS[pattern], paired, fastq, seed=7 + paired)
            for mask in ("every-other", "only-zero", "first-row-only"):
                check(wave64, *b, MASKS[mask], UN | AL)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("sinks", [0, UN, AL, UN | AL])
def test_selection_sink_subsets(wave64, paired, sinks):
    b = make_batch(256 + 65, PATTERNS["rows0125"], paired, True, seed=4)
    for mask in ("every-other", "last-row-only"):
        check(wave64, *b, MASKS[mask], sinks)


def test_a_read_s_rows_go_both_ways():
    """the batches do hold what the rule is about: a query with rows in both classes, and every mask but `all` and `none` feeds both"""
    batch, rows, rows16, printed = make_batch(65, PATTERNS["rows0_1_2_5_63"], False, True, seed=65)
    mine = splitselcases.classed(rows, printed, MASKS["every-other"])
    both = 0
    for q_row in set(map(id, rows)):
        cls = {c for r, (_, _, _, c) in zip(rows, mine) if id(r) == q_row}
        both += len(cls) == 2
    assert both >= 10
    for name in ("only-zero", "all-but-zero", "every-other", "first-row-only", "last-row-only"):
        got = check(False, batch, rows, rows16, printed, MASKS[name], UN | AL)
        assert got[0][2] > 0 and got[2][2] > 0, name


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
def test_every_taxon_but_zero_is_today_s_split(wave64, paired):
    for nq in splitcases.COUNTS:
        batch, rows, rows16, printed = make_batch(nq, PATTERNS["rows0_1_2_5_63"], paired, True, seed=nq)
        for sinks in (UN | AL, AL):
            assert emu_splitsel.split_taxa(batch, rows16, MASKS["all-but-zero"], sinks, wave64) == emu_split.split(batch, sinks, wave64)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
def test_rooms_smaller_than_the_text(wave64, paired):
    """nothing is written outside a room, the bytes sized do not depend on it, a query's records in a sink fit or stay out together:
    rooms cut inside a query's records, on a boundary between two queries, a byte short, none"""
    b = make_batch(130, PATTERNS["rows0125"], paired, True, seed=31 + paired)
    full = check(wave64, *b, MASKS["every-other"], UN | AL)
    sizes = [full[s][1] for s in range(4)]
    assert all(sizes[s] > 2000 for s in range(4) if full[s][3])
    for caps in ([1000] * 4, [n - 1 if n else 0 for n in sizes], [n // 2 for n in sizes], [0] * 4, [sizes[0], 0, 777, sizes[3]]):
        check(wave64, *b, MASKS["every-other"], UN | AL, cap=caps)
    # ... and on a boundary between two queries of sink 0
    batch, rows, rows16, printed = b
    mine = splitselcases.classed(rows, printed, MASKS["every-other"])
    key = splitselcases.sink_keys(paired)[0]
    at, i, cuts = 0, 0, []
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j] is rows[i]:
            j += 1
        at += len(splitcases.contract(mine[i:j])[key])
        cuts.append(at)
        i = j
    check(wave64, *b, MASKS["every-other"], UN | AL, cap=[cuts[len(cuts) // 2], 1 << 22, 1 << 22, 1 << 22])


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
def test_mates_of_one_base_and_250(wave64):
    b = make_batch(67, PATTERNS["rows0125"], True, True, seed=8, length_of=lambda r: (1, 250, 250, 1)[r % 4])
    for mask in ("every-other", "first-row-only"):
        check(wave64, *b, MASKS[mask], UN | AL)
