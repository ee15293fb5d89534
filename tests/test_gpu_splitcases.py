"""The device read splitter on the GPU at its edges: every batch of tests/splitcases.py — the table tests/test_split_emu.py puts
through the CPU harness, same batches, same seeds — through the tap cf_debug_split (include/centrifuge_amd.h), which launches
k_split_size / k_split_write with the code cf_batch_wait_text_split launches them with (enqueueSplit), the sinks, their sizes and
sums and the records' tally between filled margins that are read back.  Byte for byte against the contract's Python statement
(splitcases.contract), never against the CPU harness: every sink's text in its room (a query whose records do not fit is left
out, every other byte keeps the fill), the bytes sized whatever the room, the records, which sinks were sized at all."""
import pytest

import splitcases
from centrifuge_amd import capi
from splitcases import AL, PATTERNS, UN, make_batch

pytestmark = pytest.mark.gpu


def check(batch, rows, sinks, cap=None):
    splitcases.check(lambda b, s, c: capi.debug_split(b, s, cap=c), batch, rows, sinks, cap)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_split_matches_contract(paired, fastq, pattern):
    for nq in splitcases.COUNTS:
        batch, rows = make_batch(nq, PATTERNS[pattern], paired, fastq, seed=nq)
        check(batch, rows, UN | AL)
    if pattern == "unclassified":       # an empty sink is 0 bytes
        got = capi.debug_split(batch, UN | AL)
        assert got[2][:3] == (b"", 0, 0) and got[0][1] > 0


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("sinks", [0, UN, AL, UN | AL])
@pytest.mark.parametrize("nq", [70, 256 + 65])
def test_split_sink_subsets(paired, sinks, nq):
    batch, rows = make_batch(nq, PATTERNS["rows0125"], paired, True, seed=3 if nq == 70 else 4)
    check(batch, rows, sinks)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("trim", splitcases.TRIMS)
def test_split_trim_windows(fastq, trim):
    for paired in (False, True):
        batch, rows = make_batch(67, PATTERNS["rows0125"], paired, fastq, seed=5, trim5=trim[0], trim3=trim[1])
        check(batch, rows, UN | AL)


def test_split_room_too_small_leaves_the_rest_alone():
    batch, rows = make_batch(65, PATTERNS["alternating"], False, True, seed=2)
    check(batch, rows, UN | AL, cap=1000)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("lone", sorted(splitcases.LONE))
def test_split_one_classified_query_of_257(paired, lone):
    for fastq in (False, True):
        batch, rows = make_batch(257, splitcases.LONE[lone], paired, fastq, seed=6)
        check(batch, rows, UN | AL)
        check(batch, rows, AL)


def test_split_mates_of_one_base_and_250():
    batch, rows = splitcases.mate_extremes()
    assert sorted(set(zip(batch["rlen"][0::2], batch["rlen"][1::2]))) == [(1, 250), (250, 1)]
    for sinks in (UN | AL, UN):
        check(batch, rows, sinks)


@pytest.mark.parametrize("case", range(len(splitcases.room_cases())), ids=[c[0] for c in splitcases.room_cases()])
def test_split_rooms_smaller_than_the_text(case):
    _, batch, rows, sinks, caps = splitcases.room_cases()[case]
    check(batch, rows, sinks, cap=caps)


def test_the_tap_s_limits():
    """a sink bit that is none is CF_ERR_ARG; a batch without queries sizes its sinks and writes nothing"""
    batch, rows = make_batch(3, PATTERNS["alternating"], False, True, seed=1)
    with pytest.raises(capi.CfError):
        capi.debug_split(batch, 4)
    empty, none = make_batch(0, PATTERNS["alternating"], True, True, seed=1)
    assert capi.debug_split(empty, UN | AL) == [(b"", 0, 0, True)] * 4
    assert capi.debug_split(empty, 0) == [(b"", 0, 0, False)] * 4
