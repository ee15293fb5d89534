"""The read splitter of the device text path (split_size_body / split_write_body, centrifuge_amd/csrc/cf_textio.hpp) in the CPU harness
of tests/emu/emu_split.cpp — the one-lane build and wavefronts of 64 lanes — against the contract's Python statement
(tests/splitcases.py), byte for byte: synthetic FASTA (wrapped, lower case) and FASTQ blocks, unpaired reads and mates of unequal
lengths, the lengths at which the wave-wide copies change their way (dword phases, the 16-base and 32-base steps of the 2-bit
expansion), query counts around a wavefront and around a block of four, 0 .. 5 rows per query, every subset of the sinks, -5 / -3 windows and
rooms smaller than the text.  The batches and the check are those of tests/splitcases.py, which the device reads as well
(tests/test_gpu_splitcases.py)."""
import numpy as np
import pytest

import splitcases
from emu import emu_split

from splitcases import AL, PATTERNS, UN, make_batch


def check(batch, rows, sinks, wave64, cap=None):
    splitcases.check(lambda b, s, c: emu_split.split(b, s, wave64, cap=c), batch, rows, sinks, cap)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_split_matches_contract(wave64, paired, fastq, pattern):
    for nq in splitcases.COUNTS:
        batch, rows = make_batch(nq, PATTERNS[pattern], paired, fastq, seed=nq)
        check(batch, rows, UN | AL, wave64)
    if pattern == "unclassified":       # an empty sink is 0 bytes
        got = emu_split.split(batch, UN | AL, wave64)
        assert got[2][:3] == (b"", 0, 0) and got[0][1] > 0


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("sinks", [0, UN, AL, UN | AL])
def test_split_sink_subsets(wave64, paired, sinks):
    batch, rows = make_batch(70, PATTERNS["rows0125"], paired, True, seed=3)
    check(batch, rows, sinks, wave64)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("trim", splitcases.TRIMS)
def test_split_trim_windows(wave64, fastq, trim):
    for paired in (False, True):
        batch, rows = make_batch(67, PATTERNS["rows0125"], paired, fastq, seed=5, trim5=trim[0], trim3=trim[1])
        check(batch, rows, UN | AL, wave64)


def test_split_room_too_small_leaves_the_rest_alone():
    """records that do not fit the room they were promised are left out, nothing is written outside it"""
    batch, rows = make_batch(65, PATTERNS["alternating"], False, True, seed=2)
    for wave64 in (False, True):
        got = emu_split.split(batch, UN | AL, wave64, cap=1000)
        want = splitcases.contract(rows)
        for s, k in ((0, "un"), (2, "al")):
            text, n_bytes = got[s][0], got[s][1]
            assert n_bytes == len(want[k]) and len(text) == 1000
            whole = 0                                   # the records that lie wholly inside the room are there
            for row in rows:
                rec = splitcases.contract([row])[k]
                if whole + len(rec) > 1000:
                    break
                whole += len(rec)
            assert text[:whole] == want[k][:whole]
        check(batch, rows, UN | AL, wave64, cap=1000)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("sinks", [0, UN, AL, UN | AL])
def test_split_sink_subsets_over_a_block_and_a_tail(wave64, paired, sinks):
    batch, rows = make_batch(256 + 65, PATTERNS["rows0125"], paired, True, seed=4)
    check(batch, rows, sinks, wave64)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("lone", sorted(splitcases.LONE))
def test_split_one_classified_query_of_257(wave64, paired, lone):
    for fastq in (False, True):
        batch, rows = make_batch(257, splitcases.LONE[lone], paired, fastq, seed=6)
        check(batch, rows, UN | AL, wave64)
        check(batch, rows, AL, wave64)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
def test_split_mates_of_one_base_and_250(wave64):
    batch, rows = splitcases.mate_extremes()
    assert sorted(set(zip(batch["rlen"][0::2], batch["rlen"][1::2]))) == [(1, 250), (250, 1)]
    for sinks in (UN | AL, UN):
        check(batch, rows, sinks, wave64)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("case", range(len(splitcases.room_cases())), ids=[c[0] for c in splitcases.room_cases()])
def test_split_rooms_smaller_than_the_text(wave64, case):
    _, batch, rows, sinks, caps = splitcases.room_cases()[case]
    check(batch, rows, sinks, wave64, cap=caps)
