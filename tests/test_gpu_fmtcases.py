"""The device formatter on the GPU at its edges: every case of tests/fmtcases.py — the table tests/test_textcols_emu.py puts through
the CPU harness, same batches, same seeds — through the tap cf_debug_format (include/centrifuge_amd.h), which launches k_fmt_size /
k_fmt_write and k_fmt_cols_size / k_fmt_cols_write with the code cf_batch_wait_text launches them with (enqueueFormat), every
device buffer the kernels write between filled margins that are read back.  What hardware alone shows is here: the LDS stage
behind its compiler fence, the stage a wavefront picks inside a block of four, the cross-lane copies of the long fields, the
ballot loop around the tally's atomics.  Everything is compared byte for byte with the plain Python statements of the table
(expected_rows, tally), never with the CPU harness's output: the text in its room (rows that do not fit are left out, every other
byte keeps the fill), the bytes per query, their sum whatever the room, the perfect single assignments, the tuples in any order.
A tap call that fails — a limit, a changed margin — fails the test with cf_last_error."""
import numpy as np
import pytest

import fmtcases
from centrifuge_amd import capi
from emu import emu_cols
from fmtcases import BODIES, DEFAULT, LENGTHS, LIST_A, LIST_B, PROGRAMS, QUAL, READ_ID, SAM, SEQ, WORLD, expected, make_batch, split_tuples

pytestmark = pytest.mark.gpu


def run(W, b, cols, bodies, cap, tcap):
    return capi.debug_format(W, b, [] if bodies else cols, cap, tcap)


def check(b, cols, tally=None):
    want = fmtcases.check(run, b, cols)
    if tally is not None:
        # the tally does not depend on the columns: what the default eight's own kernels leave on the same rows (the tuples in any order)
        _, _, _, single, tuples, _ = run(WORLD, b, cols, False, len(want), None)
        assert np.array_equal(single, tally[0])
        assert sorted(split_tuples(tuples)) == sorted(split_tuples(tally[1]))
    return want


def default_tally(b):
    text = fmtcases.check(run, b, BODIES)
    _, _, _, single, tuples, _ = run(WORLD, b, [], True, len(text), None)
    return text, single, tuples


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_every_program_prints_what_the_host_formatter_prints(paired, fastq):
    b = make_batch(130, -1, paired, fastq, seed=5 + paired, wrap_lower=not fastq)
    text0, single, tuples = default_tally(b)
    assert len(split_tuples(tuples)) > 3 and single.sum() > 10
    for cols in PROGRAMS:
        want = check(b, cols, tally=(single, tuples))
        if cols == DEFAULT:
            assert want == text0


@pytest.mark.parametrize("nq", fmtcases.TAIL_COUNTS)
@pytest.mark.parametrize("rows", fmtcases.TAIL_ROWS)
def test_wavefront_tails_and_row_counts(nq, rows):
    for paired, fastq in ((False, True), (True, False)):
        b = make_batch(nq, rows, paired, fastq, seed=nq + rows)
        tally = default_tally(b)[1:]
        for cols in (LIST_A, LIST_B, SAM):
            check(b, cols, tally=tally)


def test_byte_phases_and_the_lds_stage():
    lds = emu_cols.lib().emu_cols_lds_bytes()
    fits = beyond = 0
    for extra in range(4):
        for rows, lengths in ((1, [1, 15, 16, 17, 31, 32, 33]), (5, LENGTHS)):
            for cols in ([SEQ], [QUAL], LIST_A, SAM):
                b = make_batch(65, rows, False, True, seed=3, id_extra=extra, lengths=lengths)
                want = check(b, [READ_ID] + cols)
                stretch = len(expected(dict(b, qinfo=b["qinfo"][:64]), [READ_ID] + cols))
                fits += stretch + 3 <= lds
                beyond += stretch > lds
                assert len(want) > stretch
    assert fits >= 8 and beyond >= 8


def test_rows_that_do_not_fit_the_buffer_are_left_out():
    b = make_batch(65, 1, False, True, seed=9)
    fmtcases.check(run, b, SAM, out_cap=len(expected(b, SAM)) // 2)


def case_params(group):
    return pytest.mark.parametrize("case", range(len(fmtcases.cases(group))), ids=fmtcases.group_ids(group))


@case_params("digits")
def test_every_count_of_digits(case):
    fmtcases.check_case(run, fmtcases.cases("digits")[case])


LDS_BYTES = emu_cols.lib().emu_cols_lds_bytes()


@pytest.mark.parametrize("case", range(36), ids=fmtcases.group_ids("lds", LDS_BYTES))
def test_the_lds_stage_s_boundary(case):
    """stretches of exactly kFmtLds - phase bytes and one more: the very first wavefront, the first wavefront of the second block of
    256 threads at each phase, a wavefront that is not its block's first at each phase"""
    c = fmtcases.cases("lds", LDS_BYTES)[case]
    front, phase, stretch = c[6]
    sizes = [len(r) for r in fmtcases.expected_rows(c[1], DEFAULT if c[3] is BODIES else c[3])]
    assert sum(sizes[:front]) % 4 == phase and sum(sizes[front:front + 64]) == stretch and stretch - (LDS_BYTES - phase) in (0, 1)
    fmtcases.check_case(run, c)


@case_params("rooms")
def test_rooms_smaller_than_the_text(case):
    fmtcases.check_case(run, fmtcases.cases("rooms")[case])


@case_params("tuples")
def test_tuples_beyond_their_room_and_the_ballot_s_two_ends(case):
    fmtcases.check_case(run, fmtcases.cases("tuples")[case])


@case_params("names")
def test_empty_and_long_read_ids(case):
    fmtcases.check_case(run, fmtcases.cases("names")[case])


@case_params("tables")
def test_string_tables_at_their_edges(case):
    fmtcases.check_case(run, fmtcases.cases("tables")[case])


def test_the_tap_s_limits():
    """more than 32 columns and a code that is no column's are CF_ERR_ARG; a batch without queries prints nothing and launches nothing"""
    b = make_batch(3, 1, False, True, seed=1)
    with pytest.raises(capi.CfError, match="32 columns"):
        capi.debug_format(WORLD, b, [READ_ID] * 33, 100)
    with pytest.raises(capi.CfError, match="none of the formatter's"):
        capi.debug_format(WORLD, b, [READ_ID, 18], 100)
    capi.debug_format(WORLD, b, [READ_ID] * 32, 100)
    empty = fmtcases.assemble([], [], [], False, True, False, [], [], [])
    for cols in ([], SAM):
        text, sizes, total, single, tuples, words = capi.debug_format(WORLD, empty, cols, 64)
        assert text == bytes([fmtcases.UNWRITTEN]) * 64 and len(sizes) == 0 and total == 0 and not single.any() and len(tuples) == 0 and words == 0
    # a place outside the text is refused before anything is launched
    with pytest.raises(capi.CfError, match="outside the text"):
        capi.debug_format(WORLD, dict(b, idOff=[len(b["text"])] * 3), DEFAULT, 100)
