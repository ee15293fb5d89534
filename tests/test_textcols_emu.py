"""Any list of columns on the device text path (fmt_cols_size_body / fmt_cols_write_body, centrifuge_amd/csrc/cf_textio.hpp) and the
default eight's own bodies in the CPU harness of tests/emu/emu_cols.cpp — the one-lane build and wavefronts of 64 lanes — against
the plain Python statements of tests/fmtcases.py (the table the device reads as well: tests/test_gpu_fmtcases.py), byte for byte:
synthetic blocks of FASTA (wrapped at 60 columns, lower case) and FASTQ text, unpaired and mates, with the sizes at which the
cooperative copy of the long fields changes its way (word and dword boundaries of the 2-bit expansion, the four byte phases of
a field's first byte, a wavefront's tail and a second wavefront, a block of four wavefronts, stretches inside and beyond the LDS
stage and on its very boundary), every count of digits, rooms smaller than the text and the tuples, odd names and string tables."""
import numpy as np
import pytest

import fmtcases
from centrifuge_amd import capi
from emu import emu_cols
from fmtcases import (BODIES, DEFAULT, LENGTHS, LIST_A, LIST_B, NAMES, PLACEHOLDER, PROGRAMS, QUAL, QUAL2, READ_ID, SAM, SEQ, WORLD, ZERO,
                      expected, first_diff, make_batch, split_tuples)


@pytest.fixture(params=[False, True], ids=["lane1", "wave64"])
def wave64(request):
    return request.param


def runner(wave64):
    return lambda W, b, cols, bodies, cap, tcap: emu_cols.format_full(W, b, DEFAULT if bodies else cols, wave64, bodies, cap, tcap)


def check(b, cols, wave64, tally=None):
    want = expected(b, cols)
    got, single, tuples = emu_cols.format_rows(WORLD, b, cols, wave64=wave64, out_cap=len(want))
    assert got == want, first_diff(got, want)
    if tally is not None:
        # the tally does not depend on the columns: what the default bodies leave on the same rows (the tuples in any order)
        assert np.array_equal(single, tally[0])
        assert sorted(split_tuples(tuples)) == sorted(split_tuples(tally[1]))
    # ... and everything the run returns against the Python statements, the tally among them
    assert fmtcases.check(runner(wave64), b, cols) == want
    return want


def default_tally(b, wave64):
    text, single, tuples = emu_cols.format_rows(WORLD, b, DEFAULT, wave64=wave64, default_bodies=True, out_cap=len(expected(b, DEFAULT)))
    fmtcases.check(runner(wave64), b, BODIES)
    return text, single, tuples


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_every_program_prints_what_the_host_formatter_prints(wave64, paired, fastq):
    # 130 queries with 0 / 1 / 5 / 2 rows in turn: two wavefronts and the tail of a third; a FASTA block wrapped at 60 columns, every
    # other record lower case
    b = make_batch(130, -1, paired, fastq, seed=5 + paired, wrap_lower=not fastq)
    text0, single, tuples = default_tally(b, wave64)
    assert len(split_tuples(tuples)) > 3 and single.sum() > 10
    for cols in PROGRAMS:
        want = check(b, cols, wave64, tally=(single, tuples))
        if cols == DEFAULT:
            assert want == text0                                       # the default eight through the new bodies: the old bodies' bytes


@pytest.mark.parametrize("nq", fmtcases.TAIL_COUNTS)
@pytest.mark.parametrize("rows", fmtcases.TAIL_ROWS)
def test_wavefront_tails_and_row_counts(wave64, nq, rows):
    for paired, fastq in ((False, True), (True, False)):
        b = make_batch(nq, rows, paired, fastq, seed=nq + rows)
        tally = default_tally(b, wave64)[1:]
        for cols in (LIST_A, LIST_B, SAM):
            check(b, cols, wave64, tally=tally)


def test_byte_phases_and_the_lds_stage(wave64):
    """the first byte of a wavefront's stretch, and with it of every long field, on each of the four places in a dword; stretches that
    fit the LDS stage (short reads, one row each) and stretches beyond it (five rows of up to 250 bases)"""
    lds = emu_cols.lib(wave64).emu_cols_lds_bytes()
    fits = beyond = 0
    for extra in range(4):
        for rows, lengths in ((1, [1, 15, 16, 17, 31, 32, 33]), (5, LENGTHS)):
            for cols in ([SEQ], [QUAL], LIST_A, SAM):
                b = make_batch(65, rows, False, True, seed=3, id_extra=extra, lengths=lengths)
                want = check(b, [READ_ID] + cols, wave64)
                # the bytes of the first wavefront's 64 queries
                stretch = len(expected(dict(b, qinfo=b["qinfo"][:64]), [READ_ID] + cols))
                fits += stretch + 3 <= lds
                beyond += stretch > lds
                assert len(want) > stretch
    assert fits >= 8 and beyond >= 8


def test_rows_that_do_not_fit_the_buffer_are_left_out(wave64):
    """the bounds of the write pass: with room for fewer bytes than the rows take, the rows that fit are printed and nothing is
    written past the room (the harness keeps marked bytes behind it)"""
    b = make_batch(65, 1, False, True, seed=9)
    want = expected(b, SAM)
    cut = len(want) // 2
    sizes = [len(expected(dict(b, qinfo=b["qinfo"][:q + 1]), SAM)) for q in range(65)]
    whole = max(s for s in sizes if s <= cut)
    part, _, _ = emu_cols.format_rows(WORLD, b, SAM, wave64=wave64, out_cap=cut)
    assert len(part) == cut and part[:whole] == want[:whole]
    fmtcases.check(runner(wave64), b, SAM, out_cap=cut)


def case_params(group):
    return pytest.mark.parametrize("case", range(len(fmtcases.cases(group))), ids=fmtcases.group_ids(group))


@case_params("digits")
def test_every_count_of_digits(wave64, case):
    c = fmtcases.cases("digits")[case]
    fmtcases.check_case(runner(wave64), c)


def test_the_lds_stage_s_boundary(wave64):
    """stretches of exactly kFmtLds - phase bytes and one more, for a block's first wavefront and another one (fmtcases.lds_cases)"""
    lds = emu_cols.lib(wave64).emu_cols_lds_bytes()
    table = fmtcases.cases("lds", lds)
    assert len(table) == 36
    for c in table:
        front, phase, stretch = c[6]
        sizes = [len(r) for r in fmtcases.expected_rows(c[1], DEFAULT if c[3] is BODIES else c[3])]
        assert sum(sizes[:front]) % 4 == phase and sum(sizes[front:front + 64]) == stretch and stretch - (lds - phase) in (0, 1)
        fmtcases.check_case(runner(wave64), c)


@case_params("rooms")
def test_rooms_smaller_than_the_text(wave64, case):
    c = fmtcases.cases("rooms")[case]
    fmtcases.check_case(runner(wave64), c)


@case_params("tuples")
def test_tuples_beyond_their_room_and_the_ballot_s_two_ends(wave64, case):
    c = fmtcases.cases("tuples")[case]
    fmtcases.check_case(runner(wave64), c)


@case_params("names")
def test_empty_and_long_read_ids(wave64, case):
    c = fmtcases.cases("names")[case]
    fmtcases.check_case(runner(wave64), c)


@case_params("tables")
def test_string_tables_at_their_edges(wave64, case):
    c = fmtcases.cases("tables")[case]
    fmtcases.check_case(runner(wave64), c)


def test_column_names_are_the_reference_s():
    """cf_text_column_of: the one table of names (no device needed); the codes are those of this file"""
    assert (capi.COL_READ_ID, capi.COL_QUAL2, capi.COL_PLACEHOLDER, capi.COL_ZERO, capi.TEXT_MAX_COLS) == (READ_ID, QUAL2, PLACEHOLDER, ZERO, 32)
    for n, c in NAMES.items():
        assert capi.text_column_of(n) == c, n
    assert capi.text_column_of("readID") == capi.COL_READ_ID and capi.text_column_of("QNAME") == capi.COL_READ_ID
    assert capi.text_column_of("taxLevel") == capi.COL_TAX_RANK and capi.text_column_of("taxRank") == capi.COL_TAX_RANK
    assert capi.text_column_of("CIGAR") == capi.COL_PLACEHOLDER and capi.text_column_of("MAPQ") == capi.COL_ZERO
    assert capi.text_column_of("QUAL2") == capi.COL_QUAL2 and capi.text_column_of("SEQ") == capi.COL_SEQ
    assert capi.text_column_of("readid") == -1 and capi.text_column_of("") == -1
