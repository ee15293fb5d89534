"""The device deflater (deflate_body, centrifuge_amd/csrc/cf_deflate.hpp) in the CPU harness of tests/emu/emu_deflate.cpp — wavefronts
of 64 fibers, one per BGZF member — against zlib, gzip and the device INFLATER's harness: every member's header, BSIZE, payload, CRC32
and ISIZE; the texts at a lane piece's and a member's edges; matches at distance 1, shorter than their length, at a text's very
end and clipped at a piece's end; 9-bit literals; the stored fallback.  The guard bytes the harness puts around the text, the
members and behind each member in its room stay as they are (emu_deflate.deflate asserts it)."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import codeccases as K
import common
from emu import emu_deflate as D
from emu import emu_inflate as I

EOF = D.EOF_MEMBER
PIECE = K.PIECE
assert K.MEMBER == D.MEMBER


def check(text, member=D.MEMBER):
    """text through the harness and back, every way the issue names -> the members (bytes), their sizes"""
    blob, sizes = D.deflate(text, member)
    n_members = (len(text) + member - 1) // member
    assert len(sizes) == n_members and int(sizes.sum()) == len(blob)
    if not text:
        assert blob == b""
        return blob, sizes
    table, n_out = I.member_table(blob)                  # (asserts the magic, the BC subfield)
    assert len(table) == n_members and n_out == len(text)
    at = 0
    for m, (p_off, p_len, t_off, t_len, crc) in enumerate(table.tolist()):
        piece = text[m * member:(m + 1) * member]
        head = blob[at:at + 18]
        assert head[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), m           # MTIME 0, XFL 0, OS 255, XLEN 6, BC 2
        assert struct.unpack("<H", head[16:])[0] == int(sizes[m]) - 1 and sizes[m] <= 65536
        assert p_off == at + 18 and p_len == sizes[m] - 26 and t_off == m * member and t_len == len(piece)
        payload = blob[p_off:p_off + p_len]
        assert zlib.decompress(payload, -15) == piece, m
        assert crc == zlib.crc32(piece) & 0xffffffff, m
        assert payload[0] & 1 == 1 and (payload[0] >> 1) & 3 in (0, 1)                        # one final block, stored or fixed
        if (payload[0] >> 1) & 3 == 0:
            assert p_len == len(piece) + 5
        else:
            assert p_len <= len(piece) + 5
        at += int(sizes[m])
    assert at == len(blob)
    assert gzip.decompress(blob + EOF) == text
    out, err, bad = I.inflate(blob, table, n_out, wave64=True)
    assert bad is None and not err.any() and out == text
    return blob, sizes


def is_stored(member_bytes):
    return (member_bytes[18] >> 1) & 3 == 0


def test_eof_member_is_an_empty_gzip_member():
    assert len(EOF) == 28 and gzip.decompress(EOF) == b"" and struct.unpack("<H", EOF[16:18])[0] == 27


def test_empty_text_gives_no_member():
    blob, sizes = check(b"")
    assert blob == b"" and len(sizes) == 0


def test_the_tables_sizes_are_the_edges():
    assert K.EDGE_SIZES == [1, 2, 3, 4, PIECE - 1, PIECE, PIECE + 1, D.MEMBER - 1, D.MEMBER, D.MEMBER + 1]
    assert K.ONE_BYTE_RUNS == [3, 257, 258, 259, 260, PIECE, PIECE + 2, 3 * PIECE + 7, D.MEMBER, D.MEMBER + 300]
    assert K.PERIODS == [1, 2, 52, 500, 13056, 13057]


@pytest.mark.parametrize("n", K.EDGE_SIZES)
def test_sizes_at_the_edges_of_a_piece_and_of_a_member(n):
    text = K.rows_text(n)
    blob, sizes = check(text)
    assert len(sizes) == (2 if n > D.MEMBER else 1)
    if n == D.MEMBER + 1:
        assert struct.unpack("<I", blob[-4:])[0] == 1     # the second member holds one byte


def golden_tsvs():
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == "fastq"][0]
    tsv = open(os.path.join(d, c["tsv"]), "rb").read()
    # the same rows as --tab-fmt-cols readID,taxID,readSeq,readQual prints them
    ls = open(os.path.join(d, "reads.fq"), "rb").read().split(b"\n")
    reads = {ls[k][1:]: (ls[k + 1], ls[k + 3]) for k in range(0, len(ls) - 1, 4)}
    rows = [b"readID\ttaxID\treadSeq\treadQual\n"]
    for ln in tsv.split(b"\n")[1:-1]:
        f = ln.split(b"\t")
        rows.append(b"\t".join((f[0], f[2]) + reads[f[0]]) + b"\n")
    k5 = open(os.path.join(d, [x for x in cases if x["name"] == "k5"][0]["tsv"]), "rb").read()
    return {"default": k5, "fastq": tsv, "cols": b"".join(rows)}


@pytest.mark.parametrize("which", ["default", "fastq", "cols"])
def test_golden_tsv_in_dozens_of_members(which):
    text = golden_tsvs()[which]
    blob, sizes = check(text, member=4096)
    assert len(sizes) == (len(text) + 4095) // 4096 and (len(sizes) >= 24 or which == "fastq")
    assert len(blob) < len(text)                          # the members together are smaller than the text
    if which == "default":
        assert len(check(text)[0]) < len(text)            # ... at the default member size too


@pytest.mark.parametrize("n", K.ONE_BYTE_RUNS)
def test_one_byte_repeated(n):
    """distance 1, matches of 258 that run into the ends of pieces and members"""
    blob, _ = check(b"\0" * n)
    assert len(blob) < n // 16 + 64


@pytest.mark.parametrize("n", K.PERIODS)
def test_distance_shorter_than_the_match(n):
    check(b"ACGTA" * n)
    check(b"AB" * n + b"A")


def test_matches_at_the_very_end_and_across_a_piece_end():
    # the last three bytes are a match; a run that starts in front of a piece's end and goes on behind it: the match is clipped at
    # the end, the next lane starts anew
    texts = K.match_end_texts()
    assert len(texts) == 7 and texts[0] == b"abcdefgh-xyz-abc"
    for text in texts:
        check(text)
    # ... the same at a member's end
    check(K.member_end_text())


def test_nine_bit_literals_mixed_with_ascii():
    texts = K.nine_bit_texts()
    assert len(texts) == 3 and texts[1] == (K.high_bytes(), D.MEMBER) and texts[2][1] == 1024
    for text, member in texts:
        check(text, member=member)


def test_random_bytes_are_stored():
    text = K.random_member()
    assert len(text) == D.MEMBER
    blob, sizes = check(text)
    assert len(sizes) == 1 and is_stored(blob) and len(blob) == D.MEMBER + 5 + 26
    # names of bytes >= 144 only: 9 bits a literal, stored as well; a member of both kinds of text is not
    blob, sizes = check(K.high_then_ascii(), member=4096)
    assert is_stored(blob[:sizes[0]]) and not is_stored(blob[sizes[0]:])


def test_the_stored_form_is_taken_only_where_it_is_shorter():
    """members of 64 random bytes: stored exactly where the literals' fixed block would take more bytes than the text and 5, fixed
    where the two are equal"""
    part = K.threshold_text()
    blob, sizes = check(part, member=64)
    assert K.stored_where_shorter(part, 64, [is_stored(blob[int(sizes[:m].sum()):]) for m in range(len(sizes))])


def test_the_bytes_are_a_function_of_the_text():
    texts = golden_tsvs()
    for member in (4096, D.MEMBER):
        a, _ = D.deflate(texts["default"], member)
        b, _ = D.deflate(texts["default"], member)
        assert a == b


def test_a_member_does_not_look_back_into_the_one_before():
    text = golden_tsvs()["default"]
    for member in (4096, 1024):
        blob, sizes = D.deflate(text[:3 * member + 77], member)
        at = 0
        for m in range(len(sizes)):
            alone, _ = D.deflate(text[m * member:(m + 1) * member][:3 * member + 77 - m * member], member)
            assert blob[at:at + int(sizes[m])] == alone, m
            at += int(sizes[m])


def test_knob_values_outside_the_range_are_refused():
    L = D.lib()
    import ctypes as C
    out, n, size = np.zeros(1 << 17, dtype=np.uint8), C.c_uint64(0), np.zeros(8, dtype=np.uint32)
    for bad in (0, 32, 100, 65344, 1 << 16):
        assert L.emu_deflate(b"abc", 3, bad, out.ctypes.data, C.byref(n), size.ctypes.data) == 2 ** 64 - 3
    assert L.emu_deflate_table_bytes() == 32768 and L.emu_deflate_window() == 1024
