"""The device DEFLATE codec on the GPU at the format's corners, through its two test taps (cf_debug_inflate, cf_debug_deflate:
include/centrifuge_amd.h), which launch the kernels of the uploads and of cf_batch_wait_text_bgzf through the same host helpers,
with filled margins around every device buffer.  The reference is Python's zlib; the cases are the table of tests/codeccases.py,
which tests/test_inflate_emu.py and tests/test_deflate_emu.py put through the CPU harness first.

  inflate, well-formed   every stream of the table on both kernels (a wavefront per member, a lane per member); launches of 1, 3, 4,
                         5, 9 and of 1, 63, 64, 65 members, empty members, texts at every alignment
  inflate, corrupt       (TestCorrupt, a group of its own) every crafted stream, the CRC, two series of 100 seeded bit flips — each
                         corrupt member between two good ones: its status word, `bad`, the neighbours' text, the margins
  the real entries       cf_batch_upload_bgzf / _pair with one damaged member in a run: corrupt / bad_member in the right file, no
                         batch on the slot, the slot's next upload prints the golden rows
  the command line       a flipped byte and a file cut off inside a member: what --host-io answers
  deflate                sizes at a piece's and a member's edges at member sizes 64, 4,096 and 65,280, the text shapes of the table:
                         every member alone under zlib, BSIZE / ISIZE / CRC32, the CPU harness's bytes, and back through the inflater"""
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

import codeccases as K
import common
from centrifuge_amd import capi, reads
from emu import emu_deflate as D
from emu import emu_inflate as E
from test_gpu_cli_bgzf import bgzf as bgzf_file
from test_gpu_cli_bgzf_pair import fastq_of
from test_gpu_cli_text import CLI
from test_gpu_inflate import members_of, slot_for

pytestmark = pytest.mark.gpu
KERNELS = [False, True]                                 # by_lane
HEADER = reads.HEADER.encode()
GOOD = E.bgzf_member(K.GOOD_NEIGHBOUR)


def test_the_library_exports_the_taps():
    for name in ("cf_debug_inflate", "cf_debug_deflate"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)


def inflate_ok(members, texts, by_lane):
    """whole members through the tap (which checks the margins): zlib's text, member by member; every status word 0 -> blocks"""
    for m, t in zip(members, texts):
        assert zlib.decompress(m, 31) == t
    out, status, blocks, bad = capi.debug_inflate(b"".join(members), by_lane)
    want = b"".join(texts)
    assert len(status) == len(members) and not status.any() and bad is None, (bad, status)
    assert out == want, common.first_diff(out.decode("latin1"), want.decode("latin1"))
    return blocks


# ---- inflate, well-formed
@pytest.mark.parametrize("by_lane", KERNELS)
@pytest.mark.parametrize("name", K.WELL_FORMED_NAMES)
def test_well_formed_streams(name, by_lane):
    members, min_blocks = K.well_formed()[name]
    # (a short member in front: the case's text starts at an odd place)
    blocks = inflate_ok([GOOD] + [m for _, m in members], [K.GOOD_NEIGHBOUR] + [t for t, _ in members], by_lane)
    assert blocks[0] == 1 and blocks[1] >= min_blocks, blocks


@pytest.mark.parametrize("by_lane", KERNELS)
def test_sizes_and_distances(by_lane):
    for texts, kw in K.sizes_and_distances():
        if kw["level"] in (0, 9):                        # (the levels between give the same kinds of streams: the CPU harness has them)
            inflate_ok([E.bgzf_member(t, **kw) for t in texts], texts, by_lane)


def shaped(lens):
    texts = [K.TEXT[997 * i:997 * i + n] for i, n in enumerate(lens)]
    return [E.bgzf_member(t) for t in texts], texts


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_a_wavefront_per_member_with_a_last_block_that_is_partly_empty(n):
    """four wavefronts a block; texts of 9 bytes and more: the members' texts start at every alignment 0 .. 7"""
    lens = [9, 9, 9, 9, 9, 9, 9, 17, 777][:n]
    if n == 9:
        assert {sum(lens[:i]) % 8 for i in range(9)} == set(range(8))
    inflate_ok(*shaped(lens), by_lane=False)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_a_lane_per_tiny_member(n):
    lens = [i % 13 + 1 for i in range(n)]
    inflate_ok(*shaped(lens), by_lane=True)
    if n == 65:
        assert {sum(lens[:i]) % 8 for i in range(n)} == set(range(8))


@pytest.mark.parametrize("by_lane", KERNELS)
def test_empty_members_first_last_and_in_between(by_lane):
    inflate_ok(*shaped([0, 701, 0, 0, 33, 0]), by_lane=by_lane)
    inflate_ok(*shaped([0]), by_lane=by_lane)
    inflate_ok(*shaped([0, 0, 0, 0, 0]), by_lane=by_lane)
    assert capi.debug_inflate(b"", by_lane)[0] == b""      # no member at all: nothing is launched


def test_a_header_that_is_not_bgzfs_is_the_hosts_to_refuse():
    bad = bytearray(GOOD); bad[12] = ord("X")
    with pytest.raises(capi.CfError):
        capi.debug_inflate(GOOD + bytes(bad))


# ---- inflate, corrupt: the purpose is the status.  Only streams the CPU harness has been given (tests/test_inflate_emu.py reads
# the same table and checks the guard bytes around them) come here.
def corrupt_between_good(corrupt, texts_claimed, by_lane):
    """good, corrupt[0], good, corrupt[1], ..., good -> the corrupt members' status words; asserts the neighbours and `bad`"""
    members = [GOOD]
    for m in corrupt:
        members += [m, GOOD]
    out, status, blocks, bad = capi.debug_inflate(b"".join(members), by_lane)          # (the tap checks the margins)
    assert len(status) == len(members) and not status[0::2].any(), status
    words = status[1::2]
    firsts = [i for i, w in enumerate(words) if w]
    assert bad == (2 * firsts[0] + 1 if firsts else None)
    # every good member's text, wherever it lies: nothing was written beyond a corrupt member's own ISIZE bytes
    at = 0
    for i, claimed in enumerate(texts_claimed):
        assert out[at:at + len(K.GOOD_NEIGHBOUR)] == K.GOOD_NEIGHBOUR, i
        at += len(K.GOOD_NEIGHBOUR) + claimed
    assert out[at:] == K.GOOD_NEIGHBOUR
    return words, out


class TestCorrupt:
    @pytest.mark.parametrize("by_lane", KERNELS)
    def test_corrupt_crafted_streams_end_in_the_tables_word(self, by_lane):
        names = sorted(K.CRAFTED)
        for name in names:                                # zlib refuses it too, or leaves another text
            payload, text, word = K.CRAFTED[name]
            try:
                d = zlib.decompressobj(-15)
                assert d.decompress(payload) != text or not d.eof, name
            except zlib.error:
                pass
        # each in a launch of three members, then all of them in one
        for name in names:
            payload, text, word = K.CRAFTED[name]
            words, _ = corrupt_between_good([E.bgzf_member(text, payload=payload)], [len(text)], by_lane)
            assert list(words) == [word], name
        words, _ = corrupt_between_good([E.bgzf_member(K.CRAFTED[n][1], payload=K.CRAFTED[n][0]) for n in names], [len(K.CRAFTED[n][1]) for n in names], by_lane)
        assert list(words) == [K.CRAFTED[n][2] for n in names]

    @pytest.mark.parametrize("by_lane", KERNELS)
    def test_corrupt_distance_one_byte_before_the_member(self, by_lane):
        short, claimed = K.distance_limit()[1]
        words, _ = corrupt_between_good([E.bgzf_member(claimed, payload=short)], [len(claimed)], by_lane)
        assert list(words) == [E.DIST_TOO_FAR]

    @pytest.mark.parametrize("by_lane", KERNELS)
    def test_corrupt_crc(self, by_lane):
        words, out = corrupt_between_good([K.crc_flip()], [len(K.CRC_TEXT)], by_lane)
        assert list(words) == [E.CRC]
        assert out[len(K.GOOD_NEIGHBOUR):][:len(K.CRC_TEXT)] == K.CRC_TEXT          # (the text itself is whole)

    @pytest.mark.parametrize("by_lane", KERNELS)
    @pytest.mark.parametrize("level", [0, 6])
    def test_corrupt_single_bit_flips(self, level, by_lane):
        """one launch, a flipped member per member slot: the word is non-zero exactly when zlib refuses the member or reads another text"""
        series = K.flips(level)
        assert len(series) == 100
        words, out = corrupt_between_good([x for x, _ in series], [len(K.FLIP_TEXT)] * 100, by_lane)
        assert [w == 0 for w in words] == [ok for _, ok in series], list(words)
        assert sum(1 for w in words if w) > 50
        step = len(K.GOOD_NEIGHBOUR) + len(K.FLIP_TEXT)
        for i, (_, ok) in enumerate(series):
            if ok:
                assert out[i * step + len(K.GOOD_NEIGHBOUR):(i + 1) * step] == K.FLIP_TEXT, i


# ---- the real entries with a corrupt member in a run of members of 700 bytes
DAMAGE = ["crc", "distance before the member", "text shorter than ISIZE"]


def damaged(member, how):
    """-> the member damaged, the word the entry reports"""
    if how == "crc":
        m = bytearray(member); m[-8] ^= 1
        return bytes(m), E.CRC
    payload, text, word = K.CRAFTED[how]
    return E.bgzf_member(text, payload=payload), word


def golden_rows(case):
    d, cases = common.golden("synth_small")
    return open(os.path.join(d, [c for c in cases if c["name"] == case][0]["tsv"]), "rb").read()


def single_entry(how):
    d, _ = common.golden("synth_small")
    text = open(os.path.join(d, "reads.fq"), "rb").read()
    want = golden_rows("fastq")
    mem = members_of(text, 700)[:-1]
    clf, slot = slot_for()
    clf.reset_counts()
    tail, info, z = slot.submit_bgzf(b"".join(mem), capi.TEXT_FASTQ, last=True)
    assert tail == b"" and HEADER + slot.wait_text()[0] == want
    clean = clf.counts()
    for at in (0, len(mem) // 2, len(mem) - 1):
        bad, word = damaged(mem[at], how)
        clf.reset_counts()
        tail, info, z = slot.submit_bgzf(b"".join(mem[:at] + [bad] + mem[at + 1:]), capi.TEXT_FASTQ, last=True)
        assert tail is None and (z.corrupt, z.bad_member) == (word, at), (how, at, z.corrupt, z.bad_member)
        with pytest.raises(capi.CfError):                 # the slot holds no batch
            slot.wait_text()
        tail, info, z = slot.submit_bgzf(b"".join(mem), capi.TEXT_FASTQ, last=True)
        assert tail == b"" and not z.corrupt and not info.irregular
        assert HEADER + slot.wait_text()[0] == want, (how, at)
        now = clf.counts()
        assert np.array_equal(now[0], clean[0]) and np.array_equal(now[1], clean[1])
    slot.close(); clf.close()


@pytest.mark.parametrize("how", DAMAGE)
def test_upload_bgzf_reports_a_corrupt_member_and_leaves_a_usable_slot(how):
    single_entry(how)


def test_upload_bgzf_with_a_lane_per_member_reports_a_corrupt_member():
    """the same with CF_INFLATE_LANES=1 (read once a process: a child)"""
    code = "import sys; sys.path[:0] = %r; import test_gpu_codec as T; [T.single_entry(h) for h in T.DAMAGE]; print('single entry ok')" % [common.ROOT, os.path.dirname(os.path.abspath(__file__))]
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=170, env=dict(os.environ, CF_INFLATE_LANES="1", CF_DEBUG_KNOBS="1"))
    assert r.returncode == 0 and "single entry ok" in r.stdout, r.stderr[-4000:]


@pytest.mark.parametrize("how", DAMAGE)
def test_upload_bgzf_pair_reports_a_corrupt_member_in_its_file(how):
    d, _ = common.golden("synth_small")
    t1, t2 = (open(os.path.join(d, f), "rb").read() for f in ("r1.fa", "r2.fa"))
    want = golden_rows("pe_k5")
    mem = [members_of(t1, 700)[:-1], members_of(t2, 700)[:-1]]
    clf, slot = slot_for()

    def upload(m1, m2):
        return slot.submit_bgzf_pair(b"".join(m1), b"".join(m2), capi.TEXT_FASTA, last1=True, last2=True)
    clf.reset_counts()
    tail1, tail2, info, z1, z2 = upload(*mem)
    assert (tail1, tail2) == (b"", b"") and HEADER + slot.wait_text()[0] == want
    clean = clf.counts()
    for f in (0, 1):
        for at in (0, len(mem[f]) // 2, len(mem[f]) - 1):
            bad, word = damaged(mem[f][at], how)
            run = [list(mem[0]), list(mem[1])]
            run[f][at] = bad
            clf.reset_counts()
            tail1, tail2, info, z1, z2 = upload(*run)
            z = (z1, z2)
            assert tail1 is None and tail2 is None
            assert (z[f].corrupt, z[f].bad_member) == (word, at) and z[1 - f].corrupt == 0, (how, f, at, z1.corrupt, z1.bad_member, z2.corrupt, z2.bad_member)
            with pytest.raises(capi.CfError):
                slot.wait_text()
            tail1, tail2, info, z1, z2 = upload(*mem)
            assert (tail1, tail2) == (b"", b"") and not z1.corrupt and not z2.corrupt and not info.irregular
            assert HEADER + slot.wait_text()[0] == want, (how, f, at)
            now = clf.counts()
            assert np.array_equal(now[0], clean[0]) and np.array_equal(now[1], clean[1])
    slot.close(); clf.close()


# ---- the command line: a damaged BGZF file answers as --host-io does
def cli(args, t, tag, env=None):
    """-> exit status, stdout, the error message (stderr's lines that are one)"""
    r = subprocess.run([CLI] + args + ["--report-file", os.path.join(t, tag + ".rep")], capture_output=True, timeout=170, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, [ln for ln in r.stderr.decode("latin1").splitlines() if ln.startswith(("Error", "Warning", "centrifuge-class:"))]


def flipped_file(text):
    """the BGZF file of text with one payload byte of a middle member flipped"""
    blob = bytearray(bgzf_file(text))
    table, _ = E.member_table(bytes(blob))
    off, n = int(table[len(table) // 2, 0]), int(table[len(table) // 2, 1])
    blob[off + n // 2] ^= 0x10
    return bytes(blob)


def truncated_file(text):
    """... cut off inside a middle member"""
    blob = bgzf_file(text)
    table, _ = E.member_table(blob)
    return blob[:int(table[len(table) // 2, 0]) + int(table[len(table) // 2, 1]) // 2]


@pytest.mark.parametrize("damage", [flipped_file, truncated_file])
def test_cli_on_a_damaged_bgzf_file_answers_as_the_host_reader_does(damage):
    d, _ = common.golden("synth_small")
    idx = os.path.join(d, "idx")
    fq = open(os.path.join(d, "reads.fq"), "rb").read()
    m1, m2 = (b"".join(fastq_of(open(os.path.join(d, f), "rb").read(), s)) for f, s in (("r1.fa", 1), ("r2.fa", 2)))
    with tempfile.TemporaryDirectory() as t:
        def put(name, data):
            with open(os.path.join(t, name), "wb") as f:
                f.write(data)
            return os.path.join(t, name)
        single = ["-q", "-p", "4", "-x", idx, "-U", put("reads.fq.gz", damage(fq))]
        runs = [(single, [])]
        for f in (0, 1):
            g = [put("m%d_r1.fq.gz" % f, damage(m1) if f == 0 else bgzf_file(m1)), put("m%d_r2.fq.gz" % f, damage(m2) if f == 1 else bgzf_file(m2))]
            runs.append((["-q", "-p", "4", "-x", idx, "-1", g[0], "-2", g[1]], ["--device-inflate", "all"]))
        for args, dev in runs:
            host = cli(args + ["--host-io"], t, "h")
            assert host[0] != 0 and host[2], host
            got = cli(args + dev, t, "d")
            assert got[0] == host[0] and got[2] == host[2], (args, got[0], got[2], host[0], host[2])
            assert got[1] == host[1], common.first_diff(got[1].decode("latin1"), host[1].decode("latin1"))
            # in runs of 4,096 bytes the runs in front of the damaged member are printed before the rest is handed over (how many
            # of them the host readers print before they meet it is a matter of timing): the status and the message are the same
            got = cli(args + dev, t, "s", env={"CF_TEXT_BLOCK": "4096"})
            assert got[0] == host[0] and got[2] == host[2] and got[1].startswith(host[1]), (args, got[0], got[2])


# ---- deflate
BGZF_HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")           # MTIME 0, XFL 0, OS 255, XLEN 6, BC 2


def deflate_ok(text, member=K.MEMBER, back=True):
    """text through the tap (which checks the margins and every member's room) -> the members, their sizes"""
    blob, sizes = capi.debug_deflate(text, member)
    n = (len(text) + member - 1) // member
    assert len(sizes) == n and int(sizes.sum()) == len(blob)
    at = 0
    for m in range(n):
        piece, mem = text[m * member:(m + 1) * member], blob[at:at + int(sizes[m])]
        assert zlib.decompress(mem, 31) == piece, m                                        # the member alone, under zlib
        assert mem[:16] == BGZF_HEAD and struct.unpack("<H", mem[16:18])[0] == len(mem) - 1 and len(mem) <= 65536, m
        assert struct.unpack("<II", mem[-8:]) == (zlib.crc32(piece), len(piece)), m
        assert mem[18] & 1 == 1 and (mem[18] >> 1) & 3 in (0, 1)                          # one final block, stored or fixed
        assert len(mem) - 26 <= len(piece) + 5
        at += int(sizes[m])
    emu_blob, emu_sizes = D.deflate(text, member)
    assert blob == emu_blob and list(sizes) == list(emu_sizes)                              # the bytes are a function of (text, member)
    if back and text:
        for by_lane in KERNELS:
            inflate_ok([blob[int(sizes[:m].sum()):int(sizes[:m + 1].sum())] for m in range(n)], [text[m * member:(m + 1) * member] for m in range(n)], by_lane)
    return blob, sizes


def is_stored(member_bytes):
    return (member_bytes[18] >> 1) & 3 == 0


@pytest.mark.parametrize("member", [64, 4096, 65280])
def test_deflate_sizes_at_the_edges_of_a_piece_and_of_a_member(member):
    piece = member // 64
    sizes = [1, 2, 3, 4, piece - 1, piece, piece + 1, member - 1, member, member + 1, 3 * member + 7]
    if member == K.MEMBER:
        assert sizes[:-1] == K.EDGE_SIZES
    for n in sizes:
        blob, s = deflate_ok(K.rows_text(n), member)
        assert len(s) == -(-n // member)
        if n == 3 * member + 7:
            assert len(s) == 4 and struct.unpack("<I", blob[-4:])[0] == 7                  # an even number of members, the last of 7 bytes
        if n == member + 1:
            assert len(s) == 2 and struct.unpack("<I", blob[-4:])[0] == 1                  # an odd wavefront idles in the last block
    # an odd number of members, the last one full
    assert len(deflate_ok(K.rows_text(3 * member), member)[1]) == 3


def test_deflate_an_empty_text_gives_no_member():
    blob, sizes = capi.debug_deflate(b"", 4096)
    assert blob == b"" and len(sizes) == 0


def test_deflate_refuses_a_member_size_that_is_none():
    for bad in (0, 32, 100, 65344, 1 << 16):
        with pytest.raises(capi.CfError):
            capi.debug_deflate(b"abc", bad)


@pytest.mark.parametrize("n", K.ONE_BYTE_RUNS)
def test_deflate_one_byte_repeated(n):
    blob, _ = deflate_ok(b"\0" * n)
    assert len(blob) < n // 16 + 64


@pytest.mark.parametrize("n", K.PERIODS)
def test_deflate_a_distance_shorter_than_the_match(n):
    deflate_ok(b"ACGTA" * n)
    deflate_ok(b"AB" * n + b"A")


def test_deflate_matches_at_the_very_end_and_across_a_piece_end():
    for text in K.match_end_texts():
        deflate_ok(text)
    for text in K.match_end_texts(4096 // 64 + 64):       # (runs of 64 bytes over the ends of several pieces of 64)
        deflate_ok(text, 4096)
    deflate_ok(K.member_end_text())


def test_deflate_nine_bit_literals_mixed_with_ascii():
    for text, member in K.nine_bit_texts():
        deflate_ok(text, member)


def test_deflate_random_bytes_come_out_stored():
    text = K.random_member()
    blob, sizes = deflate_ok(text)
    assert len(sizes) == 1 and is_stored(blob) and len(blob) == K.MEMBER + 5 + 26
    blob, sizes = deflate_ok(K.high_then_ascii(), member=4096)
    assert is_stored(blob[:sizes[0]]) and not is_stored(blob[sizes[0]:])
    # members of 64 random bytes (no three of them repeat): stored exactly where the literals' fixed block — 3 bits, 8 or 9 a byte,
    # 7 for the end — would take more bytes than the text and 5
    part = K.threshold_text()
    blob, sizes = deflate_ok(part, member=64)
    assert K.stored_where_shorter(part, 64, [is_stored(blob[int(sizes[:m].sum()):]) for m in range(len(sizes))])


def test_deflate_the_golden_tsv_twice():
    text = golden_rows("k5")
    for member in (4096, K.MEMBER):
        a, sizes = deflate_ok(text, member)
        assert len(a) < len(text) and (member != 4096 or len(sizes) >= 24)
        assert capi.debug_deflate(text, member)[0] == a


def test_deflate_a_member_does_not_look_back_into_the_one_before():
    text = golden_rows("k5")
    for member in (4096, 1024):
        part = text[:3 * member + 77]
        blob, sizes = deflate_ok(part, member, back=False)
        at = 0
        for m in range(len(sizes)):
            assert blob[at:at + int(sizes[m])] == capi.debug_deflate(part[m * member:(m + 1) * member], member)[0], m
            at += int(sizes[m])
