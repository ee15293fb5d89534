"""The three text entries of the batch ABI are ONE parser (cf_batch_upload_text, _bgzf, _bgzf_pair: include/centrifuge_amd.h), shown on
the GPU at the smallest shapes where the layout of the slot's text buffer can go wrong: the first one, two and three records of
synth_small's read files, the last readID lengthened until the text's length is 63, 0 and 1 modulo the 64 bytes of a marker piece
(kTextPiece), and the empty text.  Each text goes up as a plain block, as BGZF members of 64 and of 65,280 bytes of text, as a head
without members and as a head of 1, 63 and 64 bytes with the rest in members; mates as two plain blocks and as the members of two
files, with a head alone on either side.  Every way gives the reads, bases, longest read and printed rows of the plain block, and
leaves no tail.  No corrupt member comes here: those are tests/test_gpu_codec.py's, on the GPU as in the CPU harness."""
import os

import pytest

import common
from centrifuge_amd import capi
from test_gpu_inflate import members_of, slot_for

pytestmark = pytest.mark.gpu
PIECE = 64
RESIDUES = (63, 0, 1)
SIZES = (64, 65280)
HEADS = (1, 63, 64)


def fmt_of(name):
    return capi.TEXT_FASTQ if name.endswith(".fq") else capi.TEXT_FASTA


def shaped(name, n, residue):
    """the first n records of a golden read file, the last readID lengthened until the text is `residue` bytes beyond whole pieces"""
    d, _ = common.golden("synth_small")
    lines = open(os.path.join(d, name), "rb").read().split(b"\n")
    per = 4 if name.endswith(".fq") else 2
    assert lines[per][:1] == lines[0][:1] and lines[0][:1] in (b">", b"@")      # (a record is `per` lines)
    rec = lines[:per * n]
    size = sum(len(x) + 1 for x in rec)
    rec[per * (n - 1)] += b"x" * ((residue - size) % PIECE)
    text = b"\n".join(rec) + b"\n"
    assert len(text) % PIECE == residue
    return text


def single(slot, how, text, fmt, **kw):
    """-> (reads, bases, longest read, paired), the rows' text"""
    if how == "text":
        info = slot.submit_text(text, fmt, **kw)
    else:
        head = len(text) if how == "head" else how[1] if how[0] == "split" else 0
        mem = b"" if how == "head" else b"".join(members_of(text[head:], how[1] if how[0] == "members" else 65280))
        tail, info, z = slot.submit_bgzf(mem, fmt, head=text[:head], last=True, **kw)
        assert tail == b"" and not z.corrupt and z.inflated_bytes == len(text) - head, (how, tail, z.corrupt)
    assert not info.irregular, (how, info.irregular)
    return (info.n_reads, info.n_bases, info.max_len, info.paired), slot.wait_text()[0]


def ways(text):
    return [("members", s) for s in SIZES] + ["head"] + [("split", h) for h in HEADS if h <= len(text)]


SINGLE = [(name, n, r) for name in ("reads.fa", "reads.fq") for n in (1, 2, 3) for r in RESIDUES]


@pytest.mark.parametrize("name,n,residue", SINGLE)
def test_one_file_every_way_is_the_plain_block(name, n, residue):
    text, fmt = shaped(name, n, residue), fmt_of(name)
    clf, slot = slot_for()
    want = single(slot, "text", text, fmt)
    assert want[0][0] == n and want[0][3] == 0 and want[1].count(b"\n") >= n
    for how in ways(text):
        assert single(slot, how, text, fmt) == want, how
    slot.close(); clf.close()


@pytest.mark.parametrize("name", ["reads.fa", "reads.fq"])
def test_the_empty_text_every_way(name):
    clf, slot = slot_for()
    want = single(slot, "text", b"", fmt_of(name))
    assert want == ((0, 0, 0, 0), b"")
    for how in ways(b""):
        assert single(slot, how, b"", fmt_of(name)) == want, how
    slot.close(); clf.close()


def mates(slot, how, t1, t2, **kw):
    """-> (reads, bases, longest read), the rows' text.  (info.paired after a pair upload: tests/test_gpu_inflate_pair.py)"""
    if how == "text":
        info = slot.submit_text(t1, capi.TEXT_FASTA, text2=t2, **kw)
        assert info.paired == 1
    else:
        m1, m2 = (b"" if s == "head" else b"".join(members_of(t, s)) for s, t in zip(how, (t1, t2)))
        h1, h2 = (t if s == "head" else b"" for s, t in zip(how, (t1, t2)))
        tail1, tail2, info, z1, z2 = slot.submit_bgzf_pair(m1, m2, capi.TEXT_FASTA, head1=h1, head2=h2, last1=True, last2=True, **kw)
        assert (tail1, tail2) == (b"", b"") and not z1.corrupt and not z2.corrupt, (how, tail1, tail2)
        assert (z1.inflated_bytes, z2.inflated_bytes) == (len(t1) - len(h1), len(t2) - len(h2))
    assert not info.irregular, (how, info.irregular)
    return (info.n_reads, info.n_bases, info.max_len), slot.wait_text()[0]


MATE_WAYS = [(64, 64), (65280, 65280), (64, 65280), ("head", 64), (65280, "head"), ("head", "head")]


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_mates_every_way_are_the_two_plain_blocks(n, k):
    t1, t2 = shaped("r1.fa", n, RESIDUES[k]), shaped("r2.fa", n, RESIDUES[(k + 1) % 3])
    clf, slot = slot_for()
    want = mates(slot, "text", t1, t2)
    assert want[0][0] == 2 * n
    for how in MATE_WAYS:
        assert mates(slot, how, t1, t2) == want, how
    slot.close(); clf.close()


@pytest.mark.parametrize("option", ["trim", "skip"])
def test_trim_and_skip_through_the_three_entries(option):
    text, t1, t2 = shaped("reads.fq", 3, 0), shaped("r1.fa", 3, 63), shaped("r2.fa", 3, 1)
    clf, slot = slot_for()
    plain = single(slot, "text", text, capi.TEXT_FASTQ), mates(slot, "text", t1, t2)
    if option == "trim":
        slot.set_text_trim(3, 0)
    else:
        slot.set_text_skip(1)
    want = single(slot, "text", text, capi.TEXT_FASTQ)
    want2 = mates(slot, "text", t1, t2)
    # the option took effect: other rows (they print the query's length) for as many reads, or a record (a pair) fewer
    if option == "trim":
        assert (want[0][0], want2[0][0]) == (3, 6) and want[1] != plain[0][1] and want2[1] != plain[1][1]
    else:
        assert (want[0][0], want2[0][0]) == (2, 4)
    for how in ways(text):
        assert single(slot, how, text, capi.TEXT_FASTQ) == want, how
    for how in MATE_WAYS:
        assert mates(slot, how, t1, t2) == want2, how
    slot.close(); clf.close()
