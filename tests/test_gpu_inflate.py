"""BGZF members through the batch ABI on the GPU (cf_batch_upload_bgzf: include/centrifuge_amd.h): the read files of synth_small as
BGZF members made here with zlib — 700 bytes of text each, 65,280 (bgzip's size) and as much as a member takes —, uploaded in runs
of one, three and all members with the tails handed on; the reads that come out and the rows printed for them are those of the
plain file through cf_batch_upload_text, and the reference's golden TSV.  Corrupt members — in the CPU harness
(tests/test_inflate_emu.py) and, through this entry and the inflater's tap, on the GPU — are tests/test_gpu_codec.py's."""
import os

import pytest

import common
from centrifuge_amd import capi, reads
from emu import emu_inflate as E
from test_async_abi import dev_index

pytestmark = pytest.mark.gpu
HEADER = reads.HEADER.encode()
_plain = {}


def test_the_library_exports_the_bgzf_upload():
    assert "cf_batch_upload_bgzf" in capi.EXPORTS and hasattr(capi.lib(), "cf_batch_upload_bgzf")
    assert hasattr(capi.Slot, "submit_bgzf")


def members_of(text, size, level=6):
    return [E.bgzf_member(text[i:i + size], level=level) for i in range(0, len(text), size)] + [E.bgzf_member(b"")]     # (the empty member a BGZF file ends with)


def slot_for(arch="synth_small"):
    ix = dev_index(arch)
    clf = capi.Classifier(ix)
    slot = capi.Slot(clf)
    slot.set_result_format(capi.RESULTS_NARROW)
    return clf, slot


def plain(name):
    """what cf_batch_upload_text makes of the whole plain file: its info and printed rows (made once)"""
    if name not in _plain:
        d, _ = common.golden("synth_small")
        text = open(os.path.join(d, name), "rb").read()
        clf, slot = slot_for()
        info = slot.submit_text(text, capi.TEXT_FASTQ if name.endswith(".fq") else capi.TEXT_FASTA)
        assert not info.irregular
        _plain[name] = (text, (info.n_reads, info.n_bases, info.max_len), slot.wait_text()[0])
        slot.close(); clf.close()
    return _plain[name]


def through_bgzf(text, fmt, size, run, max_reads=0):
    """-> reads, bases, longest read, the rows' text, the runs that held no whole record"""
    mem = members_of(text, size)
    run = run or len(mem)
    clf, slot = slot_for()
    tail, out, n_reads, n_bases, max_len, empty, inflated = b"", b"", 0, 0, 0, 0, 0
    for i in range(0, len(mem), run):
        last = i + run >= len(mem)
        tail, info, z = slot.submit_bgzf(b"".join(mem[i:i + run]), fmt, head=tail, last=last, max_reads=max_reads)
        assert tail is not None and not info.irregular and not z.corrupt, (i, info.irregular, z.corrupt, z.bad_member)
        inflated += z.inflated_bytes
        n_reads += info.n_reads; n_bases += info.n_bases; max_len = max(max_len, info.max_len)
        empty += info.n_reads == 0
        if info.n_reads:
            out += slot.wait_text()[0]
        else:
            slot.wait_text()
    assert tail == b"" and inflated == len(text)
    slot.close(); clf.close()
    return n_reads, n_bases, max_len, out, empty


@pytest.mark.parametrize("run", [1, 3, 0])
@pytest.mark.parametrize("size", [700, 65280, 65536])
@pytest.mark.parametrize("name,case", [("reads.fq", "fastq"), ("reads.fa", "k5")])
def test_members_in_runs_give_the_reads_and_rows_of_the_plain_file(name, case, size, run):
    text, info, rows = plain(name)
    d, cases = common.golden("synth_small")
    n_reads, n_bases, max_len, out, _ = through_bgzf(text, capi.TEXT_FASTQ if name.endswith(".fq") else capi.TEXT_FASTA, size, run)
    assert (n_reads, n_bases, max_len) == info
    assert out == rows
    want = open(os.path.join(d, [c for c in cases if c["name"] == case][0]["tsv"]), "rb").read()
    assert HEADER + out == want, common.first_diff((HEADER + out).decode("latin1"), want.decode("latin1"))


def test_runs_without_a_whole_record():
    text, info, rows = plain("reads250.fa")
    whole = text[:text.rindex(b">", 0, 20000)]
    n_reads, n_bases, max_len, out, empty = through_bgzf(whole, capi.TEXT_FASTA, 100, 1)
    assert empty > 50
    n = whole.count(b">")
    assert n_reads == n and rows.startswith(out) and out.count(b"\n") >= n


def test_last_on_a_fastq_text_that_ends_inside_a_record_is_irregular():
    text = plain("reads.fq")[0]
    cut = text.index(b"\n+\n", 3000) + 3
    clf, slot = slot_for()
    tail, info, z = slot.submit_bgzf(b"".join(members_of(text[:cut], 700)), capi.TEXT_FASTQ, last=True)
    assert tail is None and info.irregular and not z.corrupt
    # the same members with more to follow: the open record is the tail
    tail, info, z = slot.submit_bgzf(b"".join(members_of(text[:cut], 700)), capi.TEXT_FASTQ, last=False)
    assert not info.irregular and text[:cut].endswith(tail) and tail.startswith(b"@") and tail.count(b"\n") == 3
    slot.wait_text()
    slot.close(); clf.close()


def test_refusals_leave_no_batch():
    """a tail beyond the slot's room (1 MiB at least), a text beyond the batch's 32-bit places, a member whose header is not BGZF's
    (found by the host while it makes the table: no kernel sees it)"""
    clf, slot = slot_for()
    # one FASTA record of 2.2 MB with more to follow: no cut but the text's start, everything is tail
    text = b">long\n" + b"ACGT" * 550000
    tail, info, z = slot.submit_bgzf(b"".join(members_of(text, 65536)[:-1]), capi.TEXT_FASTA, last=False)
    assert tail is None and info.irregular & 4096 and not z.corrupt          # CF_TEXT_TAIL_ROOM
    good = E.bgzf_member(b">r\nACGT\n")
    bad = bytearray(good); bad[12] = ord("X")                                  # no 'BC' field
    tail, info, z = slot.submit_bgzf(good + bytes(bad) + good, capi.TEXT_FASTA, last=True)
    assert tail is None and z.corrupt == 16 and z.bad_member == 1             # kInfHeader
    # ISIZE trailers that sum beyond 2^32 - 65536: refused from the headers alone (members that claim 64 KiB of text each)
    big = E.bgzf_member(b"")[:-4] + (65536).to_bytes(4, "little")
    with pytest.raises(Exception):
        slot.submit_bgzf(big * 65540, capi.TEXT_FASTA, last=True)
    # the slot still works
    tail, info, z = slot.submit_bgzf(good + E.bgzf_member(b""), capi.TEXT_FASTA, last=True)
    assert tail == b"" and info.n_reads == 1
    slot.wait_text()
    slot.close(); clf.close()
