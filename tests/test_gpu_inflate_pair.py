"""The BGZF files of mates through the batch ABI on the GPU (cf_batch_upload_bgzf_pair: include/centrifuge_amd.h): r1.fa / r2.fa of
synth_small as BGZF members made here with zlib, uploaded in runs whose lengths differ between the two files, the two tails handed
on; the device cuts both texts of a call behind a common record.  The reads that come out and the rows printed for them are those
of the plain files through cf_batch_upload_text (text, text2), and the reference's golden TSV.  Corrupt members — in the CPU
harness (tests/test_inflate_emu.py) and, through this entry and the inflater's tap, on the GPU — are tests/test_gpu_codec.py's."""
import os

import numpy as np
import pytest

import common
from centrifuge_amd import capi, reads
from emu import emu_inflate as E
from test_gpu_inflate import members_of, slot_for

pytestmark = pytest.mark.gpu
HEADER = reads.HEADER.encode()
_plain = {}


def mates(fastq):
    """the two files' texts; FASTQ: the FASTA records with seeded random qualities"""
    d, _ = common.golden("synth_small")
    m1, m2 = (open(os.path.join(d, f), "rb").read() for f in ("r1.fa", "r2.fa"))
    if not fastq:
        return m1, m2

    def fq(src, seed):
        rng = np.random.default_rng(seed)
        out = []
        for r in src[1:].split(b"\n>"):
            name, seq = r.split(b"\n")[:2]
            out.append(b"@" + name + b"\n" + seq + b"\n+\n" + bytes(int(q) for q in rng.integers(33, 127, len(seq))) + b"\n")
        return b"".join(out)
    return fq(m1, 1), fq(m2, 2)


def plain(fastq):
    """what cf_batch_upload_text makes of the whole plain files: the texts, its info and printed rows (made once)"""
    if fastq not in _plain:
        t1, t2 = mates(fastq)
        clf, slot = slot_for()
        info = slot.submit_text(t1, capi.TEXT_FASTQ if fastq else capi.TEXT_FASTA, text2=t2)
        assert not info.irregular and info.paired == 1
        _plain[fastq] = (t1, t2, (info.n_reads, info.n_bases, info.max_len), slot.wait_text()[0])
        slot.close(); clf.close()
    return _plain[fastq]


def test_the_library_exports_the_pair_upload():
    assert "cf_batch_upload_bgzf_pair" in capi.EXPORTS and hasattr(capi.lib(), "cf_batch_upload_bgzf_pair")
    assert hasattr(capi.Slot, "submit_bgzf_pair")


def through_pair(t1, t2, fmt, size, run1, run2):
    """-> reads, bases, longest read, the rows' text, the calls"""
    mem1, mem2 = members_of(t1, size), members_of(t2, size)
    run1, run2 = run1 or len(mem1), run2 or len(mem2)
    clf, slot = slot_for()
    tail1, tail2, out, n_reads, n_bases, max_len, inflated, calls = b"", b"", b"", 0, 0, 0, [0, 0], 0
    while calls * run1 < len(mem1) or calls * run2 < len(mem2):
        a, b = mem1[calls * run1:(calls + 1) * run1], mem2[calls * run2:(calls + 1) * run2]
        last1, last2 = (calls + 1) * run1 >= len(mem1), (calls + 1) * run2 >= len(mem2)
        tail1, tail2, info, z1, z2 = slot.submit_bgzf_pair(b"".join(a), b"".join(b), fmt, head1=tail1, head2=tail2, last1=last1, last2=last2)
        assert tail1 is not None and not info.irregular and not z1.corrupt and not z2.corrupt, (calls, info.irregular, z1.corrupt, z2.corrupt)
        inflated[0] += z1.inflated_bytes; inflated[1] += z2.inflated_bytes
        assert info.n_reads % 2 == 0 and info.paired == 1
        n_reads += info.n_reads; n_bases += info.n_bases; max_len = max(max_len, info.max_len)
        text = slot.wait_text()[0]
        if info.n_reads:
            out += text
        calls += 1
    assert (tail1, tail2) == (b"", b"") and inflated == [len(t1), len(t2)]
    slot.close(); clf.close()
    return n_reads, n_bases, max_len, out, calls


@pytest.mark.parametrize("runs", [(1, 1), (3, 2), (0, 0)])
@pytest.mark.parametrize("size", [700, 65280])
@pytest.mark.parametrize("fastq", [False, True])
def test_runs_of_different_lengths_give_the_pairs_and_rows_of_the_plain_files(fastq, size, runs):
    t1, t2, info, rows = plain(fastq)
    n_reads, n_bases, max_len, out, calls = through_pair(t1, t2, capi.TEXT_FASTQ if fastq else capi.TEXT_FASTA, size, *runs)
    assert (n_reads, n_bases, max_len) == info
    assert out == rows
    if size == 700 and runs == (3, 2):
        assert calls > 40                                     # (the first file ran out of members long before the second)
    if not fastq:
        d, cases = common.golden("synth_small")
        want = open(os.path.join(d, [c for c in cases if c["name"] == "pe_k5"][0]["tsv"]), "rb").read()
        assert HEADER + out == want, common.first_diff((HEADER + out).decode("latin1"), want.decode("latin1"))


def test_members_of_the_first_file_only_and_max_reads():
    t1, t2, info, rows = plain(False)
    clf, slot = slot_for()
    # no member of the second file yet: no pair is whole, the first file's text comes back as its tail
    some = t1[:t1.index(b">", 20000)]
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(b"".join(members_of(some, 700)), b"", capi.TEXT_FASTA)
    assert i.n_reads == 0 and not i.irregular and i.paired == 1 and (tail1, tail2) == (some, b"") and z1.inflated_bytes == len(some) and z2.inflated_bytes == 0
    slot.wait_text()
    # ... and goes in as the next call's head, with the rest of both files
    rest = b"".join(members_of(t1[len(some):], 700))
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(rest, b"".join(members_of(t2, 65280)), capi.TEXT_FASTA, head1=tail1, last1=True, last2=True)
    assert (i.n_reads, i.n_bases, i.max_len) == info and i.paired == 1 and (tail1, tail2) == (b"", b"")
    assert slot.wait_text()[0] == rows
    # max_reads counts pairs and ends inside the run
    want = slot.submit_text(t1, capi.TEXT_FASTA, text2=t2, max_reads=37)
    want_rows = slot.wait_text()[0]
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(b"".join(members_of(t1, 700)), b"".join(members_of(t2, 700)), capi.TEXT_FASTA, last1=True, last2=True, max_reads=37)
    assert i.n_reads == 74 == want.n_reads and i.paired == 1 == want.paired and (tail1, tail2) == (b"", b"")
    assert slot.wait_text()[0] == want_rows and rows.startswith(want_rows)
    slot.close(); clf.close()


def test_refusals_leave_no_batch_and_a_usable_slot():
    t1, t2, info, rows = plain(False)
    clf, slot = slot_for()
    m1 = b"".join(members_of(t1, 700))
    # both files end and the second one is three records short: CF_TEXT_MATE_COUNT
    short = t2[:t2.rindex(b">", 0, t2.rindex(b">", 0, t2.rindex(b">")))]
    assert short.count(b">") == t2.count(b">") - 3
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(m1, b"".join(members_of(short, 700)), capi.TEXT_FASTA, last1=True, last2=True)
    assert tail1 is None and tail2 is None and i.irregular & 2048 and not z1.corrupt and not z2.corrupt
    # ... with more to follow in the second file, the first one's three records are its tail
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(m1, b"".join(members_of(short, 700)), capi.TEXT_FASTA, last1=True, last2=False)
    assert not i.irregular and i.paired == 1 and i.n_reads == 2 * (t2.count(b">") - 4) and tail1.count(b">") == 4 and tail2.count(b">") == 1 and t1.endswith(tail1)
    slot.wait_text()
    # the first file brings 1.2 MB more text than the second in one call: more than the room its tail has (CF_TEXT_TAIL_ROOM)
    big = t1 * 20
    assert len(big) - len(t2) > 1200000
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(b"".join(members_of(big, 65280)), b"".join(members_of(t2, 65280)), capi.TEXT_FASTA)
    assert tail1 is None and i.irregular & 4096 and not z1.corrupt and not z2.corrupt
    # a second mate of another format
    with pytest.raises(capi.CfError):
        slot.submit_bgzf_pair(m1, b"".join(members_of(t2, 700)), capi.TEXT_FASTA, last1=True, last2=True, fmt2=capi.TEXT_FASTQ)
    # a header that is not BGZF's is reported in the file it belongs to (found by the host: no kernel sees it)
    good = E.bgzf_member(b">r\nACGT\n")
    bad = bytearray(good); bad[12] = ord("X")
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(good, good + bytes(bad), capi.TEXT_FASTA, last1=True, last2=True)
    assert tail1 is None and (z1.corrupt, z2.corrupt, z2.bad_member) == (0, 16, 1)
    # the slot still works
    tail1, tail2, i, z1, z2 = slot.submit_bgzf_pair(m1, b"".join(members_of(t2, 65280)), capi.TEXT_FASTA, last1=True, last2=True)
    assert (tail1, tail2) == (b"", b"") and (i.n_reads, i.n_bases, i.max_len) == info and i.paired == 1
    assert slot.wait_text()[0] == rows
    slot.close(); clf.close()
