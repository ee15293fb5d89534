"""The device FASTA / FASTQ parser on the GPU over tests/textcases.py, the table the CPU harness reads (tests/test_textio_emu.py):
k_text_count, k_text_mark and k_text_records through Slot.submit_text (and submit_bgzf), k_text_pack through the plan stage, and
what they left in the slot read back by the tap cf_batch_debug_text_reads (Slot.text_reads).

* every plain case, with seeds 0 and 12345: reads, bases and longest read are the host parser's (`centrifuge-class --dump-reads`,
  the harness's oracle), and read by read the readID's bytes, the bases decoded from words and masks, the words and masks
  themselves, and the seed — which must also be cf_gen_rand_seed's (host code) for the name, codes and qualities;
* every irregular case: info.irregular carries the case's bit and is the very flags word the CPU harness returns for the block —
  from records beyond the first lane, wavefront and workgroup —, nothing is submitted; a block beyond the upload's capacity comes
  back as 1024 and nothing else; the slot then still prints the golden rows of a golden block;
* the mutated blocks: the device takes exactly those the harness takes, and their reads are the host parser's.
Nothing here reads the reference tree or oracle/_ref."""
import os

import numpy as np
import pytest

import common
import textcases as T
from centrifuge_amd import capi, reads
from emu import emu_textio as E
from test_gpu_inflate import members_of
from textcases import FASTA, FASTQ

pytestmark = pytest.mark.gpu
PLAIN = T.plain_cases()
IRREGULAR = T.irregular_cases()
CAPACITY = T.capacity_cases()
FMT = {FASTA: capi.TEXT_FASTA, FASTQ: capi.TEXT_FASTQ}
BGZF_TOO = ("trials-n70-wrap0-lower-fa", "trials-n70-wrap0-lower-fq", "pieces-4096p-mod0-fa", "pieces-4097p-mod1-fq", "counts-257-fq", "seqlines-wrap8-every-phase-fa")


@pytest.fixture(scope="module")
def ctx():
    d, _ = common.golden("synth_small")
    ix = capi.Index(os.path.join(d, "idx"), device=0)
    clf = capi.Classifier(ix)
    slot = capi.Slot(clf)
    slot.set_result_format(capi.RESULTS_NARROW)
    yield d, slot
    slot.close(); clf.close(); ix.close()


def golden_rows(d, slot):
    """the slot takes a golden block and prints the golden rows"""
    info = slot.submit_text(open(os.path.join(d, "reads.fa"), "rb").read(), capi.TEXT_FASTA)
    assert not info.irregular
    assert reads.HEADER.encode() + slot.wait_text()[0] == open(os.path.join(d, "k5.tsv"), "rb").read()


def wanted(c, seed):
    """the host parser's records of the case, mates interleaved: (name, bases, qualities, seed) per read"""
    w1 = T.host_records(c.text, c.fmt, seed)
    assert w1 is not None, c.name
    if c.text2 is None:
        return w1
    w2 = T.host_records(c.text2, c.fmt, seed)
    assert w2 is not None and len(w2) == len(w1)
    return [w[q] for q in range(len(w1)) for w in (w1, w2)]


def seed_of(name, seq, qual, fmt, seed):
    """genRandSeed through the C ABI (host code, no device)"""
    codes = np.array(["ACGTN".index(ch) for ch in seq], dtype=np.uint8)
    qa = np.frombuffer(qual, dtype=np.uint8) if fmt == FASTQ else None
    assert qa is None or len(qa) == len(codes)
    return capi.lib().cf_gen_rand_seed(codes.ctypes.data if len(codes) else None, qa.ctypes.data if qa is not None and len(qa) else None, len(codes), name, len(name), seed)


def check_batch(slot, info, whole, want, fmt, seed, own_seed=True):
    """the batch the slot holds is `want`: counts, then read by read through the tap.  whole: the slot's text buffer as the upload laid it out"""
    n = len(want)
    lens = [len(w[1]) for w in want]
    assert (info.n_reads, info.n_bases, info.max_len) == (n, sum(lens), max(lens) if lens else 0)
    rlen, seeds, id_off, id_len = slot.text_reads(n)                 # before the wait: what the record pass left
    assert rlen.tolist() == lens
    slot.wait_text()
    n_words = sum((x + 31) // 32 for x in lens)
    rlen2, seeds2, id_off2, id_len2, words, nmask = slot.text_reads(n, n_words)
    assert np.array_equal(rlen, rlen2) and np.array_equal(seeds, seeds2) and np.array_equal(id_off, id_off2) and np.array_equal(id_len, id_len2)
    assert len(words) == n_words
    seqs = E.decode(words, nmask, rlen)
    ew, em = E.encode([w[1] for w in want])
    for r, (name, seq, qual, sd) in enumerate(want):
        assert whole[int(id_off[r]):int(id_off[r]) + int(id_len[r])] == T.read_id(name), r
        assert seqs[r] == seq, r
        assert int(seeds[r]) == sd, (r, name, seq)
        if own_seed:
            assert sd == seed_of(name, seq, qual, fmt, seed), (r, name, seq)
    assert np.array_equal(words, ew) and np.array_equal(nmask, em)    # (an N's field of its word is zero)


@pytest.mark.parametrize("seed", T.SEEDS)
@pytest.mark.parametrize("c", PLAIN, ids=[c.name for c in PLAIN])
def test_a_plain_block_gives_the_host_parsers_reads(ctx, c, seed):
    d, slot = ctx
    want = wanted(c, seed)
    info = slot.submit_text(c.text, FMT[c.fmt], seed=seed, text2=c.text2)
    assert info.irregular == 0 and info.paired == (c.text2 is not None)
    whole = c.text
    if c.text2 is not None:
        whole = c.text + bytes((len(c.text) + 63) // 64 * 64 + T.PAD - len(c.text)) + c.text2
    check_batch(slot, info, whole, want, c.fmt, seed)


@pytest.mark.parametrize("name", BGZF_TOO)
def test_the_same_text_as_bgzf_members_in_two_calls(ctx, name):
    d, slot = ctx
    c = [x for x in PLAIN if x.name == name][0]
    want = wanted(c, 12345)
    mem = members_of(c.text, 4096)
    half = len(mem) // 2
    tail, info, z = slot.submit_bgzf(b"".join(mem[:half]), FMT[c.fmt], seed=12345)
    assert tail is not None and not info.irregular and not z.corrupt
    first = int(info.n_reads)
    cut = z.inflated_bytes - len(tail)
    assert c.text[cut:z.inflated_bytes] == tail and 0 < first < len(want)
    check_batch(slot, info, c.text[:cut], want[:first], c.fmt, 12345, own_seed=False)
    tail2, info, z = slot.submit_bgzf(b"".join(mem[half:]), FMT[c.fmt], head=tail, last=True, seed=12345)
    assert tail2 == b"" and not info.irregular and not z.corrupt
    check_batch(slot, info, c.text[cut:], want[first:], c.fmt, 12345, own_seed=False)


def refused(slot, c, L):
    info = slot.submit_text(c.text, FMT[c.fmt])
    assert T.carries(info.irregular, c.bit), (c.name, info.irregular, c.bit)
    total = len(c.text)
    assert info.irregular == E.flags_of(L, c.text, c.fmt, 0, T.rec_cap(total), T.pos_cap(total, c.fmt)), c.name
    assert info.n_reads == 0
    with pytest.raises(capi.CfError):
        slot.wait_text()
    with pytest.raises(capi.CfError):
        slot.text_reads(16)                                       # (no batch: the tap has nothing to show either)
    return info.irregular


@pytest.mark.parametrize("group", sorted(T.groups(IRREGULAR)))
@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_an_irregular_block_is_refused_with_the_harness_flags(ctx, fmt, group):
    d, slot = ctx
    L = E.lib()
    seen = 0
    for c in IRREGULAR:
        if c.fmt == fmt and c.group == group:
            seen |= refused(slot, c, L)
    if group == "placed":                                          # every reason bit of the format, from records beyond the first workgroup
        assert seen & 0x7ff == (0x3f if fmt == FASTA else 0x3ff), hex(seen)
    golden_rows(d, slot)


@pytest.mark.parametrize("c", CAPACITY, ids=[c.name for c in CAPACITY])
def test_a_block_beyond_the_capacity_is_too_many_and_nothing_else(ctx, c):
    d, slot = ctx
    assert refused(slot, c, E.lib()) == T.TOO_MANY == 1024
    golden_rows(d, slot)


def test_the_tap_refuses_a_batch_that_did_not_come_as_text(ctx):
    d, slot = ctx
    names, qlens, seq, off, seeds, paired = reads.load([os.path.join(d, "reads.fa")], False)
    b, m, ln = capi.pack_reads(seq, off)
    ni, nk = capi.sparse_nmask(m)
    slot.submit(b, None, ln, np.ascontiguousarray(seeds, dtype=np.uint32), nwords=(ni, nk))
    slot.wait_narrow()
    with pytest.raises(capi.CfError):
        slot.text_reads(len(names))
    info = slot.submit_text(b">a\nACGT\n", capi.TEXT_FASTA)
    assert not info.irregular
    with pytest.raises(capi.CfError):
        slot.text_reads(1, 1)                                     # the words are the plan stage's: not before the wait
    with pytest.raises(capi.CfError):
        slot.text_reads(0)                                        # arrays too small
    assert slot.text_reads(1)[0].tolist() == [4]
    slot.wait_text()
    golden_rows(d, slot)


@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_the_device_takes_the_mutated_blocks_the_harness_takes(ctx, fmt):
    d, slot = ctx
    L = E.lib()
    taken = 0
    for trial, text in enumerate(T.mutated(fmt)):
        info = slot.submit_text(text, FMT[fmt])
        assert info.irregular == E.flags_of(L, text, fmt), (trial, text)
        if info.irregular:
            continue
        taken += 1
        want = T.host_records(text, fmt)
        assert want is not None, (trial, text)
        check_batch(slot, info, text, want, fmt, 0)
    assert taken >= 10
    golden_rows(d, slot)
