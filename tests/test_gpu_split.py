"""cf_batch_set_text_split / cf_batch_wait_text_split on the GPU (include/centrifuge_amd.h): a block of FASTA / FASTQ text in, the
batch's rows as text, and the reads themselves split into the four sinks — against the contract's Python statement
(tests/splitcases.py) applied to the golden rows of synth_small (the oracle's: tests/test_oracle_golden.py) and the reads of the
input file; plain and as BGZF members; the error cases; the launch record with and without a split."""
import os
import zlib

import pytest

import common
import splitcases
from centrifuge_amd import capi
from test_async_abi import dev_index

pytestmark = pytest.mark.gpu
INPUTS = [("k5", capi.TEXT_FASTA), ("fastq", capi.TEXT_FASTQ), ("pe_k5", capi.TEXT_FASTA)]


def parse_reads(text, fastq):
    """(sequence in upper case, qualities) per record of a FASTA / FASTQ file"""
    out = []
    if fastq:
        ln = text.split(b"\n")
        for i in range(0, len(ln) - 1, 4):
            out.append((ln[i + 1].upper(), ln[i + 3]))
    else:
        for rec in text.split(b">")[1:]:
            s = b"".join(rec.split(b"\n")[1:]).upper()
            out.append((s, b"I" * len(s)))
    return out


def expected(d, c, fastq):
    """the contract over the golden rows (default columns: readID first, seqID second, numMatches last) and the input's reads"""
    reads = [parse_reads(open(os.path.join(d, f), "rb").read(), fastq) for f in c["reads"]]
    rows, q, left = [], 0, 0
    for ln in open(os.path.join(d, c["tsv"]), "rb").read().split(b"\n")[1:]:
        if not ln:
            continue
        f = ln.split(b"\t")
        if left == 0:
            left = int(f[-1])
        seq, qual = reads[0][q]
        if len(reads) == 2:
            seq, qual = seq + b"_" + reads[1][q][0], qual + b"_" + reads[1][q][1]
        rows.append((f[0], seq, qual, f[1] != b"unclassified"))
        left -= 1
        if left == 0:
            q += 1
    assert q == len(reads[0])
    return splitcases.contract(rows), len(reads) == 2


def inflate_members(z):
    out, at = b"", 0
    while at < len(z):
        bsize = int.from_bytes(z[at + 16:at + 18], "little") + 1
        out += zlib.decompress(z[at:at + bsize], 31)
        at += bsize
    return out


@pytest.fixture(scope="module")
def world():
    ix = dev_index("synth_small")
    clf = capi.Classifier(ix)
    yield clf
    clf.close()


@pytest.mark.parametrize("name,tfmt", INPUTS, ids=[i[0] for i in INPUTS])
def test_sinks_are_the_contract_over_the_golden_rows(world, name, tfmt):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    want, paired = expected(d, c, tfmt == capi.TEXT_FASTQ)
    names = splitcases.SINKS_PAIRED if paired else splitcases.SINKS_UNPAIRED
    assert all(want[k] for k in names), "the case should feed every sink"
    texts = [open(os.path.join(d, f), "rb").read() for f in c["reads"]]
    golden = open(os.path.join(d, c["tsv"]), "rb").read().split(b"\n", 1)[1]
    slot = capi.Slot(world)
    slot.set_result_format(capi.RESULTS_NARROW)

    def run(sinks, bgzf):
        slot.set_text_split(sinks, bgzf)
        info = slot.submit_text(texts[0], tfmt, text2=texts[1] if paired else None)
        assert not info.irregular
        assert slot.wait_text()[0] == golden                         # the rows do not change
        return slot.wait_text_split() if sinks else None

    for sinks in (capi.SPLIT_UN | capi.SPLIT_AL, capi.SPLIT_UN, capi.SPLIT_AL):
        for bgzf in (False, True):
            got = run(sinks, bgzf)
            assert slot.wait_text_split() == got                     # a second call returns the same
            fed = 0
            for k, s in names.items():
                on = bool(sinks & (capi.SPLIT_UN if k.startswith("un") else capi.SPLIT_AL))
                data, plain, n_rec = got[s]
                if not on:
                    assert (data, plain, n_rec) == (b"", 0, 0)
                    continue
                text = inflate_members(data) if bgzf else data
                assert text == want[k], (k, sinks, bgzf, common.first_diff(text.decode("latin1"), want[k].decode("latin1")))
                assert plain == len(want[k]) and n_rec == want[k].count(b"\n") // 4
                fed |= 1 << s
            for s in range(4):
                if s not in names.values():
                    assert got[s] == (b"", 0, 0)
            assert slot.launch_record()["split_sinks"] == fed
    # a slot that never sets a split launches exactly what one with a split launches for the batch itself, and no split kernel
    # (two fresh slots, each with its first batch: a slot sizes its row workspace from the batch before, which the record shows as passes)
    def first_batch_record(sinks):
        sl = capi.Slot(world)
        sl.set_result_format(capi.RESULTS_NARROW)
        if sinks:
            sl.set_text_split(sinks)
        assert not sl.submit_text(texts[0], tfmt, text2=texts[1] if paired else None).irregular
        assert sl.wait_text()[0] == golden
        if sinks:
            sl.wait_text_split()
        return sl, sl.launch_record()
    other, with_split = first_batch_record(capi.SPLIT_UN | capi.SPLIT_AL)
    other.close()
    fresh, never = first_batch_record(0)
    assert never["split_sinks"] == 0 and with_split["split_sinks"] != 0
    assert {k: v for k, v in never.items() if k != "split_sinks"} == {k: v for k, v in with_split.items() if k != "split_sinks"}
    with pytest.raises(capi.CfError, match="no split is set"):
        fresh.wait_text_split()
    fresh.close()
    # a slot whose split is switched off again: the same
    run(0, False)
    assert slot.launch_record()["split_sinks"] == 0
    with pytest.raises(capi.CfError, match="no split is set"):
        slot.wait_text_split()
    slot.close()


def test_error_cases(world):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == "k5"][0]
    text = open(os.path.join(d, c["reads"][0]), "rb").read()
    slot = capi.Slot(world)
    with pytest.raises(capi.CfError):
        slot.set_text_split(4)
    # the slot's result format is not narrow
    slot.set_text_split(capi.SPLIT_UN | capi.SPLIT_AL)
    slot.set_result_format(capi.RESULTS_ROWS)
    with pytest.raises(capi.CfError, match="CF_RESULTS_NARROW"):
        slot.wait_text_split()
    slot.set_result_format(capi.RESULTS_NARROW)
    # no batch came as text
    with pytest.raises(capi.CfError, match="did not come as text"):
        slot.wait_text_split()
    # the batch has not been waited for as text yet
    slot.submit_text(text, capi.TEXT_FASTA)
    with pytest.raises(capi.CfError, match="has not been waited for"):
        slot.wait_text_split()
    slot.wait_text()
    assert slot.wait_text_split()[0][2] > 0
    slot.close()
