"""cf_batch_wait_text_bgzf on the GPU (include/centrifuge_amd.h): the rows of a batch as BGZF members deflated on the device — they
inflate to what cf_batch_wait_text returns for the same block, with the same tuples and counters, and they are byte for byte the
members the CPU harness (tests/emu/emu_deflate.cpp) makes of that text."""
import gzip
import os

import numpy as np
import pytest

import common
from centrifuge_amd import capi
from emu import emu_deflate as D
from emu import emu_inflate as I
from test_async_abi import dev_index

pytestmark = pytest.mark.gpu
INPUTS = [("k5", capi.TEXT_FASTA), ("fastq", capi.TEXT_FASTQ), ("pe_k5", capi.TEXT_FASTA)]
COLS = "readID,taxID,taxName,readSeq,readQual"


def tuple_records(words):
    """the tuple list (n, then n taxon indices, ...) as its records, sorted: the format pass appends them through an atomic counter,
    so their order in the list is not the same from one run of the same batch to the next"""
    out, i = [], 0
    while i < len(words):
        n = int(words[i])
        out.append(tuple(int(x) for x in words[i + 1:i + 1 + n]))
        i += n + 1
    assert i == len(words)
    return sorted(out)


def both_forms(texts, tfmt, cols=None, member=4096):
    """the block on two slots, one waited for as text, the other as BGZF members -> text, members"""
    ix = dev_index("synth_small")
    clf = capi.Classifier(ix)
    got = []
    for bgzf in (False, True):
        slot = capi.Slot(clf)
        slot.set_result_format(capi.RESULTS_NARROW)
        if cols:
            slot.set_text_columns(cols.split(","))
        clf.reset_counts()
        info = slot.submit_text(texts[0], tfmt, text2=texts[1] if len(texts) == 2 else None)
        assert not info.irregular
        if bgzf:
            members, text_bytes, tuples, res = slot.wait_text_bgzf()
            again = slot.wait_text_bgzf()
            assert again[0] == members and again[1] == text_bytes and np.array_equal(again[2], tuples) and again[3] == res     # a second wait: the same bytes
            with pytest.raises(capi.CfError) as e:
                slot.wait_text()
            assert "cf_batch_wait_text_bgzf" in str(e.value)
            assert slot.deflate_ms() > 0                  # (HIP events around the deflate kernel)
            got.append((members, text_bytes, tuples, res, clf.counts(), clf.counts_single()))
        else:
            text, tuples, res = slot.wait_text()
            with pytest.raises(capi.CfError) as e:
                slot.wait_text_bgzf()
            assert "cf_batch_wait_text" in str(e.value)
            got.append((text, len(text), tuples, res, clf.counts(), clf.counts_single()))
        slot.close()
    clf.close()
    (text, n, tup_a, res_a, cnt_a, single_a), (members, text_bytes, tup_b, res_b, cnt_b, single_b) = got
    assert text_bytes == n and gzip.decompress(members + capi.bgzf_eof()) == text
    assert tuple_records(tup_a) == tuple_records(tup_b) and len(tup_a) == len(tup_b) and res_a == res_b
    assert all(np.array_equal(x, y) for x, y in zip(cnt_a, cnt_b)) and np.array_equal(single_a, single_b)
    table, n_out = I.member_table(members)
    assert n_out == n and len(table) == (n + member - 1) // member
    assert members == D.deflate(text, member)[0]          # the device's members are the harness's
    return text, members


def golden_texts(name):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    return [open(os.path.join(d, f), "rb").read() for f in c["reads"]], open(os.path.join(d, c["tsv"]), "rb").read().split(b"\n", 1)[1]


@pytest.mark.parametrize("name,tfmt", INPUTS, ids=[i[0] for i in INPUTS])
def test_members_inflate_to_the_text_and_equal_the_harness(name, tfmt, monkeypatch):
    monkeypatch.setenv("CF_BGZF_OUT_MEMBER", "4096")
    texts, rows = golden_texts(name)
    text, members = both_forms(texts, tfmt)
    assert text == rows and len(members) < len(text)
    assert len(I.member_table(members)[0]) >= 4


@pytest.mark.parametrize("name,tfmt", INPUTS, ids=[i[0] for i in INPUTS])
def test_with_a_column_program(name, tfmt, monkeypatch):
    monkeypatch.setenv("CF_BGZF_OUT_MEMBER", "4096")
    texts, _ = golden_texts(name)
    text, _ = both_forms(texts, tfmt, cols=COLS)
    assert text.count(b"\t") == 4 * text.count(b"\n")


def test_a_block_of_no_reads_gives_no_member(monkeypatch):
    monkeypatch.setenv("CF_BGZF_OUT_MEMBER", "4096")
    texts, _ = golden_texts("k5")
    ix = dev_index("synth_small")
    clf = capi.Classifier(ix)
    slot = capi.Slot(clf)
    slot.set_result_format(capi.RESULTS_NARROW)
    slot.set_text_skip(10 ** 9)                            # beyond the block
    info = slot.submit_text(texts[0], capi.TEXT_FASTA)
    assert not info.irregular and info.n_reads == 0
    members, text_bytes, tuples, res = slot.wait_text_bgzf()
    assert members == b"" and text_bytes == 0 and len(tuples) == 0 and res["n_queries"] == 0
    assert slot.wait_text_bgzf()[0] == b"" and slot.deflate_ms() == 0
    slot.close(); clf.close()


def test_the_default_member_size_and_more_than_one_member():
    """the golden reads again and again under new names, until their rows outgrow a member of 65,280 bytes"""
    texts, _ = golden_texts("k5")
    recs = texts[0].split(b"\n>")
    recs = [recs[0][1:]] + recs[1:]
    block = b"".join(b">c%d_" % k + r.rstrip(b"\n") + b"\n" for k in range(2) for r in recs)
    text, members = both_forms([block], capi.TEXT_FASTA, member=D.MEMBER)
    table, _ = I.member_table(members)
    assert len(text) > D.MEMBER and len(table) == (len(text) + D.MEMBER - 1) // D.MEMBER and int(table[0][3]) == D.MEMBER
