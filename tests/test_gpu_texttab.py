"""Tabbed blocks through the batch ABI (capi: Slot.submit_text / submit_bgzf with TEXT_TAB5 / TEXT_TAB6, wait_text) on the device:
the text that comes back equals the reference's recorded TSV for the same reads (tests/golden/tab_reads.tar.xz, which the host
path prints too: tests/test_gpu_cli_tab.py), TextInfo.paired says what the block held, the device refuses what is not in the
plain form with the bit the CPU harness expects, and the calls that make no sense for these formats are CF_ERR_ARG."""
import os

import pytest

import common
import tabcases as T
from centrifuge_amd import capi, reads
from test_gpu_cli_bgzf import bgzf as bgzf_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    d, _ = common.golden("synth_small")
    ix = capi.Index(os.path.join(d, "idx"), device=0)
    clf = capi.Classifier(ix)
    slot = capi.Slot(clf)
    slot.set_result_format(capi.RESULTS_NARROW)
    se, pe = T.records(d)
    yield d, slot, se, pe
    slot.close(); clf.close(); ix.close()


def want_tsv(inp):
    d, g = common.golden("tab_reads")
    c = [x for x in g["cases"] if x["name"] == T.case_name(inp, "plain", False)][0]
    return open(os.path.join(d, c["tsv"]), "rb").read()


@pytest.mark.parametrize("inp", T.INPUTS)
def test_text_and_bgzf_uploads_print_the_recorded_rows_and_report_the_pair_flag(ctx, inp):
    d, slot, se, pe = ctx
    text = T.text_of(inp, se, pe)
    fmt = capi.TEXT_TAB6 if inp == "pe6" else capi.TEXT_TAB5
    n = text.count(b"\n")
    info = slot.submit_text(text, fmt)
    assert not info.irregular and info.paired == (inp != "se") and info.n_reads == n * (2 if inp != "se" else 1)
    assert reads.HEADER.encode() + slot.wait_text()[0] == want_tsv(inp)
    # the same text as BGZF members, cut in mid-line: the tail is the unfinished line
    cut = len(text) // 2 + 7
    tail, info, z = slot.submit_bgzf(bgzf_bytes(text[:cut]), fmt)
    assert tail is not None and not info.irregular and tail == text[text.rindex(b"\n", 0, cut) + 1:cut] and info.paired == (inp != "se")
    first = slot.wait_text()[0]
    tail2, info, z = slot.submit_bgzf(bgzf_bytes(text[cut:]), fmt, head=tail, last=True)
    assert tail2 == b"" and not info.irregular
    assert reads.HEADER.encode() + first + slot.wait_text()[0] == want_tsv(inp)


def test_refusals_and_argument_errors(ctx):
    d, slot, se, pe = ctx
    ok5, ok3 = b"n\tACGT\tIIII\tGGCC\tJJJJ\n", b"m\tACGT\tIIII\n"
    for text, bit in [(ok5 + ok3, 8192), (ok5 + ok5[:-1], 512), (ok5 + b"n\tACGT\tIIII\tGGCC\n", 512), (ok5 + b"n\tACGT\tIII\tGGCC\tJJJJ\n", 128),
                      (ok5 + b"n\tACGT\tII I\tGGCC\tJJJJ\n", 256), (ok5 + b"n\r\tACGT\tIIII\tGGCC\tJJJJ\n", 8), (ok5 + b"n\tACXT\tIIII\tGGCC\tJJJJ\n", 16),
                      (ok5 + b"\tACGT\tIIII\tGGCC\tJJJJ\n", 4), (ok5 + b"n\t\t\tGGCC\tJJJJ\n", 32)]:
        assert slot.submit_text(text, capi.TEXT_TAB5).irregular == bit, text
    with pytest.raises(Exception) as e:
        slot.submit_text(ok5, capi.TEXT_TAB5, text2=ok5)
    assert "argument" in str(e.value).lower() or "text2" in str(e.value)
    with pytest.raises(Exception) as e:
        slot.submit_bgzf_pair(bgzf_bytes(ok5), bgzf_bytes(ok5), capi.TEXT_TAB5, last1=True, last2=True)
    assert "argument" in str(e.value).lower() or "format" in str(e.value)
