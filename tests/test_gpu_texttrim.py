"""cf_batch_set_text_trim / cf_batch_set_text_skip on the GPU (include/centrifuge_amd.h), through capi: synth_small's reads go up as
text — a plain block, BGZF members, the BGZF members of two mate files — with the slot's trim and skip set, and the text that
cf_batch_wait_text returns is what the REFERENCE binary printed for -5 / -3 / -s / -u over the same reads
(tests/golden/trim_skip.tar.xz), for the default columns and for --out-fmt sam's list, whose SEQ and QUAL show the window."""
import os

import pytest

import common
import trimcases as T
from centrifuge_amd import capi
from test_gpu_inflate import members_of, slot_for

pytestmark = pytest.mark.gpu


def test_the_library_exports_the_setters():
    for f in ("cf_batch_set_text_trim", "cf_batch_set_text_skip"):
        assert hasattr(capi.lib(), f)
    assert hasattr(capi.Slot, "set_text_trim") and hasattr(capi.Slot, "set_text_skip")


def options(args):
    o = {"-5": 0, "-3": 0, "-s": 0, "-u": 0}
    for k, v in zip(args[::2], args[1::2]):
        o[k] = int(v)
    return o["-5"], o["-3"], o["-s"], o["-u"]


def texts_of(inp, args):
    d, _ = common.golden("synth_small")
    texts = [open(os.path.join(d, f), "rb").read() for f in T.INPUTS[inp][1]]
    if inp == "fa" and "-5" in args:
        texts = [T.long_fasta(texts[0])]
    return texts


def golden_rows(inp, lst, sam):
    d, g = common.golden("trim_skip")
    c = [x for x in g["cases"] if x["name"] == T.case_name(inp, lst, sam)][0]
    text = open(os.path.join(d, c["tsv"]), "rb").read()
    return text if sam else text.split(b"\n", 1)[1]                 # (no header line under --out-fmt sam)


def in_calls(slot, submit, calls, per, skip, upto):
    """the calls of one file (or one pair of files) the way a front end makes them: each call once as it is for its record count,
    then — where -s or -u ends inside it — once more with the slot's skip and max_reads; submit(call, tails, max_reads) -> info,
    the tails to hand to the next call.  -> the text of all of them"""
    base, out, tails = 0, b"", None
    limit = skip + upto if upto else 1 << 62
    for k, call in enumerate(calls):
        slot.set_text_skip(0)
        info, after = submit(call, tails, 0)
        assert not info.irregular
        rows = slot.wait_text()[0]
        n = info.n_reads // per
        drop = 0 if base >= skip else min(n, skip - base)
        up_to = 0 if base >= limit else min(n, limit - base)
        take = max(0, up_to - drop)
        if take and take < n:
            slot.set_text_skip(drop)
            info, again = submit(call, tails, take if up_to < n else 0)
            assert not info.irregular and info.n_reads == take * per
            assert again == after                                    # (the cut and the tails depend on neither the trim nor the skip)
            rows = slot.wait_text()[0]
        if take:
            out += rows
        base += n
        tails = after
        assert any(tails) == (k + 1 < len(calls))                    # (a tail crosses the calls; nothing is left at the end)
    slot.set_text_skip(0)
    return out


@pytest.mark.parametrize("lst,args", T.ARG_LISTS, ids=[a[0] for a in T.ARG_LISTS])
@pytest.mark.parametrize("inp", list(T.INPUTS))
def test_trimmed_and_skipped_uploads_print_what_the_reference_prints(inp, lst, args):
    t5, t3, skip, upto = options(args)
    texts = texts_of(inp, args)
    fmt = capi.TEXT_FASTQ if inp == "fq" else capi.TEXT_FASTA
    clf, slot = slot_for()
    slot.set_text_trim(t5, t3)
    mem = [members_of(t, 700) for t in texts]
    if len(texts) == 1:
        half = len(mem[0]) // 2
        calls = [(mem[0][:half], False), (mem[0][half:], True)]

        def submit(call, tails, max_reads):
            tail, info, z = slot.submit_bgzf(b"".join(call[0]), fmt, head=tails[0] if tails else b"", last=call[1], max_reads=max_reads)
            assert tail is not None and not z.corrupt
            return info, (tail,)
    else:
        h1, h2 = len(mem[0]) // 2, len(mem[1]) // 3
        calls = [(mem[0][:h1], mem[1][:h2], False), (mem[0][h1:], mem[1][h2:], True)]

        def submit(call, tails, max_reads):
            t1, t2, info, z1, z2 = slot.submit_bgzf_pair(b"".join(call[0]), b"".join(call[1]), fmt, head1=tails[0] if tails else b"",
                                                         head2=tails[1] if tails else b"", last1=call[2], last2=call[2], max_reads=max_reads)
            assert t1 is not None and not z1.corrupt and not z2.corrupt
            return info, (t1, t2)
    for sam in (False, True):
        slot.set_text_columns(T.SAM.split(",") if sam else [])
        want = golden_rows(inp, lst, sam)
        # the plain upload: one block, the skip and max_reads straight from the options
        slot.set_text_skip(skip)
        info = slot.submit_text(texts[0], fmt, max_reads=upto, text2=texts[1] if len(texts) == 2 else None)
        assert not info.irregular
        got = slot.wait_text()[0]
        assert got == want, (sam, common.first_diff(got.decode("latin1"), want.decode("latin1")))
        # BGZF members (of both mate files) in two calls, so that a tail crosses from the first into the second
        got = in_calls(slot, submit, calls, len(texts), skip, upto)
        assert got == want, (sam, "bgzf", common.first_diff(got.decode("latin1"), want.decode("latin1")))
    slot.close(); clf.close()
