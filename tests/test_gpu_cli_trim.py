"""centrifuge-class with -5 / -3 / -s / -u over the device text path: plain FASTQ and FASTA files, plain mates and a bgzipped FASTQ
file in blocks of 4096 bytes — so that the skip and the -u limit land inside a block, at a block's edge and past one —, against
the REFERENCE binary's recorded TSV and report (tests/golden/trim_skip.tar.xz), against the same command with --host-io, and with
every block parsed and printed on the device.  (Without the feature such a run never takes the text path: the block counts fail.)"""
import os
import tempfile

import pytest

import common
import trimcases as T
from test_gpu_cli_bgzf import members, write_bgzf
from test_gpu_cli_text import blocks, run

pytestmark = pytest.mark.gpu
SMALL = {"CF_TEXT_BLOCK": "4096"}


def golden_case(inp, lst):
    d, g = common.golden("trim_skip")
    c = [x for x in g["cases"] if x["name"] == T.case_name(inp, lst, False)][0]
    return open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()


@pytest.mark.parametrize("lst,args", T.ARG_LISTS, ids=[a[0] for a in T.ARG_LISTS])
@pytest.mark.parametrize("inp", ["fq", "fa", "pe", "fq.gz"])
def test_trim_and_skip_take_the_text_path_and_print_what_the_reference_prints(inp, lst, args):
    d, _ = common.golden("synth_small")
    want = golden_case(inp.split(".")[0], lst)
    with tempfile.TemporaryDirectory() as t:
        fmt, files = T.files_of(d, inp.split(".")[0], args, t)
        if inp == "fq.gz":
            files = [write_bgzf(os.path.join(t, "reads.fq.gz"), open(files[0], "rb").read())]
        reads = ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
        cmd = [fmt, "-t", "-p", "4", "-x", os.path.join(d, "idx")] + reads + args
        tsv, rep, err = run(cmd, t, env=SMALL)
        assert tsv == want[0], common.first_diff(tsv.decode("latin1"), want[0].decode("latin1"))
        assert rep == want[1]
        host = run(cmd + ["--host-io"], t, tag="h")
        assert (tsv, rep) == host[:2] and blocks(host[2]) is None
        nb = blocks(err)
        assert nb and nb[0] > 0 and nb[1] == 0, err
        if inp == "fq.gz":
            assert members(err)[0] > 0 and members(err)[1] == 0, err
        # ... and whatever the size of the blocks
        again = run(cmd, t, env={"CF_TEXT_BLOCK": "20000"}, tag="b")
        assert again[:2] == (tsv, rep) and blocks(again[2])[0] > 0 and blocks(again[2])[1] == 0


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_reads_the_trims_leave_nothing_of_take_their_blocks_to_the_host(fastq):
    """a few 12-base reads among 100-base ones and -5 10 -3 5: empty reads are the host parser's, so the blocks that hold the short
    reads are parsed there, the others on the device — and the run prints what the host threads print"""
    d, _ = common.golden("synth_small")
    src = open(os.path.join(d, "reads.fq"), "rb").read().split(b"\n")[:-1]
    out = []
    for i in range(0, len(src), 4):
        name, seq, qual = src[i][1:], src[i + 1], src[i + 3]
        if (i // 4) % 60 == 17:
            seq, qual = seq[:12], qual[:12]
        out.append(b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n" if fastq else b">" + name + b"\n" + seq + b"\n")
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "short.fq" if fastq else "short.fa")
        open(p, "wb").write(b"".join(out))
        for extra in ([], ["-s", "13", "-u", "40"]):
            cmd = ["-q" if fastq else "-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", p, "-5", "10", "-3", "5"] + extra
            tsv, rep, err = run(cmd, t, env=SMALL)
            host = run(cmd + ["--host-io"], t, tag="h")
            assert (tsv, rep) == host[:2], common.first_diff(tsv.decode("latin1"), host[0].decode("latin1"))
            nb = blocks(err)
            assert nb and nb[0] > 0 and nb[1] > 0, err
