"""centrifuge-class over tabbed files (--tab5 / --12 / --tab6) on the device text path: synth_small's reads as three-field lines, as
tab5 and tab6 pair lines and as a file that mixes both, plain and BGZF, in blocks of 4096 and 20000 bytes, against the REFERENCE
binary's recorded TSV and report for the same reads (tests/golden/tab_reads.tar.xz; tests/tabcases.py says by which command lines
the reference can read them) and against the same command with --host-io; the plain inputs are parsed and printed on the device
block by block, the mixed file on both sides.  Without the feature every run ends with "unrecognized option"."""
import os
import subprocess
import tempfile

import pytest

import common
import tabcases as T
from test_gpu_cli_bgzf import members, write_bgzf
from test_gpu_cli_text import CLI, blocks, run

pytestmark = pytest.mark.gpu
SMALL = {"CF_TEXT_BLOCK": "4096"}
HOST_SMALL = {"CF_DEBUG_KNOBS": "1", "CF_INGEST_BLOCK": "4096"}


def golden_case(inp, lst, sam):
    d, g = common.golden("tab_reads")
    c = [x for x in g["cases"] if x["name"] == T.case_name(inp, lst, sam)][0]
    return open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()


@pytest.mark.parametrize("lst,args", T.ARG_LISTS, ids=[a[0] for a in T.ARG_LISTS])
@pytest.mark.parametrize("inp", T.INPUTS + [i + ".gz" for i in T.INPUTS])
def test_tabbed_reads_take_the_text_path_and_print_what_the_reference_prints(inp, lst, args):
    d, _ = common.golden("synth_small")
    gz, inp = inp.endswith(".gz"), inp.split(".")[0]
    se, pe = T.records(d, T.MIN_LONG if "-5" in args else 0)
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, inp + ".tab")
        open(p, "wb").write(T.text_of(inp, se, pe))
        if gz:
            p = write_bgzf(p + ".gz", T.text_of(inp, se, pe))
        cmd = ["-t", "-p", "4", "-x", os.path.join(d, "idx"), T.flag_of(inp), p] + args
        for sam in (False, True):
            want = golden_case(inp, lst, sam)
            extra = ["--out-fmt", "sam"] if sam else []
            tsv, rep, err = run(cmd + extra, t, env=SMALL)
            assert tsv == want[0], common.first_diff(tsv.decode("latin1"), want[0].decode("latin1"))
            assert rep == want[1]
            nb = blocks(err)
            assert nb and nb[0] > 0 and nb[1] == 0, err
            if gz:
                assert members(err)[0] > 0 and members(err)[1] == 0, err
        host = run(cmd + extra + ["--host-io", "--batch", "64"], t, env=HOST_SMALL, tag="h")
        assert host[:2] == want and blocks(host[2]) is None
        again = run(cmd + extra, t, env={"CF_TEXT_BLOCK": "20000"}, tag="b")
        assert again[:2] == want and blocks(again[2])[0] > 0 and blocks(again[2])[1] == 0
        if inp != "pe6":
            assert run(["--12" if a == "--tab5" else a for a in cmd] + extra, t, env=SMALL)[:2] == want


@pytest.mark.parametrize("lst,args", T.ARG_LISTS, ids=[a[0] for a in T.ARG_LISTS])
def test_a_file_that_mixes_pairs_and_unpaired_reads_comes_out_in_file_order(lst, args):
    """runs of 7 pair lines and 5 three-field lines: the blocks that hold one kind are parsed on the device, those with both on the
    host; the rows are the recorded ones read by read (plain list), and TSV and report equal the host threads' for every list"""
    d, _ = common.golden("synth_small")
    se, pe = T.records(d, T.MIN_LONG if "-5" in args else 0)
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "mix.tab")
        open(p, "wb").write(T.text_of("mix", se, pe))
        cmd = ["-t", "-p", "4", "-x", os.path.join(d, "idx"), "--tab5", p] + args
        for extra in ([], ["--out-fmt", "sam"]):
            tsv, rep, err = run(cmd + extra, t, env={"CF_TEXT_BLOCK": "4096"})
            host = run(cmd + extra + ["--host-io", "--batch", "3"], t, env=HOST_SMALL, tag="h")
            assert (tsv, rep) == host[:2], common.first_diff(tsv.decode("latin1"), host[0].decode("latin1"))
            # (-s 13 -u 40 prints records 13 .. 52 only: the first blocks, every one of which holds lines of both kinds)
            nb = blocks(err)
            assert "-u" in args or (nb and nb[0] > 0 and nb[1] > 0), err
        if lst == "plain":
            se_tsv, pe_tsv = golden_case("se", "plain", False)[0], golden_case("pe5", "plain", False)[0]
            want = T.mix_rows(se_tsv.split(b"\n")[0], se, pe, se_tsv, pe_tsv)
            tsv = run(cmd, t, env={"CF_TEXT_BLOCK": "4096"})[0]
            assert tsv == want, common.first_diff(tsv.decode("latin1"), want.decode("latin1"))


def test_a_quality_string_one_short_ends_the_run_with_the_references_message():
    d, _ = common.golden("synth_small")
    g = common.golden("tab_reads")[1]["bad_qual"]
    se, pe = T.records(d)
    bad = T.text_of("se", se, pe).split(b"\n")
    f = bad[1].split(b"\t")
    bad[1] = b"\t".join([f[0], f[1], f[2][:-1]])
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "bad.tab")
        open(p, "wb").write(b"\n".join(bad))
        r = subprocess.run([CLI, "-x", os.path.join(d, "idx"), "--tab5", p, "-S", os.path.join(t, "o.tsv"), "--report-file", os.path.join(t, "o.rep")], capture_output=True, timeout=120)
        assert r.returncode == g["returncode"] and g["stderr"].encode() in r.stderr, r.stderr
