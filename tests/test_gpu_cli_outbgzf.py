"""centrifuge-class --out-bgzf: the classification output (-S or stdout) is one BGZF file — header line, rows, --separator markers,
the SAM form — that inflates to exactly the bytes the same command prints without the flag, whichever way the rows were made: on
the device text path (deflated on the device, cf_batch_wait_text_bgzf) or by host threads (zlib); the report stays as it is."""
import gzip
import os
import subprocess
import tempfile

import pytest

import common
import tabcases as T
from emu import emu_inflate as I
from test_gpu_cli_bgzf import write_bgzf
import re

from test_gpu_cli_text import CLI, blocks, run

pytestmark = pytest.mark.gpu
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SMALL = {"CF_BGZF_OUT_MEMBER": "4096"}


def inflated(z):
    """a BGZF file's text; every member parses, the file ends with the EOF member"""
    assert z.endswith(EOF)
    table, n = I.member_table(z)
    assert len(table) >= 2 and int(table[-1][3]) == 0 and all(int(r[3]) <= 65280 for r in table)
    text = gzip.decompress(z)
    assert len(text) == n
    return text


def golden_case(name):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    return d, c, open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()


@pytest.mark.parametrize("name,fmt", [("k5", "-f"), ("fastq", "-q"), ("pe_k5", "-f")])
def test_golden_cases_inflate_to_the_golden_tsv(name, fmt):
    d, c, tsv, rep = golden_case(name)
    files = [os.path.join(d, f) for f in c["reads"]]
    reads = ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
    with tempfile.TemporaryDirectory() as t:
        for env in ({}, SMALL):
            z, got_rep, err = run([fmt, "-p", "4", "-x", os.path.join(d, "idx")] + reads + ["--out-bgzf"], t, env=env)
            assert inflated(z) == tsv and got_rep == rep, err
            assert len(z) < len(tsv)


def test_a_tab6_case_inflates_to_the_recorded_tsv():
    d, _ = common.golden("synth_small")
    dg, g = common.golden("tab_reads")
    c = [x for x in g["cases"] if x["name"] == T.case_name("pe6", "plain", False)][0]
    want = open(os.path.join(dg, c["tsv"]), "rb").read(), open(os.path.join(dg, c["report"]), "rb").read()
    se, pe = T.records(d)
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "pe6.tab")
        open(p, "wb").write(T.text_of("pe6", se, pe))
        z, rep, err = run(["-p", "4", "-x", os.path.join(d, "idx"), "--tab6", p, "--out-bgzf"], t, env=dict(SMALL, CF_TEXT_BLOCK="4096"))
        assert inflated(z) == want[0] and rep == want[1], err


VARIANTS = {
    "small_blocks": (["-t"], {"CF_TEXT_BLOCK": "4096"}),
    "host_io": (["--host-io"], {}),
    "host_parse": ([], {"CF_TEXT_BLOCK": "8192", "CF_CLI_TEXT_HOST_PARSE": "1"}),
    "cols": (["--tab-fmt-cols", "readID,taxID,taxName,readSeq,readQual"], {"CF_TEXT_BLOCK": "4096"}),
    "sam": (["--out-fmt", "sam"], {"CF_TEXT_BLOCK": "4096"}),
    "upto": (["-u", "37"], {"CF_TEXT_BLOCK": "4096"}),
    "one_slot": (["--slots", "1"], {"CF_TEXT_BLOCK": "4096"}),
    "two_threads_one_gpu": (["--gpu-list", "0,0"], {"CF_TEXT_BLOCK": "4096"}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants_inflate_to_what_the_command_prints_without_the_flag(variant):
    extra, env = VARIANTS[variant]
    d, c, tsv, rep = golden_case("fastq")
    args = ["-q", "-p", "4", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fq")] + extra
    with tempfile.TemporaryDirectory() as t:
        plain = run(args, t, env=env, tag="p")
        z = run(args + ["--out-bgzf"], t, env=dict(SMALL, **env), tag="z")
        assert inflated(z[0]) == plain[0] and z[1] == plain[1]
        if variant == "small_blocks":
            # the blocks took the device path, and their rows were deflated there: none went through the host's zlib
            nb = blocks(z[2])
            assert nb and nb[0] > 10 and nb[1] == 0, z[2]
            m = re.search(r"Device deflate: (\d+) batch\(es\), (\d+) bytes of text into (\d+) bytes", z[2])
            assert m and int(m.group(1)) == nb[0] and int(m.group(2)) == len(plain[0]) - len(plain[0].split(b"\n", 1)[0]) - 1, z[2]
            members = I.member_table(z[0])[0]
            assert int(m.group(3)) == len(z[0]) - 28 - (int(members[0][1]) + 26)          # everything but the header line's member and the EOF member
        if variant in ("small_blocks", "host_io", "host_parse", "one_slot", "two_threads_one_gpu"):
            assert plain[0] == tsv


def test_separator_markers_are_part_of_the_file():
    """--separator: the marker line behind each input goes through the same container, in its place (the per-input reports go into
    the working directory)"""
    d, c, tsv, rep = golden_case("k5")
    reads = os.path.join(d, "reads.fa")
    outs = []
    for extra in ([], ["--out-bgzf"]):
        with tempfile.TemporaryDirectory() as t:
            r = subprocess.run([CLI, "-f", "-p", "4", "-x", os.path.join(d, "idx"), "-U", reads + "," + reads, "--separator", "-S", os.path.join(t, "o.tsv")] + extra,
                               capture_output=True, cwd=t, env=dict(os.environ, **SMALL), timeout=180)
            assert r.returncode == 0, r.stderr
            outs.append((open(os.path.join(t, "o.tsv"), "rb").read(), [open(os.path.join(t, "centrifuge_report_%d.tsv" % i), "rb").read() for i in (0, 1)]))
    assert inflated(outs[1][0]) == outs[0][0] and outs[1][1] == outs[0][1]
    assert outs[0][0].count(b"#File_End_Here\n") == 2


def test_output_into_a_pipe():
    d, c, tsv, rep = golden_case("k5")
    with tempfile.TemporaryDirectory() as t:
        r = subprocess.run([CLI, "-f", "-p", "4", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "--out-bgzf", "--report-file", os.path.join(t, "p.rep")],
                           capture_output=True, env=dict(os.environ, CF_TEXT_BLOCK="4096", **SMALL), timeout=180)
        assert r.returncode == 0, r.stderr
        assert inflated(r.stdout) == tsv and open(os.path.join(t, "p.rep"), "rb").read() == rep


def test_a_bgzf_input_is_inflated_and_its_output_deflated_in_one_process():
    d, c, tsv, rep = golden_case("fastq")
    with tempfile.TemporaryDirectory() as t:
        p = write_bgzf(os.path.join(t, "reads.fq.gz"), open(os.path.join(d, "reads.fq"), "rb").read())
        args = ["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", p]
        z, got_rep, err = run(args + ["--out-bgzf"], t, env=SMALL)
        assert "BGZF member(s) inflated on the device" in err
        assert inflated(z) == tsv and got_rep == rep
    # ... and a pair of BGZF mate files
    d, c, tsv, rep = golden_case("pe_k5")
    with tempfile.TemporaryDirectory() as t:
        ps = [write_bgzf(os.path.join(t, f + ".gz"), open(os.path.join(d, f), "rb").read()) for f in c["reads"]]
        z, got_rep, err = run(["-f", "-p", "4", "-x", os.path.join(d, "idx"), "-1", ps[0], "-2", ps[1], "--device-inflate", "all", "--out-bgzf"], t, env=SMALL)
        assert inflated(z) == tsv and got_rep == rep


def test_an_input_without_reads_gives_the_header_member_and_the_eof_member():
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "none.fa")
        open(p, "wb").close()
        args = ["-f", "-x", os.path.join(d, "idx"), "-U", p]
        plain = run(args, t, tag="p")
        z = run(args + ["--out-bgzf"], t, tag="z")
        assert inflated(z[0]) == plain[0] and plain[0].count(b"\n") == 1 and z[1] == plain[1]
        assert len(I.member_table(z[0])[0]) == 2
