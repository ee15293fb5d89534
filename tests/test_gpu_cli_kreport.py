"""centrifuge-class --kreport-file: the Kraken-style report tallied on the device equals what centrifuge-kreport prints for the same
run's classification output, on every input path; two neighbouring reads of one name — which the tool counts as one — are refused
(exit status 1, no file, output and report as without the flag), inside a block, across a block border and with names of 300 bytes."""
import os
import subprocess
import tempfile

import pytest

import common
import tabcases as T
from test_gpu_cli_bgzf import write_bgzf
from test_gpu_cli_text import CLI, blocks

pytestmark = pytest.mark.gpu
KREPORT = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-kreport")


def run(args, d, env=None, tag="o", kreport=True):
    """-> returncode, tsv, report, kreport file (None: not written), stderr"""
    out, rep, kr = (os.path.join(d, tag + e) for e in (".tsv", ".rep", ".kreport"))
    r = subprocess.run([CLI] + args + ["-S", out, "--report-file", rep] + (["--kreport-file", kr] if kreport else []),
                       capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=180)
    return r.returncode, open(out, "rb").read(), open(rep, "rb").read(), (open(kr, "rb").read() if os.path.exists(kr) else None), r.stderr, out


def tool(idx, tsv_path):
    r = subprocess.run([KREPORT, "-x", idx, tsv_path], capture_output=True)
    assert r.returncode == 0 and r.stdout.count(b"\n") > 3, r.stderr
    return r.stdout


def golden_case(name):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    return d, c, open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()


@pytest.mark.parametrize("name,fmt", [("k5", "-f"), ("fastq", "-q"), ("pe_k5", "-f")])
def test_golden_cases(name, fmt):
    d, c, tsv, rep = golden_case(name)
    files = [os.path.join(d, f) for f in c["reads"]]
    reads = ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
    with tempfile.TemporaryDirectory() as t:
        rc, got, got_rep, kr, err, out = run([fmt, "-p", "4", "-x", os.path.join(d, "idx")] + reads, t)
        assert rc == 0 and got == tsv and got_rep == rep, err
        assert kr == tool(os.path.join(d, "idx"), out)


def test_a_tab6_case():
    d, _ = common.golden("synth_small")
    dg, g = common.golden("tab_reads")
    c = [x for x in g["cases"] if x["name"] == T.case_name("pe6", "plain", False)][0]
    want = open(os.path.join(dg, c["tsv"]), "rb").read(), open(os.path.join(dg, c["report"]), "rb").read()
    se, pe = T.records(d)
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "pe6.tab")
        open(p, "wb").write(T.text_of("pe6", se, pe))
        rc, got, rep, kr, err, out = run(["-p", "4", "-x", os.path.join(d, "idx"), "--tab6", p], t, env={"CF_TEXT_BLOCK": "4096"})
        assert rc == 0 and (got, rep) == want, err
        assert kr == tool(os.path.join(d, "idx"), out)


VARIANTS = {
    "small_blocks": (["-t"], {"CF_TEXT_BLOCK": "4096"}),
    "host_io": (["--host-io"], {}),
    "host_parse": ([], {"CF_TEXT_BLOCK": "8192", "CF_CLI_TEXT_HOST_PARSE": "1"}),
    "upto": (["-u", "37"], {"CF_TEXT_BLOCK": "4096"}),
    "skip": (["-s", "5"], {"CF_TEXT_BLOCK": "4096"}),
    "trim": (["-5", "3", "-3", "3"], {"CF_TEXT_BLOCK": "4096"}),
    "two_threads_one_gpu": (["--gpu-list", "0,0"], {"CF_TEXT_BLOCK": "4096"}),
    "bgzf_in": ([], {}),
    "out_bgzf": (["--out-bgzf"], {"CF_TEXT_BLOCK": "4096"}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants(variant):
    extra, env = VARIANTS[variant]
    d, c, tsv, rep = golden_case("fastq")
    idx = os.path.join(d, "idx")
    with tempfile.TemporaryDirectory() as t:
        reads = os.path.join(d, "reads.fq")
        if variant == "bgzf_in":
            reads = write_bgzf(os.path.join(t, "reads.fq.gz"), open(reads, "rb").read())
        args = ["-q", "-p", "4", "-x", idx, "-U", reads] + extra
        plain = run(args, t, env=env, tag="p", kreport=False)
        rc, got, got_rep, kr, err, out = run(args, t, env=env)
        assert rc == 0 and plain[0] == 0 and (got, got_rep) == (plain[1], plain[2]), err
        assert kr == tool(idx, out)                              # (--out-bgzf: the tool reads the .gz as it is)
        if variant in ("small_blocks", "host_io", "host_parse", "two_threads_one_gpu", "bgzf_in"):
            assert got == tsv and got_rep == rep
        if variant == "small_blocks":
            nb = blocks(err)
            assert nb and nb[0] > 10 and nb[1] == 0 and "k_kreport" in err, err


def fasta_records(d, n, names, width=44):
    """n FASTA records of one line each, `width` golden reads long (more than 4,096 bytes: a block of 4,096 holds one record)"""
    seqs = [ln for ln in open(os.path.join(d, "reads.fa")).read().split("\n") if ln and ln[0] != ">"]
    return "".join(">%s\n%s\n" % (names[i], "".join(seqs[i * width:(i + 1) * width])) for i in range(n)).encode()


def fastq_with_names(d, rename):
    """the golden FASTQ reads, record i named rename[i] where given"""
    lines = open(os.path.join(d, "reads.fq")).read().split("\n")[:-1]
    for i, nm in rename.items():
        lines[4 * i] = "@" + nm
    return ("\n".join(lines) + "\n").encode()


def refused(d, t, path, fmt, name, extra, env, want_blocks=None):
    idx = os.path.join(d, "idx")
    args = [fmt, "-t", "-p", "4", "-x", idx, "-U", path] + extra
    plain = run(args, t, env=env, tag="p", kreport=False)
    rc, got, rep, kr, err, out = run(args, t, env=env)
    assert plain[0] == 0 and rc == 1, err
    assert kr is None and (got, rep) == (plain[1], plain[2]) and got.count(b"\n") > 5
    assert name[:255] in err and "centrifuge-kreport" in err
    if want_blocks is not None:
        assert blocks(err) == want_blocks, err


@pytest.mark.parametrize("extra", [[], ["--host-io"]], ids=["device", "host_io"])
def test_neighbouring_reads_of_one_name_are_refused(extra):
    d, _ = common.golden("synth_small")
    dev = not extra
    one = [] if dev else ["--batch", "1"]                        # (--host-io: a read a batch, so that the pair lies across two host-parsed pieces)
    with tempfile.TemporaryDirectory() as t:
        # inside a block
        p = os.path.join(t, "dup.fq")
        open(p, "wb").write(fastq_with_names(d, {40: "twin", 41: "twin extra words"}))
        refused(d, t, p, "-q", "twin", extra, {}, (1, 0) if dev else None)
        # across a block border: every block holds one record
        names = ["c%d" % i for i in range(6)]
        names[3] = names[2] = "straddle"
        p = os.path.join(t, "border.fa")
        open(p, "wb").write(fasta_records(d, 6, names))
        refused(d, t, p, "-f", "straddle", extra + one, {"CF_TEXT_BLOCK": "4096"}, (6, 0) if dev else None)
        # ... with names of 300 bytes
        long = "L" * 300
        names = ["c%d" % i for i in range(6)]
        names[4] = names[3] = long
        p = os.path.join(t, "long.fa")
        open(p, "wb").write(fasta_records(d, 6, names))
        refused(d, t, p, "-f", long, extra + one, {"CF_TEXT_BLOCK": "4096"}, (6, 0) if dev else None)
        # ... and names of 300 bytes that differ behind byte 255 are refused too (erring towards refusal)
        names[4] = "L" * 299 + "x"
        open(p, "wb").write(fasta_records(d, 6, names))
        refused(d, t, p, "-f", "L" * 255, extra + one, {"CF_TEXT_BLOCK": "4096"}, (6, 0) if dev else None)


@pytest.mark.parametrize("extra", [[], ["--host-io"]], ids=["device", "host_io"])
def test_reads_of_one_name_that_are_no_neighbours_are_counted(extra):
    d, _ = common.golden("synth_small")
    idx = os.path.join(d, "idx")
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "apart.fq")
        open(p, "wb").write(fastq_with_names(d, {40: "twin", 42: "twin"}))
        rc, got, rep, kr, err, out = run(["-q", "-p", "4", "-x", idx, "-U", p] + extra, t, env={"CF_TEXT_BLOCK": "4096"})
        assert rc == 0 and kr is not None and kr == tool(idx, out), err
