"""centrifuge-class --device-inflate all on the BGZF files of mates: -1 r1.gz -2 r2.gz go up compressed, in runs of whole members
of both files, are inflated on the device and cut there behind a common record (cf_batch_upload_bgzf_pair) — the same bytes out as
the host threads give and as the reference's golden TSV and report hold; files whose records use up different amounts of text
stay on the device all the way, files that leave the plain form or hold different numbers of records are handed to the parser
pool.  The files are made here with zlib (raw deflate in BGZF headers)."""
import gzip
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common
from test_gpu_cli_bgzf import first_reads, members, n_reads, write_bgzf
from test_gpu_cli_text import CLI, blocks, run

pytestmark = pytest.mark.gpu
MEMBER = 1500
ALL = ["--device-inflate", "all"]
SMALL = {"CF_TEXT_BLOCK": "4096"}


def golden_pair():
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == "pe_k5"][0]
    want = open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()
    m1, m2 = (open(os.path.join(d, f), "rb").read() for f in ("r1.fa", "r2.fa"))
    return d, want, m1, m2


def records(src):
    return [b">" + r + (b"" if r.endswith(b"\n") else b"\n") for r in src[1:].split(b"\n>")]


def fastq_of(src, seed):
    """the FASTA records as FASTQ, with seeded random qualities"""
    rng = np.random.default_rng(seed)
    out = []
    for r in records(src):
        name, seq = r.split(b"\n")[:2]
        out.append(b"@" + name[1:] + b"\n" + seq + b"\n+\n" + bytes(int(q) for q in rng.integers(33, 127, len(seq))) + b"\n")
    return out


def n_members(text, size=MEMBER):
    return -(-len(text) // size) + 1


def test_bgzf_mates_are_inflated_on_the_device_and_print_the_golden_output():
    d, want, m1, m2 = golden_pair()
    with tempfile.TemporaryDirectory() as t:
        g1, g2 = write_bgzf(os.path.join(t, "r1.fa.gz"), m1), write_bgzf(os.path.join(t, "r2.fa.gz"), m2)
        n = n_members(m1) + n_members(m2)
        args = ["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2] + ALL
        for env in (SMALL, None):
            tsv, rep, err = run(args, t, env=env)
            assert (tsv, rep) == want, common.first_diff(tsv.decode("latin1"), want[0].decode("latin1"))
            assert members(err) == (n, 0) and n > 40, err
            assert blocks(err)[1] == 0 and (blocks(err)[0] > 10 if env else blocks(err)[0] == 1), err
        tsv, rep, err = run(args + ["--slots", "1"], t, env=SMALL)
        assert (tsv, rep) == want and members(err) == (n, 0)
        # the output into a pipe
        r = subprocess.run([CLI] + args + ["--report-file", os.path.join(t, "p.rep")], capture_output=True, env=dict(os.environ, **SMALL))
        assert r.returncode == 0 and r.stdout == want[0] and open(os.path.join(t, "p.rep"), "rb").read() == want[1]
        assert members(r.stderr.decode()) == (n, 0)
        # -u inside a run, past a run's end, past the files
        for u in (1, 37, 100000):
            a = run(args + ["-u", str(u)], t, env=SMALL, tag="a")
            b = run(args + ["-u", str(u), "--host-io"], t, tag="b")
            assert a[:2] == b[:2] and a[0] == first_reads(want[0], u), u
            assert members(a[2])[0] >= 1 and members(a[2])[1] == 0 and members(b[2]) is None, a[2]


@pytest.mark.parametrize("window,printed", [(["-s", "13", "-u", "40"], 40), (["-s", "101"], 299)])
def test_skip_and_upto_windows_on_bgzf_mates_print_what_the_host_threads_print(window, printed):
    """-s beyond the first run's pairs (the first runs hold about nine of the 400): runs of which nothing is printed, then a run that
    starts in its middle — and, with -u, one that ends in its middle"""
    d, want, m1, m2 = golden_pair()
    with tempfile.TemporaryDirectory() as t:
        g1, g2 = write_bgzf(os.path.join(t, "r1.fa.gz"), m1), write_bgzf(os.path.join(t, "r2.fa.gz"), m2)
        args = ["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2] + window
        a = run(args + ALL, t, env=SMALL, tag="a")
        b = run(args + ["--host-io"], t, tag="b")
        assert a[0] == b[0], common.first_diff(a[0].decode("latin1"), b[0].decode("latin1"))
        assert a[1] == b[1] and n_reads(b[0]) == printed
        assert members(a[2])[0] >= 3 and members(a[2])[1] == 0 and members(b[2]) is None, a[2]


def test_fastq_mates_and_columns_that_hold_the_reads_own_text():
    d, want, m1, m2 = golden_pair()
    cols = ["--tab-fmt-cols", "readID,taxID,readSeq1,readQual2,readSeq,readQual"]
    with tempfile.TemporaryDirectory() as t:
        q1, q2 = b"".join(fastq_of(m1, 1)), b"".join(fastq_of(m2, 2))
        g1, g2 = write_bgzf(os.path.join(t, "r1.fq.gz"), q1), write_bgzf(os.path.join(t, "r2.fq.gz"), q2)
        args = ["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2]
        for extra in ([], cols):
            a = run(args + extra + ALL, t, env=SMALL, tag="a")
            b = run(args + extra + ["--host-io"], t, tag="b")
            assert a[0] == b[0], common.first_diff(a[0].decode("latin1"), b[0].decode("latin1"))
            assert a[1] == b[1] and members(a[2]) == (n_members(q1) + n_members(q2), 0) and members(b[2]) is None, a[2]


def test_lopsided_files_stay_on_the_device():
    """every name of the second file carries a 150-character comment: its records take about twice the text of the first file's"""
    d, want, m1, m2 = golden_pair()
    rng = np.random.default_rng(3)
    wide = []
    for r in records(m2):
        name, rest = r.split(b"\n", 1)
        wide.append(name + b" " + bytes(int(c) for c in rng.integers(97, 123, 150)) + b"\n" + rest)
    w2 = b"".join(wide)
    assert 1.8 < len(w2) / len(m1) < 2.2
    with tempfile.TemporaryDirectory() as t:
        g1, g2 = write_bgzf(os.path.join(t, "r1.fa.gz"), m1, 1500), write_bgzf(os.path.join(t, "r2.fa.gz"), w2, 900)
        args = ["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2]
        a = run(args + ALL, t, env=SMALL, tag="a")
        b = run(args + ["--host-io"], t, tag="b")
        assert a[0] == b[0], common.first_diff(a[0].decode("latin1"), b[0].decode("latin1"))
        assert a[1] == b[1]
        assert members(a[2]) == (n_members(m1, 1500) + n_members(w2, 900), 0), a[2]      # the whole input stayed on the device
        assert blocks(a[2])[0] > 20 and blocks(a[2])[1] == 0


def test_mates_that_leave_the_plain_form_are_handed_to_the_parser_pool():
    d, want, m1, m2 = golden_pair()
    r2 = records(m2)
    for i in range(200, 220):
        r2[i] = b"\r\n".join(r2[i].split(b"\n")[:-1]) + b"\r\n"
    odd = b"".join(r2)
    with tempfile.TemporaryDirectory() as t:
        g1, g2 = write_bgzf(os.path.join(t, "r1.fa.gz"), m1), write_bgzf(os.path.join(t, "r2.fa.gz"), odd)
        args = ["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2]
        for extra in ([], ["-u", "300"]):
            b = run(args + extra + ["--host-io"], t, tag="b")
            a = run(args + extra + ALL, t, env=SMALL, tag="a")
            assert a[0] == b[0], common.first_diff(a[0].decode("latin1"), b[0].decode("latin1"))
            assert a[1] == b[1]
            dev, host = members(a[2])
            assert dev >= 5 and host >= 5 and (extra or dev + host == n_members(m1) + n_members(odd)), a[2]


def test_a_second_file_that_is_short_ends_with_the_reference_message():
    d, want, m1, m2 = golden_pair()
    short = b"".join(records(m2)[:-3])
    with tempfile.TemporaryDirectory() as t:
        g1, g2 = write_bgzf(os.path.join(t, "r1.fa.gz"), m1), write_bgzf(os.path.join(t, "r2.fa.gz"), short)
        args = ["-f", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2, "-S", os.path.join(t, "o.tsv"), "--report-file", os.path.join(t, "o.rep")]
        r = subprocess.run([CLI] + args + ALL, capture_output=True, env=dict(os.environ, **SMALL), timeout=180)
        assert r.returncode == 1 and b"Error, fewer reads in file specified with -2 than in file specified with -1" in r.stderr, r.stderr
        h = subprocess.run([CLI] + args + ["--host-io"], capture_output=True, timeout=180)
        assert h.returncode == 1 and h.stderr.splitlines()[-1:] == r.stderr.splitlines()[-1:]


def test_what_keeps_the_host_threads_and_the_option_itself():
    d, want, m1, m2 = golden_pair()
    cases = common.golden("synth_small")[1]
    with tempfile.TemporaryDirectory() as t:
        # one mate BGZF, the other an ordinary gzip file
        g1 = write_bgzf(os.path.join(t, "r1.fa.gz"), m1)
        g2 = os.path.join(t, "r2.fa.gz")
        with gzip.open(g2, "wb") as f:
            f.write(m2)
        tsv, rep, err = run(["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2] + ALL, t)
        assert (tsv, rep) == want and members(err) is None, err
        # off: an unpaired BGZF file is the host threads' as well
        c = [x for x in cases if x["name"] == "fastq"][0]
        wantq = open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()
        gq = write_bgzf(os.path.join(t, "reads.fq.gz"), open(os.path.join(d, "reads.fq"), "rb").read())
        tsv, rep, err = run(["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", gq, "--device-inflate", "off"], t)
        assert (tsv, rep) == wantq and members(err) is None, err
        # the knob wins over the option
        g2b = write_bgzf(os.path.join(t, "r2b.fa.gz"), m2)
        tsv, rep, err = run(["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", g1, "-2", g2b] + ALL, t, env={"CF_CLI_DEVICE_INFLATE": "0"})
        assert (tsv, rep) == want and members(err) is None, err
        r = subprocess.run([CLI, "-f", "-x", os.path.join(d, "idx"), "-U", gq, "--device-inflate", "bogus"], capture_output=True, timeout=60)
        assert r.returncode != 0 and b"--device-inflate" in r.stderr
