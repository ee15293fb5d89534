"""centrifuge-class on BGZF read files: an unpaired .gz file whose members are BGZF's goes up compressed, in runs of whole members,
is inflated on the device (cf_batch_upload_bgzf) and takes the device text path from there — the same bytes out as the host
threads give and as the reference's golden TSV and report hold; a file with records outside the plain form is handed to the
parser pool where they begin.  The files are made here with zlib (raw deflate in BGZF headers).  Corrupt members — in the CPU
harness (tests/test_inflate_emu.py) and, as damaged files given to this program, on the GPU — are tests/test_gpu_codec.py's."""
import gzip
import os
import re
import subprocess
import tempfile

import pytest

import common
from emu import emu_inflate as E
from test_gpu_cli_text import CLI, blocks, run

pytestmark = pytest.mark.gpu
MEMBER = 1500                      # text bytes per member: every file here holds dozens of them
COLS = ["--tab-fmt-cols", "readID,taxID,numMatches,readSeq,readQual"]


def bgzf(text, size=MEMBER):
    return b"".join(E.bgzf_member(text[i:i + size]) for i in range(0, len(text), size)) + E.bgzf_member(b"")


def write_bgzf(path, text, size=MEMBER):
    with open(path, "wb") as f:
        f.write(bgzf(text, size))
    return path


def members(err):
    """(on the device, on the host) of the stderr line, None when it is not printed"""
    m = re.search(r"Device inflate: (\d+) BGZF member\(s\) inflated on the device, (\d+) on the host", err)
    return (int(m.group(1)), int(m.group(2))) if m else None


def first_reads(tsv, n):
    """the header and the rows of the first n reads of a TSV (a read's rows are adjacent)"""
    lines = tsv.split(b"\n")[:-1]
    out, seen, last = [lines[0]], 0, None
    for ln in lines[1:]:
        rid = ln.split(b"\t", 1)[0]
        if rid != last:
            seen += 1
            last = rid
        if seen > n:
            break
        out.append(ln)
    return b"\n".join(out) + b"\n"


@pytest.mark.parametrize("name,fmt,reads", [("k5", "-f", "reads.fa"), ("fastq", "-q", "reads.fq"), ("r250_k5", "-f", "reads250.fa")])
def test_bgzf_files_are_inflated_on_the_device_and_print_the_golden_output(name, fmt, reads):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    want = open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()
    text = open(os.path.join(d, reads), "rb").read()
    with tempfile.TemporaryDirectory() as t:
        gz = write_bgzf(os.path.join(t, reads + ".gz"), text)
        n_members = -(-len(text) // MEMBER) + 1
        args = [fmt, "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", gz]
        small = {"CF_TEXT_BLOCK": "4096"}
        for env in (small, None):
            tsv, rep, err = run(args, t, env=env)
            assert (tsv, rep) == want, common.first_diff(tsv.decode("latin1"), want[0].decode("latin1"))
            assert members(err) == (n_members, 0) and n_members > 10, err
            assert blocks(err)[1] == 0 and (blocks(err)[0] > 10 if env else blocks(err)[0] == 1), err
        # one slot; -u inside a run, past a run's end, past the file; the output into a pipe; columns that hold the reads' own text
        tsv, rep, err = run(args + ["--slots", "1"], t, env=small)
        assert (tsv, rep) == want and members(err)[0] > 10 and members(err)[1] == 0
        for u in (1, 37, 100000):
            tsv, rep, err = run(args + ["-u", str(u)], t, env=small)
            assert tsv == first_reads(want[0], u), u
            assert members(err)[0] >= 1 and members(err)[1] == 0, err
            if u == 37:
                assert rep == run(args + ["-u", "37", "--host-io"], t, tag="h")[1]
        r = subprocess.run([CLI] + args + ["--report-file", os.path.join(t, "p.rep")], capture_output=True, env=dict(os.environ, **small))
        assert r.returncode == 0 and r.stdout == want[0] and open(os.path.join(t, "p.rep"), "rb").read() == want[1]
        assert members(r.stderr.decode()) == (n_members, 0)
        a = run(args + COLS, t, env=small, tag="a")
        b = run(args + COLS + ["--host-io"], t, tag="b")
        assert a[:2] == b[:2] and members(a[2]) == (n_members, 0) and members(b[2]) is None


def n_reads(tsv):
    """the reads a TSV holds rows for (a read's rows are adjacent)"""
    ids = [ln.split(b"\t", 1)[0] for ln in tsv.split(b"\n")[1:-1]]
    return sum(1 for i, r in enumerate(ids) if i == 0 or r != ids[i - 1])


@pytest.mark.parametrize("window,printed", [(["-s", "13", "-u", "40"], 40), (["-s", "101"], 199)])
def test_skip_and_upto_windows_on_a_bgzf_file_print_what_the_host_threads_print(window, printed):
    """-s beyond the first run's records (a run of 4096 bytes holds about seven of the 300): runs of which nothing is printed, then a
    run that starts in its middle — and, with -u, one that ends in its middle"""
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        gz = write_bgzf(os.path.join(t, "reads.fq.gz"), open(os.path.join(d, "reads.fq"), "rb").read())
        args = ["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", gz] + window
        a = run(args, t, env={"CF_TEXT_BLOCK": "4096"}, tag="a")
        b = run(args + ["--host-io"], t, tag="b")
        assert a[0] == b[0], common.first_diff(a[0].decode("latin1"), b[0].decode("latin1"))
        assert a[1] == b[1] and n_reads(b[0]) == printed
        assert members(a[2])[0] >= 3 and members(a[2])[1] == 0 and members(b[2]) is None, a[2]


def test_the_switches_leave_bgzf_files_to_the_host_threads():
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == "fastq"][0]
    want = open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()
    with tempfile.TemporaryDirectory() as t:
        gz = write_bgzf(os.path.join(t, "reads.fq.gz"), open(os.path.join(d, "reads.fq"), "rb").read())
        args = ["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", gz]
        for extra, env in ((["--host-io"], None), ([], {"CF_CLI_DEVICE_INFLATE": "0"})):
            tsv, rep, err = run(args + extra, t, env=env)
            assert (tsv, rep) == want and members(err) is None and blocks(err) is None, err


def odd_fastq(text, kind):
    """the FASTQ text with records 200..219 written with CR LF, or with their bases wrapped at 40 letters (the qualities stay one line: the parser, as the reference's, asks for that)"""
    ls = text.split(b"\n")[:-1]
    recs = [ls[k:k + 4] for k in range(0, len(ls), 4)]
    out = []
    for i, r in enumerate(recs):
        if 200 <= i < 220 and kind == "crlf":
            out.append(b"\r\n".join(r) + b"\r\n")
        elif 200 <= i < 220:
            wrap = lambda s: b"\n".join(s[k:k + 40] for k in range(0, len(s), 40))
            out.append(r[0] + b"\n" + wrap(r[1]) + b"\n+\n" + r[3] + b"\n")
        else:
            out.append(b"\n".join(r) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("kind", ["crlf", "wrapped"])
def test_a_file_that_leaves_the_plain_form_is_handed_to_the_parser_pool(kind):
    d, _ = common.golden("synth_small")
    text = odd_fastq(open(os.path.join(d, "reads.fq"), "rb").read(), kind)
    with tempfile.TemporaryDirectory() as t:
        gz = write_bgzf(os.path.join(t, "odd.fq.gz"), text)
        n_members = -(-len(text) // MEMBER) + 1
        args = ["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", gz]
        for extra in ([], ["-u", "300"]):
            want = run(args + extra + ["--host-io"], t, tag="h")
            got = run(args + extra, t, env={"CF_TEXT_BLOCK": "4096"})
            assert got[0] == want[0], common.first_diff(got[0].decode("latin1"), want[0].decode("latin1"))
            assert got[1] == want[1]
            dev, host = members(got[2])
            assert dev >= 5 and host >= 5 and (extra or dev + host == n_members), got[2]


def test_other_gz_files_and_mates_keep_the_host_threads():
    d, cases = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        # a .gz file that is not BGZF
        c = [x for x in cases if x["name"] == "k5"][0]
        want = open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()
        gz = os.path.join(t, "reads.fa.gz")
        with gzip.open(gz, "wb") as f:
            f.write(open(os.path.join(d, "reads.fa"), "rb").read())
        tsv, rep, err = run(["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", gz], t)
        assert (tsv, rep) == want and members(err) is None, err
        # mates of BGZF files
        c = [x for x in cases if x["name"] == "pe_k5"][0]
        want = open(os.path.join(d, c["tsv"]), "rb").read(), open(os.path.join(d, c["report"]), "rb").read()
        m1 = write_bgzf(os.path.join(t, "r1.fa.gz"), open(os.path.join(d, "r1.fa"), "rb").read())
        m2 = write_bgzf(os.path.join(t, "r2.fa.gz"), open(os.path.join(d, "r2.fa"), "rb").read())
        tsv, rep, err = run(["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", m1, "-2", m2], t)
        assert (tsv, rep) == want and members(err) is None, err
