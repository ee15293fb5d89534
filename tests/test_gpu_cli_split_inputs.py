"""--un / --al / --un-conc / --al-conc of centrifuge-class over the inputs tests/test_gpu_cli_split.py does not reach: BGZF files
inflated on the device (unpaired, and mates under --device-inflate all), a BGZF file handed over to the parser pool half way,
tabbed files (--tab5 unpaired, --tab6 pairs, a file that mixes both: runs of the host's), and FASTQ mates of UNEQUAL lengths, plain
and BGZF.  The expected files are the contract's Python statement (tests/splitcases.py) applied to the rows the same command prints
with --host-io --tab-fmt-cols readID,seqID,readSeq,readQual and no split option (the host's general formatter, pinned to the
reference binary by tests/test_gpu_cli.py); the -S output must be the bytes of the same run without the options."""
import os
import tempfile

import pytest

import common
import splitcases
import tabcases as T
from test_gpu_cli_bgzf import members, odd_fastq, write_bgzf
from test_gpu_cli_bgzf_pair import fastq_of
from test_gpu_cli_text import blocks, run

pytestmark = pytest.mark.gpu
COLS = ["readID", "seqID", "readSeq", "readQual"]
SMALL = {"CF_TEXT_BLOCK": "4096"}
FILES = {"un": "u.fq", "al": "a.fq", "un1": "uc.1.fq", "un2": "uc.2.fq", "al1": "ac_1", "al2": "ac_2"}
OPTS = ["--un", "u.fq", "--al", "a.fq", "--un-conc", "uc.fq", "--al-conc", "ac_%"]


def check(args, t, env=None, gz=False, feeds=None):
    """-> stderr of the run with the split options.  feeds: the files that must not stay empty"""
    rows_tsv = run(args + ["--host-io", "--tab-fmt-cols", ",".join(COLS)], t, tag="rows")[0]
    want = splitcases.contract(splitcases.rows_of_tsv(rows_tsv, COLS))
    plain = run(args, t, env=env, tag="plain")[0]
    opts = [o + "-gz" if gz and o.startswith("--") else o for o in OPTS]
    opts = [os.path.join(t, o) if not o.startswith("--") else o for o in opts]
    tsv, _, err = run(args + opts, t, env=env, tag="split")
    assert tsv == plain, "the -S output changes with the split options"
    for key, fn in FILES.items():
        got = open(os.path.join(t, fn), "rb").read()
        if gz:
            got = splitcases.inflate_bgzf(got)
        assert got == want[key], (key, common.first_diff(got.decode("latin1"), want[key].decode("latin1")))
    for key in feeds or ():
        assert want[key], "the case should feed " + key
    return err


def unequal_fastq_mates(d):
    """r1.fa / r2.fa as FASTQ with seeded qualities, every second mate cut short by 1 .. 9 bases: (text 1, text 2)"""
    m1, m2 = (open(os.path.join(d, f), "rb").read() for f in ("r1.fa", "r2.fa"))
    q2 = []
    for i, rec in enumerate(fastq_of(m2, 2)):
        name, seq, plus, qual = rec.split(b"\n")[:4]
        cut = 1 + i % 9
        q2.append(b"\n".join([name, seq[:-cut], plus, qual[:-cut]]) + b"\n")
    return b"".join(fastq_of(m1, 1)), b"".join(q2)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_bgzf_input_inflated_on_the_device(gz):
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        f = write_bgzf(os.path.join(t, "reads.fq.gz"), open(os.path.join(d, "reads.fq"), "rb").read())
        err = check(["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", f], t, env=SMALL, gz=gz, feeds=("un", "al"))
        assert members(err)[0] > 10 and members(err)[1] == 0 and blocks(err)[0] > 10, err
        assert "split on the device" in err


def test_bgzf_input_handed_over_to_the_parser_pool():
    """records 200 .. 219 with CR LF: the runs in front of them are the device's, the rest of the file the parser pool's"""
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        f = write_bgzf(os.path.join(t, "odd.fq.gz"), odd_fastq(open(os.path.join(d, "reads.fq"), "rb").read(), "crlf"))
        err = check(["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", f], t, env=SMALL, feeds=("un", "al"))
        dev, host = members(err)
        assert dev >= 5 and host >= 5, err


@pytest.mark.parametrize("bgzf", [False, True], ids=["text", "bgzf"])
def test_fastq_mates_of_unequal_lengths(bgzf):
    d, _ = common.golden("synth_small")
    q1, q2 = unequal_fastq_mates(d)
    with tempfile.TemporaryDirectory() as t:
        if bgzf:
            f1, f2 = write_bgzf(os.path.join(t, "r1.fq.gz"), q1), write_bgzf(os.path.join(t, "r2.fq.gz"), q2)
        else:
            f1, f2 = os.path.join(t, "r1.fq"), os.path.join(t, "r2.fq")
            open(f1, "wb").write(q1); open(f2, "wb").write(q2)
        args = ["-q", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-1", f1, "-2", f2] + (["--device-inflate", "all"] if bgzf else [])
        err = check(args, t, env=SMALL, feeds=("un1", "un2", "al1", "al2"))
        assert blocks(err)[0] > 10 and blocks(err)[1] == 0, err
        if bgzf:
            assert members(err)[0] > 40 and members(err)[1] == 0, err
        sizes = [os.path.getsize(os.path.join(t, FILES[k])) for k in ("al1", "al2")]
        assert sizes[0] != sizes[1]


@pytest.mark.parametrize("inp", ["se", "pe5", "pe6", "mix"])
def test_tabbed_inputs(inp):
    d, _ = common.golden("synth_small")
    se, pe = T.records(d)
    with tempfile.TemporaryDirectory() as t:
        f = os.path.join(t, inp + ".tab")
        open(f, "wb").write(T.text_of(inp, se, pe))
        args = ["-t", "-p", "4", "-x", os.path.join(d, "idx"), T.flag_of(inp), f]
        err = check(args, t, env=SMALL, feeds=("un", "al") if inp == "se" else ("un1", "al1") if inp != "mix" else ("un", "al", "un1", "al1"))
        b = blocks(err)
        assert b[0] + b[1] > 10 and (b[1] == 0 if inp != "mix" else b[1] >= 1), err


def test_tab6_bgzf_input():
    d, _ = common.golden("synth_small")
    se, pe = T.records(d)
    with tempfile.TemporaryDirectory() as t:
        f = write_bgzf(os.path.join(t, "pe6.tab.gz"), T.text_of("pe6", se, pe))
        err = check(["-t", "-p", "4", "-x", os.path.join(d, "idx"), "--tab6", f], t, env=SMALL, gz=True, feeds=("un1", "al1"))
        assert members(err)[0] > 10 and members(err)[1] == 0, err
