"""--tab5 / --12 / --tab6 through the host parser (cf_ingest.cpp parseTabChunk, a restatement of TabbedPatternSource::readPair,
pat.cpp:1217-1503): `centrifuge-class --dump-reads` prints name, bases, qualities and seed per read.  The seeds are checked
against the FASTQ / FASTA parsers' for the same reads (genRandSeed sees the same name, bases and qualities), the rules record by
record against small hand-made files.  Needs no GPU; on the code before this change every test fails: the options are unknown."""
import os
import subprocess
import tempfile

import pytest

import common
import tabcases as T

CLI = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-class")
SMALL = {"CF_DEBUG_KNOBS": "1", "CF_INGEST_BLOCK": "4096"}


def dump(args, env=None, ok=True):
    r = subprocess.run([CLI, "--dump-reads"] + args, capture_output=True, env=dict(os.environ, **(env or {})))
    if not ok:
        return r
    assert r.returncode == 0, r.stderr.decode()
    return [tuple(ln.split(b"\t")) for ln in r.stdout.split(b"\n")[:-1]]


def dump_text(text, flag="--tab5", extra=(), ok=True, how="file"):
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "in.tab")
        open(p, "wb").write(text)
        return dump([flag, p] + list(extra), ok=ok) if how == "file" else dump(["--tab5", p, how, p] + list(extra), ok=ok)


@pytest.fixture(scope="module")
def synth():
    d, _ = common.golden("synth_small")
    se, pe = T.records(d)
    fq = dump(["-q", "-U", os.path.join(d, "reads.fq")])
    m1, m2 = dump(["-f", "-U", os.path.join(d, "r1.fa")]), dump(["-f", "-U", os.path.join(d, "r2.fa")])
    return d, se, pe, fq, m1, m2


@pytest.mark.parametrize("env", [None, SMALL], ids=["one_block", "blocks_of_4096"])
def test_synth_small_as_tabbed_files_gives_the_reads_and_seeds_of_the_fastq_and_fasta_parsers(synth, env):
    d, se, pe, fq, m1, m2 = synth
    assert len(fq) == len(se) and len(m1) == len(pe)
    with tempfile.TemporaryDirectory() as t:
        for inp in ("se", "pe5", "pe6", "mix"):
            open(os.path.join(t, inp), "wb").write(T.text_of(inp, se, pe))
        p = lambda n: os.path.join(t, n)
        assert dump(["--tab5", p("se"), "-p", "3"], env) == fq
        assert dump(["--12", p("se"), "-p", "3"], env) == fq
        want6 = [r for ab in zip(m1, m2) for r in ab]
        assert dump(["--tab6", p("pe6"), "-p", "3"], env) == want6
        # --tab5: both mates under the first mate's name (the file's names have no /1: the seed stops at a '/' anyway)
        want5 = [(T.base(r[0]),) + r[1:] for r in want6]
        assert dump(["--tab5", p("pe5"), "-p", "3"], env) == want5
        got = dump(["--tab5", p("mix"), "-p", "3"], env)
        want = []
        for kind, k in T.mix_kinds(se, pe):
            want += [fq[k]] if kind == "se" else want5[2 * k:2 * k + 2]
        assert got == want
        # -s / -u count records (a pair is one), -5 / -3 trim each mate
        got = dump(["--tab5", p("mix"), "-s", "5", "-u", "6"], env)
        assert got == want[10:18]                            # records 5 and 6 are pairs, 7 .. 10 unpaired (-u counts behind -s)
        got = dump(["--tab6", p("pe6"), "-5", "7", "-3", "11", "-u", "9"], env)
        assert [(r[0], r[1], r[2]) for r in got] == [(r[0], r[1][7:-11], r[2][7:-11]) for r in want6[:18]]


def test_the_rules_of_readpair_record_by_record():
    rec = lambda *f: b"\t".join(f)
    # blank lines in front of records are skipped; CR LF; lower case and N; what is no letter is dropped from a sequence; quality
    # values beyond the bases are skipped unseen; the last line needs no line end
    text = b"\n\r\n" + rec(b"a", b"acgtN", b"IIIII") + b"\r\n\n" + rec(b"b x/1", b"AC-G.T1", b"ABCDEFG", b"NNgg", b"5678") + b"\n" + rec(b"c", b"A", b"#")
    got = dump_text(text)
    assert [(r[0], r[1], r[2]) for r in got] == [(b"a", b"ACGTN", b"IIIII"), (b"b x/1", b"ACGT", b"ABCD"), (b"b x/1", b"NNGG", b"5678"), (b"c", b"A", b"#")]
    # a record without a name is named after its number, both mates alike; --tab6 with an empty second name
    text = rec(b"", b"AC", b"II") + b"\n" + rec(b"n", b"A", b"I") + b"\n" + rec(b"", b"AC", b"II", b"", b"GT", b"II") + b"\n" + rec(b"m", b"AC", b"II", b"", b"GT", b"II") + b"\n"
    assert [r[0] for r in dump_text(text, "--tab6")] == [b"0", b"n", b"2", b"2", b"m", b"3"]
    assert [r[0] for r in dump_text(rec(b"", b"AC", b"II", b"GT", b"II") + b"\n" + rec(b"", b"A", b"I") + b"\n")] == [b"0", b"0", b"1"]
    # a line end inside a name ends the input, as does the end of the file inside a record
    assert [r[0] for r in dump_text(rec(b"a", b"A", b"I") + b"\nno tab here\n" + rec(b"b", b"A", b"I") + b"\n")] == [b"a"]
    assert [r[0] for r in dump_text(rec(b"a", b"A", b"I") + b"\n" + rec(b"b", b"ACGT", b"II"))] == [b"a"]
    # -U / -1 / -2 files of a tabbed run: a line a read, what follows the third field unseen (TabbedPatternSource::read)
    pair = rec(b"p", b"AC", b"II", b"GT", b"II") + b"\n"
    assert [(r[0], r[1]) for r in dump_text(pair, how="-U")] == [(b"p", b"AC"), (b"p", b"GT"), (b"p", b"AC")]      # (named twice: as a --tab5 file first, then as a -U file)
    assert [(r[0], r[1]) for r in dump_text(pair)] == [(b"p", b"AC"), (b"p", b"GT")]


@pytest.mark.parametrize("text,message", [
    (b"r\tACGT\tIII\n", b"Error: Read r has more read characters than quality values."),
    (b"r\tACGT\tIIII\tACGT\tIII\n", b"Error: Read r has more read characters than quality values."),
    (b"r\tACGT\tII I\n", b"Error: Encountered one or more spaces while parsing the quality string for read r."),
    (b"r\tACGT\tII\x1fI\n", b"Saw ASCII character 31 but expected 33-based Phred qual."),
], ids=["short", "short_mate2", "space", "below_33"])
def test_quality_errors_carry_the_references_messages(text, message):
    r = dump_text(text, ok=False)
    assert r.returncode == 1 and message in r.stderr, r.stderr


def test_the_recorded_bad_quality_case_and_the_command_line():
    d, g = common.golden("tab_reads")
    se, pe = T.records(common.golden("synth_small")[0])
    bad = T.text_of("se", se, pe).split(b"\n")
    f = bad[1].split(b"\t")
    bad[1] = b"\t".join([f[0], f[1], f[2][:-1]])
    r = dump_text(b"\n".join(bad), ok=False)
    assert r.returncode == g["bad_qual"]["returncode"] and g["bad_qual"]["stderr"].encode() in r.stderr
    # a tabbed option names read input; the usage text knows the options
    r = subprocess.run([CLI, "--dump-reads"], capture_output=True)
    assert r.returncode == 1 and b"Must specify at least one read input" in r.stderr and b"--tab6" in r.stderr
