"""centrifuge-class --split-taxids against files DERIVED from the goldens of --un / --al (tests/golden/read_split.tar.xz: per case the
reference's TSV and the files its wrapper script wrote).  The golden `un` and `al` files hold one record per row of the TSV, the
rows with taxID 0 in `un`, the others in `al`, each in the TSV's order; so the TSV's rows are walked, each takes the next record of
its golden file, and the record is dealt to the class the rule gives the row: `al` when its taxID is listed or lies below a listed
taxon in the tree `centrifuge-inspect --taxonomy-tree` prints, `un` otherwise.  Nothing new comes from the reference.

Every case runs on the device text path (the block counts of -t prove the path) with one block and with many, with --host-io
(splitRange), with one CR LF record spliced in (device and host blocks in one file), with the -gz sinks; one from a BGZF input;
the TSV stays the golden's throughout.  On the parent commit --split-taxids is an unrecognized option: every test here fails."""
import functools
import os
import subprocess
import tempfile

import pytest

import common
import splitcases
from test_gpu_cli_bgzf import members, write_bgzf
from test_gpu_cli_split import CLI, blocks, cases, run

pytestmark = pytest.mark.gpu
INSPECT = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-inspect-bin")
CASES = ["fa_k5", "fq_k1_trim", "pe_percent", "pe_bare"]
SELECTIONS = ["internal", "leaf", "zero", "leaf+unknown"]
UNKNOWN = 3999999999


def case(name):
    gd, cs = cases()
    return gd, [x for x in cs if x["name"] == name][0]


def records(data):
    ln = data.split(b"\n")
    assert ln[-1] == b"" and (len(ln) - 1) % 4 == 0
    return [b"\n".join(ln[i:i + 4]) + b"\n" for i in range(0, len(ln) - 1, 4)]


@functools.lru_cache(maxsize=None)
def tree():
    d, _ = common.golden("synth_small")
    out = subprocess.run([INSPECT, "--taxonomy-tree", os.path.join(d, "idx")], capture_output=True, text=True, check=True).stdout
    return {int(ln.split("\t|\t")[0]): int(ln.split("\t|\t")[1]) for ln in out.splitlines()}


def selected(tid, listed):
    parent, steps = tree(), 0
    while True:
        if tid in listed:
            return True
        if tid not in parent or parent[tid] in (tid, 0) or tid == 1:
            return False
        tid, steps = parent[tid], steps + 1
        assert steps < 4096


@functools.lru_cache(maxsize=None)
def golden_rows(name):
    """per row of the golden TSV (taxID, readID, its record per file of its class), from the golden files alone"""
    gd, c = case(name)
    paired = "un1" in c["files"]
    recs = {k: iter(records(open(os.path.join(gd, f), "rb").read())) for k, f in c["files"].items()}
    rows = []
    for ln in open(os.path.join(gd, c["tsv"]), "rb").read().split(b"\n")[1:]:
        if not ln:
            continue
        f = ln.split(b"\t")
        cls = "un" if f[2] == b"0" else "al"
        rec = [next(recs[cls + m]) for m in (("1", "2") if paired else ("",))]
        assert all(r.startswith(b"@" + f[0] + b"\n") for r in rec)
        rows.append((int(f[2]), f[0], rec))
    # the golden files are the TSV's rows, no more
    assert all(next(it, None) is None for it in recs.values())
    return paired, rows


@functools.lru_cache(maxsize=None)
def selection(name, what):
    """the listed IDs, taken from the index's tree and the case's rows: an internal taxon with descendants on the rows, a leaf, 0"""
    parent = tree()
    _, rows = golden_rows(name)
    on_rows = [t for t, _, _ in rows]
    inner = set(parent.values())
    internal = max((t for t in inner if t > 2 and any(x != t and selected(x, {t}) for x in on_rows)), key=lambda t: (on_rows.count(t) > 0, t))
    leaf = max((t for t in set(on_rows) if t in parent and t not in inner), key=on_rows.count)
    listed = {"internal": [internal], "leaf": [leaf], "zero": [0], "leaf+unknown": [leaf, UNKNOWN]}[what]
    return listed


def expected(name, listed):
    paired, rows = golden_rows(name)
    keys = ("un1", "un2", "al1", "al2") if paired else ("un", "al")
    out = {k: b"" for k in keys}
    both, last, seen = 0, None, set()
    for tid, rid, rec in rows:
        cls = "al" if selected(tid, set(listed)) else "un"
        for m, r in enumerate(rec):
            out[cls + (str(m + 1) if paired else "")] += r
        if rid != last:
            both += seen == {"un", "al"}
            seen, last = set(), rid
        seen.add(cls)
    both += seen == {"un", "al"}
    # from the golden TSV alone: the selection leaves neither class empty
    assert all(out[k] for k in keys), (name, listed)
    return out, both


def options(c, listed, gz=False):
    opts = [o + "-gz" if gz and o.startswith("--") else o for o in c["options"]]
    return opts + ["--split-taxids", ",".join(str(t) for t in listed)]


def check(name, listed, t, err, gz=False):
    gd, c = case(name)
    want, _ = expected(name, listed)
    for key, fn in c["names"].items():
        got = open(os.path.join(t, fn), "rb").read()
        if gz:
            got = splitcases.inflate_bgzf(got)
        assert got == want[key], (name, key, listed, common.first_diff(got.decode("latin1"), want[key].decode("latin1")))
    assert open(os.path.join(t, "out.tsv"), "rb").read() == open(os.path.join(gd, c["tsv"]), "rb").read()
    assert ("Warning: --split-taxids" in err and str(UNKNOWN) in err) == (UNKNOWN in listed), err


def test_the_goldens_hold_what_the_rule_is_about():
    """checked on the golden TSVs alone: reads whose rows fall into both classes under the internal taxon (rows 100, 101, 102)"""
    for name in ("fa_k5", "pe_percent", "pe_bare"):
        listed = selection(name, "internal")
        assert expected(name, listed)[1] >= 20, (name, listed)
    assert selection("fa_k5", "internal") != selection("fa_k5", "leaf")


@pytest.mark.parametrize("what", SELECTIONS)
@pytest.mark.parametrize("name", CASES)
def test_case_on_the_device_text_path(name, what):
    _, c = case(name)
    listed = selection(name, what)
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t, options=options(c, listed))
        assert blocks(err)[0] >= 1 and blocks(err)[1] == 0, err
        assert "batch(es) split on the device" in err
        check(name, listed, t, err)
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t, options=options(c, listed), env={"CF_TEXT_BLOCK": "4096"})
        assert blocks(err)[0] > 4 and blocks(err)[1] == 0, err
        check(name, listed, t, err)


@pytest.mark.parametrize("what", SELECTIONS)
@pytest.mark.parametrize("name", CASES)
def test_case_with_host_io(name, what):
    _, c = case(name)
    listed = selection(name, what)
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t, options=options(c, listed), extra=["--host-io"])
        assert blocks(err) == (0, 0)
        check(name, listed, t, err)


def with_crlf_record(text, fastq):
    """one record in the middle with CR LF line ends"""
    lines = text.split(b"\n")
    starts = list(range(0, len(lines) - 1, 4)) if fastq else [i for i, ln in enumerate(lines) if ln.startswith(b">")]
    k = len(starts) // 2
    for i in range(starts[k], starts[k + 1]):
        lines[i] += b"\r"
    return b"\n".join(lines)


@pytest.mark.parametrize("what", ["internal", "zero"])
@pytest.mark.parametrize("name", CASES)
def test_device_and_host_blocks_mix_in_one_file(name, what):
    _, c = case(name)
    listed = selection(name, what)
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        files = []
        for f in c["reads"]:
            files.append(os.path.join(t, "crlf_" + f))
            open(files[-1], "wb").write(with_crlf_record(open(os.path.join(d, f), "rb").read(), c["format"] == "-q"))
        err = run(c, t, options=options(c, listed), env={"CF_TEXT_BLOCK": "4096"}, reads=files)
        assert blocks(err)[0] > 2 and blocks(err)[1] >= 1, err
        check(name, listed, t, err)


@pytest.mark.parametrize("what", ["internal", "leaf+unknown"])
@pytest.mark.parametrize("name", CASES)
def test_gz_sinks_inflate_to_the_plain_files(name, what):
    _, c = case(name)
    listed = selection(name, what)
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t, options=options(c, listed, gz=True), env={"CF_TEXT_BLOCK": "8192"})
        assert blocks(err)[0] > 2 and blocks(err)[1] == 0, err
        check(name, listed, t, err, gz=True)


def test_case_from_a_bgzf_input():
    name = "fq_k1_trim"
    _, c = case(name)
    listed = selection(name, "internal")
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        f = write_bgzf(os.path.join(t, "reads.fq.gz"), open(os.path.join(d, "reads.fq"), "rb").read())
        err = run(c, t, options=options(c, listed), reads=[f])
        assert members(err) is not None and members(err)[0] >= 1 and members(err)[1] == 0, err
        check(name, listed, t, err)


@pytest.mark.parametrize("options,message", [(["--un", "u.fq", "--split-taxids", ""], "--split-taxids"),
                                             (["--un", "u.fq", "--split-taxids", ","], "--split-taxids"),
                                             (["--split-taxids", "100"], "--un"),
                                             (["--al", "a.fq", "--split-taxids", "100,x7"], "x7"),
                                             (["--al", "a.fq", "--split-taxids", "-5"], "-5")],
                         ids=["empty", "commas-only", "no-sink", "not-a-number", "negative"])
def test_option_errors(options, message):
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        p = subprocess.run([CLI, "-f", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "-S", "o.tsv"] + options, cwd=t,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = p.stderr.decode()
        assert p.returncode != 0 and "split-taxids" in err and message in err, err[-2000:]
        assert "unrecognized option" not in err
        assert not os.path.exists(os.path.join(t, "o.tsv")) and not os.path.exists(os.path.join(t, "u.fq")) and not os.path.exists(os.path.join(t, "a.fq"))
