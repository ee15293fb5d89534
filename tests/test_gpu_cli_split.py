"""--un / --al / --un-conc / --al-conc of centrifuge-class against the files the reference's own wrapper script wrote
(tests/golden/read_split.tar.xz, made by tests/golden/make_split_golden.py): byte-identical split files and TSV on the device text
path (the block counts of -t prove the path), with many small blocks (the per-file order chains), with --host-io (splitRange), with
one CR LF record spliced in (device and host blocks in one file), the -gz forms, --out-bgzf beside them, the name rules and the
option errors.  On the parent commit the options were swallowed and no file was written: every test here fails there."""
import os
import re
import subprocess
import tempfile

import pytest

import common
import splitcases

pytestmark = pytest.mark.gpu
CLI = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-class")


def cases():
    d, c = common.golden("read_split")
    return d, c["cases"]


def run(c, t, extra=(), env=None, options=None, reads=None):
    d, _ = common.golden("synth_small")
    files = reads or [os.path.join(d, f) for f in c["reads"]]
    cmd = [CLI, "-t", c["format"], "-x", os.path.join(d, "idx"), "-S", "out.tsv", "--report-file", "rep.tsv"] + c["args"] + list(options if options is not None else c["options"]) + list(extra)
    cmd += ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, cwd=t, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p.stderr.decode()


def blocks(err):
    m = re.search(r"Device text path: (\d+) block\(s\) parsed and printed on the device, (\d+) on the host", err)
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def check_files(c, gd, t, gz=False, names=None):
    for key, fn in (names or c["names"]).items():
        got = open(os.path.join(t, fn), "rb").read()
        if gz:
            got = splitcases.inflate_bgzf(got)
        want = open(os.path.join(gd, c["files"][key]), "rb").read()
        assert got == want, (c["name"], key, common.first_diff(got.decode("latin1"), want.decode("latin1")))
    assert open(os.path.join(t, "out.tsv"), "rb").read() == open(os.path.join(gd, c["tsv"]), "rb").read()


CASE_NAMES = ["fa_k5", "fa_k1", "fq_k5", "fq_k1_trim", "pe_percent", "pe_ext_k1", "pe_bare"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_golden_case_on_the_device_text_path(name):
    gd, cs = cases()
    assert [c["name"] for c in cs] == CASE_NAMES
    c = [x for x in cs if x["name"] == name][0]
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t)
        assert blocks(err)[0] >= 1 and blocks(err)[1] == 0, err
        assert "batch(es) split on the device" in err
        check_files(c, gd, t)
    # many blocks: the per-file chains hand out the places in block order
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t, env={"CF_TEXT_BLOCK": "4096"})
        assert blocks(err)[0] > 4 and blocks(err)[1] == 0, err
        check_files(c, gd, t)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_golden_case_with_host_io(name):
    gd, cs = cases()
    c = [x for x in cs if x["name"] == name][0]
    with tempfile.TemporaryDirectory() as t:
        err = run(c, t, extra=["--host-io"])
        assert blocks(err) == (0, 0)
        check_files(c, gd, t)


def test_device_and_host_blocks_mix_in_one_file():
    """one record with CR LF line ends: its block is the host parser's, the blocks around it the device's; same files"""
    gd, cs = cases()
    c = [x for x in cs if x["name"] == "fq_k5"][0]
    d, _ = common.golden("synth_small")
    lines = open(os.path.join(d, "reads.fq"), "rb").read().split(b"\n")
    k = 4 * (len(lines) // 8)
    for i in range(k, k + 4):
        lines[i] += b"\r"
    with tempfile.TemporaryDirectory() as t:
        open(os.path.join(t, "crlf.fq"), "wb").write(b"\n".join(lines))
        err = run(c, t, env={"CF_TEXT_BLOCK": "4096"}, reads=[os.path.join(t, "crlf.fq")])
        assert blocks(err)[0] > 2 and blocks(err)[1] >= 1, err
        check_files(c, gd, t)


@pytest.mark.parametrize("name", ["fq_k5", "pe_ext_k1"])
@pytest.mark.parametrize("extra", [[], ["--host-io"], ["--out-bgzf"]], ids=["device", "host-io", "out-bgzf"])
def test_gz_forms_inflate_to_the_plain_files(name, extra):
    gd, cs = cases()
    c = [x for x in cs if x["name"] == name][0]
    opts = [o + "-gz" if o.startswith("--") else o for o in c["options"]]
    with tempfile.TemporaryDirectory() as t:
        run(c, t, extra=extra, options=opts, env={"CF_TEXT_BLOCK": "8192"})
        if "--out-bgzf" in extra:
            z = open(os.path.join(t, "out.tsv"), "rb").read()
            open(os.path.join(t, "out.tsv"), "wb").write(splitcases.inflate_bgzf(z))
        check_files(c, gd, t, gz=True)


def test_a_gz_file_beside_a_plain_one():
    gd, cs = cases()
    c = [x for x in cs if x["name"] == "fa_k5"][0]
    with tempfile.TemporaryDirectory() as t:
        run(c, t, options=["--un-gz", "un.fq", "--al", "al.fq"])
        assert splitcases.inflate_bgzf(open(os.path.join(t, "un.fq"), "rb").read()) == open(os.path.join(gd, c["files"]["un"]), "rb").read()
        assert open(os.path.join(t, "al.fq"), "rb").read() == open(os.path.join(gd, c["files"]["al"]), "rb").read()


def test_name_rules_and_files_that_stay_empty():
    gd, cs = cases()
    with tempfile.TemporaryDirectory() as t:
        os.mkdir(os.path.join(t, "dir"))
        c = [x for x in cs if x["name"] == "fa_k5"][0]
        # a directory takes un-seqs / al-seqs; unpaired reads never reach the -conc files, which are created all the same
        run(c, t, options=["--un", "dir", "--al", "dir", "--un-conc", "dir", "--al-conc", "x.y.fq"])
        check_files(c, gd, t, names={"un": "dir/un-seqs", "al": "dir/al-seqs"})
        for fn in ("dir/un-conc-mate.1", "dir/un-conc-mate.2", "x.y.1.fq", "x.y.2.fq"):
            assert os.path.getsize(os.path.join(t, fn)) == 0
        c = [x for x in cs if x["name"] == "pe_bare"][0]
        run(c, t, options=["--un-conc", "dir", "--al-conc", "m%", "--un", "u.fq"])
        check_files(c, gd, t, names={"un1": "dir/un-conc-mate.1", "un2": "dir/un-conc-mate.2", "al1": "m1", "al2": "m2"})
        assert os.path.getsize(os.path.join(t, "u.fq")) == 0
    for path in ("a/b%.fq", "a/b.fq", "a.dir/b", "b"):
        assert splitcases.conc_names(path)[0] != splitcases.conc_names(path)[1]


@pytest.mark.parametrize("options", [["--un", "x.fq", "--al", "x.fq"], ["--un", "m.1.fq", "--un-conc", "m.fq"], ["--un-conc", "y%", "--al-conc-gz", "./y%"]])
def test_two_options_that_name_one_file_are_an_option_error(options):
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        p = subprocess.run([CLI, "-f", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "-S", "o.tsv"] + options, cwd=t,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode != 0 and "name the same file" in p.stderr.decode(), p.stderr.decode()[-2000:]


@pytest.mark.parametrize("opt", ["--un-bz2", "--al-bz2", "--un-conc-bz2", "--al-conc-bz2"])
def test_bz2_forms_are_option_errors(opt):
    d, _ = common.golden("synth_small")
    with tempfile.TemporaryDirectory() as t:
        p = subprocess.run([CLI, "-f", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), opt, "x", "-S", "o.tsv"], cwd=t,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode != 0 and (opt[:-4] + "-gz") in p.stderr.decode()
        assert not os.path.exists(os.path.join(t, "x"))
