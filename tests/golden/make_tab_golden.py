#!/usr/bin/env python3
"""Regenerates tests/golden/tab_reads.tar.xz with the compiled, unmodified reference (oracle/_ref, built by oracle/Makefile): its
TSVs and reports for synth_small's reads handed over as tabbed files — plain, with -5 7 -3 11 (over the reads of at least 34 bases),
with -s 13 -u 40 and with -k 1, with the default columns and with --out-fmt sam.  tests/tabcases.py says by which command lines
the reference binary can read these reads at all (it ignores the files a tabbed option names) and makes the inputs; the archive
holds cases.json and the outputs only.  Also recorded: the message and exit code for one quality string that is a character short.

Checked while generating: no case has a queryLength of 0, and `--tab5 <file>` alone still makes the reference print nothing but
the header (the day that changes, the cases can be recorded from the pair lines themselves)."""
import json
import os
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common  # noqa: E402
import tabcases as T  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "centrifuge-class")


def main():
    d, _ = common.golden("synth_small")
    out, scratch = tempfile.mkdtemp(), tempfile.mkdtemp()
    cases = []
    for inp in T.INPUTS:
        for lst, args in T.ARG_LISTS:
            se, pe = T.records(d, T.MIN_LONG if "-5" in args else 0)
            files = []
            for i, text in enumerate(T.ref_files(inp, se, pe)):
                files.append(os.path.join(scratch, "m%d.tab" % i))
                open(files[-1], "wb").write(text)
            for sam in (False, True):
                name = T.case_name(inp, lst, sam)
                tsv, rep = os.path.join(out, name + ".tsv"), os.path.join(out, name + ".report.tsv")
                cmd = [REF, "-p", "1", "-x", os.path.join(d, "idx"), "-S", tsv, "--report-file", rep, "--tab5", files[0]] + args + (["--out-fmt", "sam"] if sam else [])
                cmd += ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
                rows = open(tsv, "rb").read().split(b"\n")[:-1]
                body = [r for r in rows if not r.startswith((b"readID", b"@"))]
                assert body and all(int(r.split(b"\t")[8 if sam else 6]) > 0 for r in body), "%s: a read is trimmed to nothing" % name
                cases.append({"name": name, "input": inp, "list": lst, "args": args, "sam": sam, "tsv": name + ".tsv", "report": name + ".report.tsv", "rows": len(body)})
    # the reference reads no file a tabbed option names
    se, pe = T.records(d)
    p = os.path.join(scratch, "pe.tab5")
    open(p, "wb").write(T.text_of("pe5", se, pe))
    t = os.path.join(scratch, "alone.tsv")
    subprocess.run([REF, "-p", "1", "-x", os.path.join(d, "idx"), "-S", t, "--report-file", os.path.join(scratch, "alone.rep"), "--tab5", p], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    assert len(open(t, "rb").read().split(b"\n")) == 2, "the reference now reads --tab5 files: record the cases from the pair lines"
    # one quality string a character short
    bad = T.text_of("se", se, pe).split(b"\n")
    f = bad[1].split(b"\t")
    assert f[0] == T.BAD_QUAL["read"].encode()
    bad[1] = b"\t".join([f[0], f[1], f[2][:-1]])
    p = os.path.join(scratch, "bad.tab5")
    open(p, "wb").write(b"\n".join(bad))
    r = subprocess.run([REF, "-p", "1", "-x", os.path.join(d, "idx"), "-S", t, "--report-file", os.path.join(scratch, "bad.rep"), "--tab5", p, "-U", p], capture_output=True, timeout=120)
    err = [ln for ln in r.stderr.decode().split("\n") if ln.startswith("Error: Read")]
    assert r.returncode == T.BAD_QUAL["reference_returncode"] and err == [T.BAD_QUAL["stderr"]], (r.returncode, r.stderr)
    json.dump({"cases": cases, "bad_qual": T.BAD_QUAL}, open(os.path.join(out, "cases.json"), "w"), indent=1)
    dst = os.path.join(HERE, "tab_reads.tar.xz")
    with tarfile.open(dst, "w:xz", preset=9) as t:
        for f in sorted(os.listdir(out)):
            t.add(os.path.join(out, f), arcname=f)
    print(dst, os.path.getsize(dst), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
