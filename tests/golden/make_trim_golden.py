#!/usr/bin/env python3
"""Regenerates tests/golden/trim_skip.tar.xz with the compiled, unmodified reference (oracle/_ref, built by oracle/Makefile): its
TSVs and reports for -5 7 -3 11, -s 13, -s 13 -u 40 and all four together over synth_small's reads.fq, reads.fa and r1.fa / r2.fa,
with the default columns and with --out-fmt sam (tests/trimcases.py names the cases).  The archive holds cases.json and those
outputs only: the reads and the index are synth_small.tar.xz's.

Checked while generating: no read of any case is trimmed to nothing (a queryLength of 0 in the reference's output) — empty reads
are the host parser's business and would take their blocks off the device path the tests assert.  A case the reference does not
finish within the time limit is left out and named under "dropped" in cases.json."""
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
import trimcases as T  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "centrifuge-class")


def main():
    d, _ = common.golden("synth_small")
    out = tempfile.mkdtemp()
    scratch = tempfile.mkdtemp()
    cases, dropped = [], []
    for inp in T.INPUTS:
        for lst, args in T.ARG_LISTS:
            for sam in (False, True):
                name = T.case_name(inp, lst, sam)
                fmt, files = T.files_of(d, inp, args, scratch)
                tsv, rep = os.path.join(out, name + ".tsv"), os.path.join(out, name + ".report.tsv")
                cmd = [REF, "-p", "1", fmt, "-x", os.path.join(d, "idx"), "-S", tsv, "--report-file", rep] + args + (["--out-fmt", "sam"] if sam else [])
                cmd += ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
                try:
                    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
                except subprocess.TimeoutExpired:
                    dropped.append({"name": name, "why": "the reference binary does not finish this argument list"})
                    for p in (tsv, rep):
                        if os.path.exists(p):
                            os.remove(p)
                    continue
                rows = open(tsv, "rb").read().split(b"\n")[:-1]
                qlen_col = 8 if sam else 6
                body = [r for r in rows if not r.startswith((b"readID", b"@"))]
                assert body and all(int(r.split(b"\t")[qlen_col]) > 0 for r in body), "%s: a read is trimmed to nothing" % name
                cases.append({"name": name, "input": inp, "list": lst, "args": args, "sam": sam, "reads": [os.path.basename(f) for f in files],
                              "tsv": name + ".tsv", "report": name + ".report.tsv", "rows": len(body)})
    json.dump({"cases": cases, "dropped": dropped,
               "derived": {"reads_long.fa": "synth_small's reads.fa without its records of fewer than %d bases (tests/trimcases.py long_fasta)" % T.MIN_LONG}},
              open(os.path.join(out, "cases.json"), "w"), indent=1)
    dst = os.path.join(HERE, "trim_skip.tar.xz")
    with tarfile.open(dst, "w:xz", preset=9) as t:
        for f in sorted(os.listdir(out)):
            t.add(os.path.join(out, f), arcname=f)
    print(dst, os.path.getsize(dst), "bytes;", len(cases), "cases,", len(dropped), "dropped")


if __name__ == "__main__":
    main()
