#!/usr/bin/env python3
"""Regenerates tests/golden/classify_edges.json with the compiled, unmodified reference (oracle/_ref: centrifuge-build-bin and
centrifuge-class): for every case of tests/classifycases.py the index is built by the reference builder (buildcases.run_reference)
and the case's reads are classified by the reference binary (oracle.ref_classify) with -k 5 and -k 1, on the d-group also with
-k 50 --min-hitlen 15, and as mates where the case has them.  The record holds the sha256 of the reads' FASTA, and per run the
reference's exit status and the sha256 and line count of its TSV and report: results only.  Runs on the CPU.

A case the reference cannot build or classify (non-zero status, or ended by a signal) is recorded as `refused` with that status and
leaves the comparisons; the script stops when fewer than half of a group or fewer than 85 % of all cases are left."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import buildcases as B  # noqa: E402
import classifycases as K  # noqa: E402
from oracle import oracle as O  # noqa: E402


def digest(path):
    raw = open(path, "rb").read()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "rows": raw.count(b"\n")}


def run_case(c, d):
    """the reference over one case in directory d -> its record"""
    rec = {"reads_sha256": c.fasta_sha256(), "n_reads": len(c.reads), "build_args": c.build.ref_args}
    built = B.run_reference(c.build, d)
    if built["exit"] != 0:
        rec["refused"] = {"step": "build", "exit": built["exit"]}
        return rec
    with open(os.path.join(d, "reads.fa"), "wb") as f:
        f.write(K.fasta_bytes(c.reads))
    if c.mates:
        with open(os.path.join(d, "r2.fa"), "wb") as f:
            f.write(K.fasta_bytes(c.mate2))
    rec["runs"] = {}
    for rid, args, paired in c.runs():
        tsv, rep = os.path.join(d, rid + ".tsv"), os.path.join(d, rid + ".rep")
        src = dict(m1=os.path.join(d, "reads.fa"), m2=os.path.join(d, "r2.fa")) if paired else dict(u=os.path.join(d, "reads.fa"))
        try:
            O.ref_classify(os.path.join(d, "idx"), tsv, rep, extra=args, **src)
        except subprocess.CalledProcessError as e:
            rec["refused"] = {"step": rid, "exit": e.returncode}
            del rec["runs"]
            return rec
        rec["runs"][rid] = {"args": args, "exit": 0, "tsv": digest(tsv), "report": digest(rep)}
    return rec


def main():
    assert O.have_ref(), "oracle/_ref is not built"
    cases = {}
    for c in K.CASES:
        with tempfile.TemporaryDirectory() as d:
            cases[c.name] = run_case(c, d)
        r = cases[c.name]
        print(c.name, "refused (%s: exit %d)" % (r["refused"]["step"], r["refused"]["exit"]) if "refused" in r else "kept", flush=True)
    kept = [n for n in K.NAMES if "refused" not in cases[n]]
    for g, names in K.by_group(K.NAMES).items():
        k = [n for n in names if n in kept]
        assert 2 * len(k) >= len(names), "group %s keeps %d of %d cases" % (g, len(k), len(names))
    assert len(kept) >= 0.85 * len(K.NAMES), "%d of %d cases kept" % (len(kept), len(K.NAMES))
    with open(K.GOLDEN_JSON, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(K.GOLDEN_JSON, "%d cases: %d kept, %d refused" % (len(cases), len(kept), len(cases) - len(kept)))


if __name__ == "__main__":
    main()
