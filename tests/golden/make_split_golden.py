#!/usr/bin/env python3
"""Regenerates tests/golden/read_split.tar.xz with the reference's OWN wrapper script: `centrifuge` (Perl) is copied, for the run
only, into a temporary directory beside the compiled, unmodified reference binary (oracle/_ref/centrifuge-class, built by
oracle/Makefile) and run with -p 1 over synth_small's reads.fa, reads.fq and r1.fa / r2.fa with --un / --al and --un-conc /
--al-conc (the %, extension and bare forms of the name), under -k 1 and the default -k, and once with -5 7 -3 11.  The archive holds
cases.json, the split files and the TSVs only: the reads and the index are synth_small.tar.xz's.

Checked while generating: every case has classified AND unclassified reads (both files of a pair of options are fed), and no read
name holds "unclassified" (the wrapper decides by that word on the whole line; this package by the query having no assignment)."""
import json
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
WRAPPER = os.path.join(os.environ.get("CENTRIFUGE_REFERENCE", "/root/reference"), "centrifuge")     # (the tree oracle/Makefile builds oracle/_ref from)

# name, format flag, read files, the options' form (file names relative to the run's directory), further arguments
CASES = [
    ("fa_k5", "-f", ["reads.fa"], "plain", []),
    ("fa_k1", "-f", ["reads.fa"], "plain", ["-k", "1"]),
    ("fq_k5", "-q", ["reads.fq"], "plain", []),
    ("fq_k1_trim", "-q", ["reads.fq"], "plain", ["-k", "1", "-5", "7", "-3", "11"]),
    ("pe_percent", "-f", ["r1.fa", "r2.fa"], "percent", []),
    ("pe_ext_k1", "-f", ["r1.fa", "r2.fa"], "ext", ["-k", "1"]),
    ("pe_bare", "-f", ["r1.fa", "r2.fa"], "bare", []),
]
FORMS = {"plain": (["--un", "un.fq", "--al", "al.fq"], {"un": "un.fq", "al": "al.fq"}),
         "percent": (["--un-conc", "un_%.fq", "--al-conc", "al_%.fq"], {"un1": "un_1.fq", "un2": "un_2.fq", "al1": "al_1.fq", "al2": "al_2.fq"}),
         "ext": (["--un-conc", "unc.fq", "--al-conc", "alc.fq"], {"un1": "unc.1.fq", "un2": "unc.2.fq", "al1": "alc.1.fq", "al2": "alc.2.fq"}),
         "bare": (["--un-conc", "unc", "--al-conc", "alc"], {"un1": "unc.1", "un2": "unc.2", "al1": "alc.1", "al2": "alc.2"})}


def main():
    d, _ = common.golden("synth_small")
    out = tempfile.mkdtemp()
    tools = tempfile.mkdtemp()
    shutil.copy(WRAPPER, os.path.join(tools, "centrifuge"))              # (for the run only: never into the repository)
    os.symlink(os.path.join(REF_DIR, "centrifuge-class"), os.path.join(tools, "centrifuge-class"))
    cases = []
    for name, fmt, reads, form, extra in CASES:
        run = tempfile.mkdtemp()
        opts, files = FORMS[form]
        cmd = ["perl", os.path.join(tools, "centrifuge"), "-p", "1", fmt, "-x", os.path.join(d, "idx"), "-S", "out.tsv", "--report-file", "rep.tsv"] + extra + opts
        cmd += ["-U", os.path.join(d, reads[0])] if len(reads) == 1 else ["-1", os.path.join(d, reads[0]), "-2", os.path.join(d, reads[1])]
        subprocess.run(cmd, check=True, cwd=run, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
        tsv = open(os.path.join(run, "out.tsv"), "rb").read()
        body = tsv.split(b"\n")[1:-1]
        assert not any(b"unclassified" in ln.split(b"\t")[0] for ln in body), "%s: a read name holds 'unclassified'" % name
        shutil.copy(os.path.join(run, "out.tsv"), os.path.join(out, name + ".tsv"))
        rec = {}
        for key, fn in files.items():
            data = open(os.path.join(run, fn), "rb").read()
            assert data, "%s: nothing went to %s — the case needs classified and unclassified reads" % (name, fn)
            open(os.path.join(out, name + "." + key), "wb").write(data)
            rec[key] = name + "." + key
        cases.append({"name": name, "format": fmt, "reads": reads, "form": form, "args": extra, "options": opts, "names": files,
                      "tsv": name + ".tsv", "files": rec, "rows": len(body)})
    json.dump({"cases": cases, "made_by": "the reference's wrapper script `centrifuge` around oracle/_ref/centrifuge-class, -p 1"},
              open(os.path.join(out, "cases.json"), "w"), indent=1)
    dst = os.path.join(HERE, "read_split.tar.xz")
    with tarfile.open(dst, "w:xz", preset=9) as t:
        for f in sorted(os.listdir(out)):
            t.add(os.path.join(out, f), arcname=f)
    print(dst, os.path.getsize(dst), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
