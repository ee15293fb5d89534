#!/usr/bin/env python3
"""Regenerates tests/golden/build_edges.json with the compiled, unmodified reference builder (oracle/_ref/centrifuge-build-bin, made by
`python -c "from oracle import oracle as O; O.build()"`): for every case of tests/buildcases.py the sha256 of the generated genomes.fa,
the builder's options and exit status and, where it accepted the input, the size and sha256 of idx.{1,2,3,4}.cf.  Hashes and sizes
only: the index files themselves are not kept (the ftab alone is 8 MB at the default width).  Runs on the CPU.

Only a case marked may_refuse in the table may be refused by the reference; any other refusal stops the script."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import buildcases as B  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    assert O.have_ref(), "oracle/_ref is not built"
    cases = {}
    for c in B.CASES:
        with tempfile.TemporaryDirectory() as d:
            rec = B.run_reference(c, d)
        assert rec["exit"] == 0 or c.may_refuse, "%s: the reference refuses a case it must accept (exit %d)" % (c.name, rec["exit"])
        cases[c.name] = rec
        print(c.name, "accepted" if rec["exit"] == 0 else "refused (exit %d)" % rec["exit"], flush=True)
    with open(B.GOLDEN_JSON, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    n_ok = sum(1 for r in cases.values() if r["exit"] == 0)
    print(B.GOLDEN_JSON, "%d cases: %d accepted, %d refused" % (len(cases), n_ok, len(cases) - n_ok))


if __name__ == "__main__":
    main()
