"""centrifuge-kreport reads what centrifuge-class --out-bgzf writes: a classification file, its gzip form and its BGZF form
(concatenated gzip members, the empty one at the end) give the same bytes."""
import gzip
import os
import subprocess
import tempfile

import pytest

import common
from test_gpu_cli_bgzf import write_bgzf

KREPORT = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-kreport")


@pytest.mark.parametrize("name,opts", [("k5", []), ("pe_k5", []), ("fastq", ["--show-zeros"]), ("k5", ["--min-score", "300"])])
def test_plain_gzip_and_bgzf_inputs_agree(name, opts):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    tsv = open(os.path.join(d, c["tsv"]), "rb").read()
    idx = os.path.join(d, "idx")
    with tempfile.TemporaryDirectory() as t:
        plain, gz, bg, small = (os.path.join(t, f) for f in ("o.tsv", "o.tsv.gz", "o.bgzf.gz", "o.small.gz"))
        open(plain, "wb").write(tsv)
        open(gz, "wb").write(gzip.compress(tsv))
        write_bgzf(bg, tsv)
        write_bgzf(small, tsv, 192)                              # many members, lines cut anywhere
        want = subprocess.run([KREPORT, "-x", idx] + opts + [plain], capture_output=True)
        assert want.returncode == 0 and want.stdout.count(b"\n") > 3
        for p in (gz, bg, small):
            got = subprocess.run([KREPORT, "-x", idx] + opts + [p], capture_output=True)
            assert got.returncode == 0 and got.stdout == want.stdout, p
        # ... through stdin, and a plain file behind a compressed one (Perl's <> over both)
        got = subprocess.run([KREPORT, "-x", idx] + opts, stdin=open(bg, "rb"), capture_output=True)
        assert got.returncode == 0 and got.stdout == want.stdout
        two = subprocess.run([KREPORT, "-x", idx] + opts + [plain, plain], capture_output=True)
        got = subprocess.run([KREPORT, "-x", idx] + opts + [bg, plain], capture_output=True)
        assert got.returncode == 0 and got.stdout == two.stdout and two.stdout != want.stdout
