"""centrifuge-class over the device text path with columns other than the default eight (--tab-fmt-cols, --out-fmt sam): plain FASTA /
FASTQ files and mates go up as text and the rows come back as text, formatted on the device — the same bytes as the host parser
and the host's general formatter give (--host-io), as the reference binary gives; a block with a record outside the plain form is
parsed and formatted on the host, and the two formatters' text mixes in one file."""
import os
import tempfile

import pytest

import common
from oracle import oracle as O
from test_gpu_cli_text import CLI, blocks, run

pytestmark = pytest.mark.gpu
LIST_A = ["--tab-fmt-cols", "readID,taxID,taxRank,taxName,numMatches,readSeq,readQual"]                          # tests/test_gpu_cli.py:46
LIST_B = ["--tab-fmt-cols", "QNAME,CIGAR,FLAG,RNAME,RNEXT,TLEN,SEQ1,QUAL2,readSeq2,taxLevel"]                    # tests/test_gpu_cli.py:48
SAM = ["--out-fmt", "sam"]
INPUTS = [("fasta", "-f", ["reads.fa"]), ("fastq", "-q", ["reads.fq"]), ("mates", "-f", ["r1.fa", "r2.fa"])]


def read_args(files):
    return ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]


def with_one_crlf_record(src, fastq):
    """the file with the record in its middle rewritten with CR LF line ends: the block that holds it is not in the plain form"""
    lines = src.split(b"\n")[:-1]
    per = 4 if fastq else 2
    assert len(lines) % per == 0
    k = (len(lines) // per // 2) * per
    return b"\n".join(lines[:k]) + b"\n" + b"\r\n".join(lines[k:k + per]) + b"\r\n" + b"\n".join(lines[k + per:]) + b"\n"


@pytest.mark.parametrize("cols", [LIST_A, LIST_B, SAM], ids=["names_and_reads", "sam_names", "sam"])
@pytest.mark.parametrize("name,fmt,reads", INPUTS, ids=[i[0] for i in INPUTS])
def test_other_columns_take_the_text_path_and_print_the_host_s_bytes(name, fmt, reads, cols):
    d, _ = common.golden("synth_small")
    files = [os.path.join(d, f) for f in reads]
    base = [fmt, "-t", "-p", "4", "-x", os.path.join(d, "idx")]
    with tempfile.TemporaryDirectory() as t:
        args = base + read_args(files) + cols
        want = run(args + ["--host-io"], t, tag="h")
        assert blocks(want[2]) is None
        got = run(args, t)
        assert got[:2] == want[:2], common.first_diff(got[0].decode("latin1"), want[0].decode("latin1"))
        nb = blocks(got[2])
        assert nb and nb[0] >= 1 and nb[1] == 0, got[2]
        if O.have_ref():
            ref = run([fmt, "-x", os.path.join(d, "idx")] + read_args(files) + cols, t, exe=os.path.join(O.REF_DIR, "centrifuge-class"), tag="ref")
            assert got[:2] == ref[:2], common.first_diff(got[0].decode("latin1"), ref[0].decode("latin1"))
        # many small blocks
        got = run(args, t, env={"CF_TEXT_BLOCK": "4096"})
        assert got[:2] == want[:2], common.first_diff(got[0].decode("latin1"), want[0].decode("latin1"))
        nb = blocks(got[2])
        assert nb and nb[0] > 10 and nb[1] == 0, got[2]
        # one CR LF record spliced in: its block takes the host parser and the host formatter, the others the device's
        odd = [os.path.join(t, "odd%d" % i) for i in range(len(files))]
        for i, (src, dst) in enumerate(zip(files, odd)):
            text = open(src, "rb").read()
            open(dst, "wb").write(with_one_crlf_record(text, fmt == "-q") if i == 0 else text)
        args = base + read_args(odd) + cols
        want = run(args + ["--host-io"], t, tag="h")
        got = run(args, t, env={"CF_TEXT_BLOCK": "4096"})
        assert got[:2] == want[:2], common.first_diff(got[0].decode("latin1"), want[0].decode("latin1"))
        nb = blocks(got[2])
        assert nb and nb[0] >= 3 and nb[1] >= 1, got[2]


def test_more_columns_than_the_device_takes_keep_the_host_pool():
    d, _ = common.golden("synth_small")
    cols = ",".join(["readID", "taxID", "readSeq"] * 11)                     # 33
    args = ["-f", "-t", "-p", "4", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "--tab-fmt-cols", cols]
    with tempfile.TemporaryDirectory() as t:
        got = run(args, t)
        want = run(args + ["--host-io"], t, tag="h")
        assert got[:2] == want[:2] and (blocks(got[2]) is None or blocks(got[2])[0] == 0)
        assert got[0].split(b"\n")[1].count(b"\t") == 32
