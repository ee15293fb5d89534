"""cf_batch_set_text_columns on the GPU (include/centrifuge_amd.h): a block of FASTA / FASTQ text in, ANY list of columns out as text,
formatted on the device — against what `centrifuge-class --host-io --tab-fmt-cols <the same list>` prints for the same file (the
host's general formatter, itself pinned to the reference binary by tests/test_gpu_cli.py), and against the reference binary where
oracle/_ref is built; the tally the same pass leaves gives the golden report whatever the columns."""
import os
import subprocess
import tempfile

import pytest

import common
from centrifuge_amd import capi
from oracle import oracle as O
from test_async_abi import dev_index

pytestmark = pytest.mark.gpu
CLI = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-class")
LIST_A = "readID,taxID,taxRank,taxName,numMatches,readSeq,readQual"                          # tests/test_gpu_cli.py:46
LIST_B = "QNAME,CIGAR,FLAG,RNAME,RNEXT,TLEN,SEQ1,QUAL2,readSeq2,taxLevel"                    # tests/test_gpu_cli.py:48
SAM = "QNAME,FLAG,RNAME,POS,MAPQ,CIGAR,RNEXT,PNEXT,TLEN,SEQ,QUAL"
REPEATED = "readSeq,readSeq,taxID,taxID,readQual1,readQual1"
WIDE32 = ",".join(("readID,seqID,taxID,score,2ndBestScore,hitLength,queryLength,numMatches,taxRank,taxName,readSeq,readQual,readSeq1,readQual1,"
                   "readSeq2,readQual2,CIGAR,FLAG," * 2).split(",")[:32])
DEFAULT = "readID,seqID,taxID,score,2ndBestScore,hitLength,queryLength,numMatches"
PROGRAMS = [REPEATED, LIST_A, LIST_B, SAM, WIDE32, DEFAULT]
INPUTS = [("k5", capi.TEXT_FASTA, "-f"), ("fastq", capi.TEXT_FASTQ, "-q"), ("pe_k5", capi.TEXT_FASTA, "-f")]


def cli_rows(exe, fmt, files, cols, t, extra=()):
    """the rows (no header line) the command prints for that list of columns"""
    out = os.path.join(t, "o.tsv")
    reads = ["-U", files[0]] if len(files) == 1 else ["-1", files[0], "-2", files[1]]
    p = subprocess.Popen([exe, fmt, "-x", os.path.join(os.path.dirname(files[0]), "idx")] + reads + list(extra) + ["--tab-fmt-cols", cols, "-S", out,
                          "--report-file", os.path.join(t, "o.rep")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        _, err = p.communicate(timeout=180)
    except subprocess.TimeoutExpired:
        p.kill()
        _, err = p.communicate()
        raise AssertionError("the run hangs: %s\n%s" % (exe, (err or "")[-4000:]))
    assert p.returncode == 0, err
    return open(out, "rb").read().split(b"\n", 1)[1]


@pytest.mark.parametrize("name,tfmt,flag", INPUTS, ids=[i[0] for i in INPUTS])
def test_any_columns_come_back_as_the_host_formatter_prints_them(name, tfmt, flag):
    d, cases = common.golden("synth_small")
    c = [x for x in cases if x["name"] == name][0]
    files = [os.path.join(d, f) for f in c["reads"]]
    texts = [open(f, "rb").read() for f in files]
    ix = dev_index("synth_small")
    clf = capi.Classifier(ix)
    clf.reset_counts()
    slot = capi.Slot(clf)
    slot.set_result_format(capi.RESULTS_NARROW)

    def device_rows():
        info = slot.submit_text(texts[0], tfmt, text2=texts[1] if len(texts) == 2 else None)
        assert not info.irregular
        return slot.wait_text()
    golden_rows = open(os.path.join(d, c["tsv"]), "rb").read().split(b"\n", 1)[1]
    first = True
    with tempfile.TemporaryDirectory() as t:
        for cols in PROGRAMS:
            slot.set_text_columns(cols.split(","))
            got, tuples, _ = device_rows()
            want = cli_rows(CLI, flag, files, cols, t, extra=["--host-io"])
            assert got == want, (cols, common.first_diff(got.decode("latin1"), want.decode("latin1")))
            if O.have_ref():
                ref = cli_rows(os.path.join(O.REF_DIR, "centrifuge-class"), flag, files, cols, t)
                assert got == ref, (cols, common.first_diff(got.decode("latin1"), ref.decode("latin1")))
            if cols == DEFAULT:
                assert got == golden_rows
            if first:
                # the report from what the device tallied alone, under a program that is not the default one
                rep = capi.Report(ix)
                rep.add_tuples(tuples)
                n_reads, n_unique = clf.counts()
                rep.adopt_device_tally(n_reads, n_unique, clf.counts_single())
                rep.write(os.path.join(t, "r.tsv"))
                assert open(os.path.join(t, "r.tsv")).read() == open(os.path.join(d, c["report"])).read()
                rep.close()
                first = False
                # a change of the program behind a batch's first wait does not format that batch again
                slot.set_text_columns(["readID"])
                assert slot.wait_text()[0] == got
    # a list that is refused leaves the program before it in force
    slot.set_text_columns(LIST_A.split(","))
    want_a = device_rows()[0]
    with pytest.raises(capi.CfError):
        slot.set_text_columns(["readID"] * 33)
    with pytest.raises(capi.CfError):
        slot.set_text_columns([capi.COL_READ_ID, 99])
    with pytest.raises(capi.CfError):
        slot.set_text_columns(["readID", "noSuchColumn"])
    assert device_rows()[0] == want_a and want_a != golden_rows
    # names and codes are the same thing; no columns at all: today's default text
    slot.set_text_columns([capi.text_column_of(n) for n in LIST_A.split(",")])
    assert device_rows()[0] == want_a
    slot.set_text_columns([])
    assert device_rows()[0] == golden_rows
    slot.close(); clf.close()
