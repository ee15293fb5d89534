"""What tests/golden/trim_skip.tar.xz holds (tests/golden/make_trim_golden.py makes it, tests/test_gpu_texttrim.py and
tests/test_gpu_cli_trim.py read it): the reference binary's TSVs and reports for -5 / -3 / -s / -u over synth_small's reads."""
import os

TRIM = ["-5", "7", "-3", "11"]
SKIP = ["-s", "13"]
SKIP_UPTO = ["-s", "13", "-u", "40"]
ALL = TRIM + SKIP_UPTO
ARG_LISTS = [("trim", TRIM), ("skip", SKIP), ("skip_upto", SKIP_UPTO), ("all", ALL)]
# input name -> (format flag, files of synth_small).  reads.fa holds eight reads of 1 to 33 bases (len1 ... len33), of which 7 + 11
# trimmed bases leave nothing: the argument lists that trim run over reads_long.fa — reads.fa without its records of fewer than
# MIN_LONG bases, so that no window is empty and every block stays on the device; the lists that only skip run over reads.fa itself
INPUTS = {"fq": ("-q", ["reads.fq"]), "fa": ("-f", ["reads.fa"]), "pe": ("-f", ["r1.fa", "r2.fa"])}
MIN_LONG = 34
SAM = "QNAME,FLAG,RNAME,POS,MAPQ,CIGAR,RNEXT,PNEXT,TLEN,SEQ,QUAL"                      # --out-fmt sam's columns (centrifuge.cpp:484-520)


def long_fasta(text, min_len=MIN_LONG):
    """the FASTA text without its records of fewer than min_len bases"""
    out = []
    for rec in text.split(b">")[1:]:
        if sum(len(ln) for ln in rec.split(b"\n")[1:]) >= min_len:
            out.append(b">" + rec)
    return b"".join(out)


def files_of(d, inp, args, scratch):
    """the files the case (input, argument list) runs over; reads_long.fa is written into `scratch` when it is needed"""
    fmt, files = INPUTS[inp]
    if inp == "fa" and "-5" in args:
        p = os.path.join(scratch, "reads_long.fa")
        if not os.path.exists(p):
            open(p, "wb").write(long_fasta(open(os.path.join(d, "reads.fa"), "rb").read()))
        return fmt, [p]
    return fmt, [os.path.join(d, f) for f in files]


def case_name(inp, lst, sam):
    return "%s_%s%s" % (inp, lst, "_sam" if sam else "")
