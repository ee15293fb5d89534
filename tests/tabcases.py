"""What tests/golden/tab_reads.tar.xz holds (tests/golden/make_tab_golden.py makes it; tests/test_tab_ingest.py and
tests/test_gpu_cli_tab.py read it) and the tabbed inputs of those tests, made from synth_small's reads at test time.

The reference BINARY reads no file named by --tab5 / --12 / --tab6: its loop over the inputs (centrifuge.cpp:3007-3060) hands
PairedPatternSource::setupPatternSources the -1 / -2 and -U files only, so `--tab5 f` alone prints the header and nothing else.  What
a tabbed option does there is switch the format of the -U / -1 / -2 files, which TabbedPatternSource::read then takes a line a read.
The recorded outputs are therefore the reference's for the SAME READS over the command lines it can read them by —
    se           -U se.tab5 --tab5 se.tab5                   (three fields a line)
    pe5 / pe6    -1 m1.tab5 -2 m2.tab5 --tab5 m1.tab5        (the pair lines' halves, three fields a line each: ref_files)
— with the same parser functions (parseName, parseSeq, parseQuals), seeds and classification as a pair line would get from
TabbedPatternSource::readPair.  The mixed file has no such command line: its expected rows are put together from the recorded
cases read by read (mix_rows)."""
import os

TRIM = ["-5", "7", "-3", "11"]
SKIP_UPTO = ["-s", "13", "-u", "40"]
ARG_LISTS = [("plain", []), ("trim", TRIM), ("skip_upto", SKIP_UPTO), ("k1", ["-k", "1"])]
INPUTS = ["se", "pe5", "pe6"]
MIN_LONG = 34                                              # the trimming lists run over reads of at least that many bases
BAD_QUAL = {"name": "bad_qual", "read": "r1_20", "stderr": "Error: Read r1_20 has more read characters than quality values.", "returncode": 1,
            "reference_returncode": -6}      # the reference throws from a worker thread and aborts; centrifuge-class ends with 1, as for FASTQ


def fastq_records(text):
    ln = text.split(b"\n")[:-1]
    return [(ln[i][1:], ln[i + 1], ln[i + 3]) for i in range(0, len(ln), 4)]


def fasta_records(text):
    out = []
    for rec in text.split(b">")[1:]:
        lines = rec.split(b"\n")
        seq = b"".join(lines[1:])
        out.append((lines[0], seq, b"I" * len(seq)))
    return out


def records(d, min_len=0):
    """(singles, pairs) of synth_small: reads.fq's records, and r1.fa / r2.fa's side by side (names as the files have them: x/1, x/2)"""
    se = fastq_records(open(os.path.join(d, "reads.fq"), "rb").read())
    r1 = fasta_records(open(os.path.join(d, "r1.fa"), "rb").read())
    r2 = fasta_records(open(os.path.join(d, "r2.fa"), "rb").read())
    pe = list(zip(r1, r2))
    if min_len:
        se = [r for r in se if len(r[1]) >= min_len]
        pe = [p for p in pe if len(p[0][1]) >= min_len and len(p[1][1]) >= min_len]
    return se, pe


def base(name):
    return name[:-2] if name[-2:] in (b"/1", b"/2") else name


def single_line(r):
    return b"\t".join(r) + b"\n"


def pair_line(p, tab6):
    a, b = p
    if tab6:
        return b"\t".join([a[0], a[1], a[2], b[0], b[1], b[2]]) + b"\n"
    return b"\t".join([base(a[0]), a[1], a[2], b[1], b[2]]) + b"\n"


def text_of(inp, se, pe):
    """the bytes of input `inp`: se, pe5, pe6, or mix — a tab5 file of runs of 7 pair lines and 5 three-field lines in turn"""
    if inp == "se":
        return b"".join(single_line(r) for r in se)
    if inp in ("pe5", "pe6"):
        return b"".join(pair_line(p, inp == "pe6") for p in pe)
    out, i, j = [], 0, 0
    while i < len(pe) or j < len(se):
        out += [pair_line(p, False) for p in pe[i:i + 7]]; i += 7
        out += [single_line(r) for r in se[j:j + 5]]; j += 5
    return b"".join(out)


def mix_kinds(se, pe):
    """the records of the mixed file in file order: ("pe", index) / ("se", index)"""
    out, i, j = [], 0, 0
    while i < len(pe) or j < len(se):
        out += [("pe", k) for k in range(i, min(i + 7, len(pe)))]; i += 7
        out += [("se", k) for k in range(j, min(j + 5, len(se)))]; j += 5
    return out


def ref_files(inp, se, pe):
    """the three-field files the reference binary reads the same reads from: [unpaired] or [mates 1, mates 2]"""
    if inp == "se":
        return [text_of("se", se, pe)]
    nm = (lambda r: r[0]) if inp == "pe6" else (lambda r: base(r[0]))
    return [b"".join(single_line((nm(a), a[1], a[2])) for a, _ in pe), b"".join(single_line((nm(b), b[1], b[2])) for _, b in pe)]


def flag_of(inp):
    return "--tab6" if inp == "pe6" else "--tab5"


def case_name(inp, lst, sam):
    return "%s_%s%s" % (inp, lst, "_sam" if sam else "")


def rows_by_read(tsv):
    """a recorded TSV (default columns) -> {readID: its rows}"""
    out = {}
    for ln in tsv.split(b"\n")[1:-1]:
        out.setdefault(ln.split(b"\t")[0], []).append(ln)
    return out


def mix_rows(header, se, pe, se_tsv, pe_tsv):
    """the TSV of the mixed file: every record's rows as the recorded unpaired / paired case has them, in file order"""
    s, p = rows_by_read(se_tsv), rows_by_read(pe_tsv)
    out = [header]
    for kind, k in mix_kinds(se, pe):
        out += s[se[k][0].split()[0]] if kind == "se" else p[base(pe[k][0][0]).split()[0]]
    return b"\n".join(out) + b"\n"
