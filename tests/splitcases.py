"""What --un / --al / --un-conc / --al-conc write, stated on the output's rows (the reference's wrapper script `centrifuge` does the
same from the readSeq / readQual columns it has centrifuge-class print) — shared by the tests of the read splitter."""
import zlib

KEYS = ("un", "al", "un1", "un2", "al1", "al2")
# the sinks of cf_batch_wait_text_split, by what the contract calls them: an unpaired batch feeds 0 and 2, mates all four
SINKS_UNPAIRED = {"un": 0, "al": 2}
SINKS_PAIRED = {"un1": 0, "un2": 1, "al1": 2, "al2": 3}


def contract(rows):
    """rows: (readID, readSeq, readQual, classified) per PRINTED row -> the six files' bytes"""
    out = {k: b"" for k in KEYS}
    for rid, seq, qual, classified in rows:
        k = "al" if classified else "un"
        if b"_" in seq:                                      # a pair: seq1_seq2, the qualities cut at len(seq1)
            s1, s2 = seq.split(b"_")
            out[k + "1"] += b"@%s\n%s\n+\n%s\n" % (rid, s1, qual[:len(s1)])
            out[k + "2"] += b"@%s\n%s\n+\n%s\n" % (rid, s2, qual[len(s1) + 1:])
        else:
            out[k] += b"@%s\n%s\n+\n%s\n" % (rid, seq, qual)
    return out


def rows_of_tsv(tsv, cols):
    """the rows of a run printed with --tab-fmt-cols <cols> (readID, seqID, readSeq, readQual among them), header line included"""
    lines = tsv.split(b"\n")
    assert lines[0].split(b"\t") == [c.encode() for c in cols]
    i_id, i_seqid, i_seq, i_qual = (cols.index(c) for c in ("readID", "seqID", "readSeq", "readQual"))
    out = []
    for ln in lines[1:]:
        if ln:
            f = ln.split(b"\t")
            out.append((f[i_id], f[i_seq], f[i_qual], f[i_seqid] != b"unclassified"))
    return out


def conc_names(path):
    """the two files of --un-conc / --al-conc <path> (centrifuge:725-769; not a directory)"""
    d, _, base = path.rpartition("/")
    d = d + "/" if _ else ""
    if "%" in base:
        return d + base.replace("%", "1"), d + base.replace("%", "2")
    if "." in base:
        stem, _, ext = base.rpartition(".")
        return d + stem + ".1." + ext, d + stem + ".2." + ext
    return path + ".1", path + ".2"


def inflate_bgzf(data):
    """the text of a BGZF file (every member inflated; the last one must be the empty member)"""
    out, at, last = b"", 0, None
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", "not a BGZF member at byte %d" % at
        bsize = int.from_bytes(data[at + 16:at + 18], "little") + 1
        last = zlib.decompress(data[at:at + bsize], 31)
        out += last
        at += bsize
    assert last == b"", "no empty member at the end"
    return out
