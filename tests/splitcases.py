"""What --un / --al / --un-conc / --al-conc write, stated on the output's rows (the reference's wrapper script `centrifuge` does the
same from the readSeq / readQual columns it has centrifuge-class print) — shared by the tests of the read splitter."""
import functools
import zlib

import numpy as np

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


# ---- the splitter's table: synthetic batches for split_size_body / split_write_body, read by the CPU harness (tests/test_split_emu.py)
# and by the device (tests/test_gpu_splitcases.py, through the tap cf_debug_split).  A runner is a callable (batch, sinks, cap) ->
# per sink (the first min(bytes sized, room) bytes of its room with UNWRITTEN where nothing was written, the bytes sized, the
# records, sized): emu_split.split and capi.debug_split.
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 250]
UN, AL = 1, 2
UNWRITTEN = 0x5A
COUNTS = [1, 63, 64, 65, 130, 255, 256, 257, 256 + 65]       # a wavefront's tail; a block of four wavefronts and its tail
TRIMS = [(7, 11), (1, 0), (0, 3)]


def read_id(name):
    """aln_sink.h:2203-2217: a trailing /1 /2 /3 goes, then the name up to the first white space"""
    if len(name) >= 2 and name[-2:-1] == b"/" and name[-1:] in (b"1", b"2", b"3"):
        name = name[:-2]
    return name.split()[0] if name.split() else b""


def pack(seqs):
    """2-bit words and N masks, ceil(len / 32) per read (an N: code 0, its mask bit set)"""
    words, masks = [], []
    for s in seqs:
        for k in range(0, len(s), 32):
            w = m = 0
            for j, ch in enumerate(s[k:k + 32]):
                if ch == ord("N"):
                    m |= 1 << j
                else:
                    w |= b"ACGT".index(bytes([ch])) << (2 * j)
            words.append(w); masks.append(m)
    return np.array(words, dtype=np.uint64), np.array(masks, dtype=np.uint32)


def make_batch(nq, pattern, paired, fastq, seed, trim5=0, trim3=0, length_of=None):
    """pattern(q) -> rows of query q.  The block's text, what the record pass leaves of it under -5 / -3 (the window's length, its
    packed bases, the place of its first quality), and the rows the run prints: (readID, readSeq, readQual, classified).
    length_of(r): the length of read r, in place of the turn through LENGTHS"""
    rng = np.random.default_rng(seed)
    per = 2 if paired else 1
    text, id_off, id_len, qual_off, rlen, kept, kq = b"", [], [], [], [], [], []
    for r in range(nq * per):
        n = (length_of(r) if length_of else LENGTHS[(r * (3 if paired else 1) + seed) % len(LENGTHS)]) + trim5 + trim3      # (mates: unequal lengths)
        s = bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)))
        for p in ((0,), (31, 32), (n - 1,), (), ())[r % 5]:
            if p < n:
                s[p] = ord("N")
        s = bytes(s)
        q = bytes(rng.integers(33, 127, n, dtype=np.uint8))
        nm = b"r%d.%s" % (r, b"x" * (r % 7)) + (b" some comment" if r % 3 == 0 else b"") + (b"/1" if r % 4 == 1 else b"")
        text += b"@" if fastq else b">"
        id_off.append(len(text)); id_len.append(len(read_id(nm)))
        text += nm + b"\n"
        if fastq:
            text += s + b"\n+\n"
            qual_off.append(len(text) + trim5)
            text += q + b"\n"
        else:
            t = s.lower() if r % 2 else s
            text += b"\n".join(t[k:k + 60] for k in range(0, len(t), 60)) + b"\n"
        w = s[trim5:n - trim3]
        kept.append(w); kq.append(q[trim5:n - trim3] if fastq else b"I" * len(w)); rlen.append(len(w))
    bases, nmask = pack(kept)
    qinfo = np.array([pattern(q) for q in range(nq)], dtype=np.uint8)
    rows = []
    for q in range(nq):
        ra = q * per
        rid = text[id_off[ra]:id_off[ra] + id_len[ra]]
        seq, qual = (kept[ra] + b"_" + kept[ra + 1], kq[ra] + b"_" + kq[ra + 1]) if paired else (kept[ra], kq[ra])
        rows += [(rid, seq, qual, qinfo[q] > 0)] * max(1, int(qinfo[q]))
    b = dict(text=text, idOff=id_off, idLen=id_len, rlen=rlen, qualOff=qual_off if fastq else None, bases=bases, nmask=nmask,
             qinfo=qinfo | 0x40, paired=paired)          # (the bits above the row count are the mates' "took part" bits: not the splitter's)
    return b, rows


PATTERNS = {"classified": lambda q: 1 + (q % 3 == 0), "unclassified": lambda q: 0, "alternating": lambda q: q & 1,
            "rows0125": lambda q: (0, 1, 2, 5)[q % 4]}
# only the last query of 257 is classified (a block's tail of one thread), only the first
LONE = {"last-of-257": lambda q: int(q == 256), "first-of-257": lambda q: int(q == 0)}


def sink_keys(paired):
    names = SINKS_PAIRED if paired else SINKS_UNPAIRED
    return {v: k for k, v in names.items()}


def check(run, batch, rows, sinks, cap=None):
    """one batch through one runner against the contract.  cap: the room of every sink or four of them (None: plenty); the records
    that lie wholly inside a sink's room are there, every other byte of it is UNWRITTEN"""
    want = contract(rows)
    got = run(batch, sinks, cap) if cap is not None else run(batch, sinks, 1 << 22)
    caps = [1 << 22] * 4 if cap is None else [cap] * 4 if np.isscalar(cap) else list(cap)
    keys = sink_keys(batch["paired"])
    for s in range(4):
        key = keys.get(s)
        on = key is not None and bool(sinks & (UN if key.startswith("un") else AL))
        text, n_bytes, n_rec, sized = got[s]
        assert sized == on, "sink %d: sized %r, asked for %r" % (s, sized, on)
        if not on:
            assert n_bytes == 0 and n_rec == 0 and text == b""
            continue
        assert n_bytes == len(want[key]), "sink %d (%s): %d bytes sized, %d expected" % (s, key, n_bytes, len(want[key]))
        assert n_rec == want[key].count(b"\n") // 4
        room = min(caps[s], len(want[key]))
        assert len(text) == room
        # a query's records fit or are left out together: the write pass asks whether all of them lie inside the room
        img, at = bytearray([UNWRITTEN]) * room, 0
        for recs in sink_records(rows, key):
            if at + len(recs) <= room:
                img[at:at + len(recs)] = recs
            at += len(recs)
        assert at == len(want[key])
        assert text == bytes(img), "sink %d (%s) differs" % (s, key)


def sink_records(rows, key):
    """per query (a run of equal rows: one record per printed row) its bytes in the sink"""
    out, i = [], 0
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j] is rows[i]:
            j += 1
        out.append(contract(rows[i:j])[key])
        i = j
    return out


@functools.lru_cache(maxsize=None)
def room_cases():
    """(id, batch, rows, sinks, caps): every sink's room all of its text, a byte less, cut inside a query's records, on a boundary
    between two queries, inside the last wavefront's stretch, none"""
    from fmtcases import room_points
    out = []
    for pattern in ("unclassified", "classified"):
        for paired in (False, True):
            batch, rows = make_batch(130, PATTERNS[pattern], paired, True, seed=31 + paired)
            keys = sink_keys(paired)
            points = {s: dict(room_points([len(r) for r in sink_records(rows, k)])) for s, k in keys.items() if k.startswith(pattern[:2] if pattern == "unclassified" else "al")}
            for what in ("all", "less1", "in-row", "row-boundary", "last-wave", "none"):
                out.append(("%s-%s-%s" % (pattern, "mates" if paired else "unpaired", what), batch, rows, UN | AL, [points[s][what] if s in points else 0 for s in range(4)]))
    return out


def mate_extremes():
    """mates where one is one base long and the other 250, in both orders"""
    return make_batch(67, PATTERNS["rows0125"], True, True, seed=8, length_of=lambda r: (1, 250, 250, 1)[r % 4])
