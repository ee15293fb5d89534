"""The read splitter of the device text path (split_size_body / split_write_body, centrifuge_amd/csrc/cf_textio.hpp) in the CPU harness
of tests/emu/emu_split.cpp — the one-lane build and wavefronts of 64 lanes — against the contract's Python statement
(tests/splitcases.py), byte for byte: synthetic FASTA (wrapped, lower case) and FASTQ blocks, unpaired reads and mates of unequal
lengths, the lengths at which the wave-wide copies change their way (dword phases, the 16-base and 32-base steps of the 2-bit
expansion), query counts around a wavefront, 0 .. 5 rows per query, every subset of the sinks, and -5 / -3 windows."""
import numpy as np
import pytest

import splitcases
from emu import emu_split

LENGTHS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 250]
UN, AL = 1, 2


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


def make_batch(nq, pattern, paired, fastq, seed, trim5=0, trim3=0):
    """pattern(q) -> rows of query q.  The block's text, what the record pass leaves of it under -5 / -3 (the window's length, its
    packed bases, the place of its first quality), and the rows the run prints: (readID, readSeq, readQual, classified)"""
    rng = np.random.default_rng(seed)
    per = 2 if paired else 1
    text, id_off, id_len, qual_off, rlen, kept, kq = b"", [], [], [], [], [], []
    for r in range(nq * per):
        n = LENGTHS[(r * (3 if paired else 1) + seed) % len(LENGTHS)] + trim5 + trim3      # (mates: unequal lengths)
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


def check(batch, rows, sinks, wave64):
    want = splitcases.contract(rows)
    got = emu_split.split(batch, sinks, wave64)
    names = splitcases.SINKS_PAIRED if batch["paired"] else splitcases.SINKS_UNPAIRED
    for s in range(4):
        key = [k for k, v in names.items() if v == s]
        on = bool(key) and bool(sinks & (UN if key[0].startswith("un") else AL))
        text, n_bytes, n_rec, sized = got[s]
        assert sized == on, "sink %d: sized %r, asked for %r" % (s, sized, on)
        if not on:
            assert n_bytes == 0 and n_rec == 0 and text == b""
            continue
        assert n_bytes == len(want[key[0]]), "sink %d (%s): %d bytes sized, %d expected" % (s, key[0], n_bytes, len(want[key[0]]))
        assert text == want[key[0]], "sink %d (%s) differs" % (s, key[0])
        assert n_rec == want[key[0]].count(b"\n") // 4


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_split_matches_contract(wave64, paired, fastq, pattern):
    for nq in (1, 63, 64, 65, 130):
        batch, rows = make_batch(nq, PATTERNS[pattern], paired, fastq, seed=nq)
        check(batch, rows, UN | AL, wave64)
    if pattern == "unclassified":       # an empty sink is 0 bytes
        got = emu_split.split(batch, UN | AL, wave64)
        assert got[2][:3] == (b"", 0, 0) and got[0][1] > 0


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "mates"])
@pytest.mark.parametrize("sinks", [0, UN, AL, UN | AL])
def test_split_sink_subsets(wave64, paired, sinks):
    batch, rows = make_batch(70, PATTERNS["rows0125"], paired, True, seed=3)
    check(batch, rows, sinks, wave64)


@pytest.mark.parametrize("wave64", [False, True], ids=["lane1", "wave64"])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("trim", [(7, 11), (1, 0), (0, 3)])
def test_split_trim_windows(wave64, fastq, trim):
    for paired in (False, True):
        batch, rows = make_batch(67, PATTERNS["rows0125"], paired, fastq, seed=5, trim5=trim[0], trim3=trim[1])
        check(batch, rows, UN | AL, wave64)


def test_split_room_too_small_leaves_the_rest_alone():
    """records that do not fit the room they were promised are left out, nothing is written outside it"""
    batch, rows = make_batch(65, PATTERNS["alternating"], False, True, seed=2)
    for wave64 in (False, True):
        got = emu_split.split(batch, UN | AL, wave64, cap=1000)
        want = splitcases.contract(rows)
        for s, k in ((0, "un"), (2, "al")):
            text, n_bytes = got[s][0], got[s][1]
            assert n_bytes == len(want[k]) and len(text) == 1000
            whole = 0                                   # the records that lie wholly inside the room are there
            for row in rows:
                rec = splitcases.contract([row])[k]
                if whole + len(rec) > 1000:
                    break
                whole += len(rec)
            assert text[:whole] == want[k][:whole]
