"""The common cut of the two texts of a BGZF pair upload (text_cut_pair_body of centrifuge_amd/csrc/cf_inflate.hpp, launched as
k_text_cut_pair) on the CPU, through tests/emu/emu_matecut.cpp — as one thread and as the 64 threads of the launch — against the
rule stated here once more in plain Python; and the property the mates' way of the front end rests on: two files that go up
piece by piece, the tails handed on, come out record by record, pair by pair."""
import random

import pytest

from emu import emu_matecut as E

WAVES = [False, True]
BIG = 1 << 30


def markers(text, fastq):
    ch = 10 if fastq else 62
    return [i for i, c in enumerate(text) if c == ch]


def single(text, fastq, last, cap):
    """the cut of one text and the markers in front of it (text_cut_body's rule)"""
    pos = markers(text, fastq)
    if len(pos) > cap or last:
        return len(text), len(pos)
    if fastq:
        k = len(pos) // 4 * 4
        return (pos[k - 1] + 1 if k else 0), k
    starts = [p for p in pos if p == 0 or text[p - 1] == 10]
    if not starts or starts[-1] == 0:
        return 0, 0
    return starts[-1], sum(1 for p in pos if p < starts[-1])


def pair(t, fastq, last, cap=(BIG, BIG)):
    own = [single(t[i], fastq, last[i], cap[i]) for i in (0, 1)]
    k = [o[1] // 4 if fastq else o[1] for o in own]
    n = min(k)
    out, flags = [], 0
    for i in (0, 1):
        pos = markers(t[i], fastq)
        if len(pos) > cap[i] or k[i] == n:
            out.append(own[i])
        elif fastq:
            out.append((pos[4 * n - 1] + 1 if n else 0, 4 * n))
        else:
            p = pos[n]
            if p != 0 and t[i][p - 1] != 10:
                flags |= 1
            out.append((p, n))
    return out[0], out[1], flags


def fasta_records(n, rng, tag, odd_names=False):
    recs = []
    for i in range(n):
        name = b"r%d/%d" % (i, tag) + (b" a>b" if odd_names and rng.random() < 0.2 else b"")
        lines = [bytes(rng.choice(b"ACGTN") for _ in range(rng.choice([1, 7, 30, 60]))) for _ in range(rng.choice([1, 1, 2, 3]))]
        recs.append(b">" + name + b"\n" + b"\n".join(lines) + b"\n")
    return recs


def fastq_records(n, rng, tag):
    recs = []
    for i in range(n):
        L = rng.choice([1, 36, 100])
        # ('>' and '@' among the qualities, as real files have them)
        recs.append(b"@r%d/%d\n%s\n+\n%s\n" % (i, tag, bytes(rng.choice(b"ACGT") for _ in range(L)), bytes(rng.choice(b"#5>@I") for _ in range(L))))
    return recs


def check(t0, t1, fastq, last0, last1, wave64, cap=(BIG, BIG)):
    got = E.text_cut_pair(t0, t1, fastq, last0, last1, cap[0], cap[1], wave64=wave64)
    want = pair((t0, t1), fastq, (last0, last1), cap)
    assert got == want, (len(t0), len(t1), fastq, last0, last1, cap, got, want)
    for i, t in enumerate((t0, t1)):
        cut, k = got[i]
        assert cut <= len(t)                                  # (a marker beyond the kept ones reads as 2^32 - 1)
        if len(markers(t, fastq)) <= cap[i]:
            assert k == len(markers(t[:cut], fastq))
    return got


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("fastq", [0, 1])
def test_random_cuts(fastq, wave64):
    assert E.bad_start(wave64) == 1                           # kTxBadStart
    rng = random.Random(11 + fastq)
    make = fastq_records if fastq else (lambda n, r, tag: fasta_records(n, r, tag, odd_names=True))
    f0, f1 = b"".join(make(12, rng, 1)), b"".join(make(12, rng, 2))
    n_bad = 0
    for _ in range(150):
        e0, e1 = rng.choice([0, len(f0), rng.randrange(len(f0) + 1)]), rng.choice([0, len(f1), rng.randrange(len(f1) + 1)])
        for last0 in (0, 1):
            for last1 in (0, 1):
                n_bad += check(f0[:e0], f1[:e1], fastq, last0, last1, wave64)[2] != 0
    if not fastq:
        assert n_bad > 0                                      # (a '>' inside a name was marker n at least once)


@pytest.mark.parametrize("wave64", WAVES)
def test_edges(wave64):
    fa = b">a\nAC\n>b\nGG\n>c\nTT\n"
    fq = b"@a\nAC\n+\nII\n@b\nGG\n+\nII\n@c\nT"
    # n == 0: one side holds no whole record, nothing goes through and everything is tail
    assert check(fa, b">x\nAC", 0, 0, 0, wave64) == ((0, 0), (0, 0), 0)
    assert check(fq, b"@x\nAC\n+\nI", 1, 0, 0, wave64) == ((0, 0), (0, 0), 0)
    # one side empty, the other one last or not
    for last in (0, 1):
        assert check(fa, b"", 0, last, 0, wave64) == ((0, 0), (0, 0), 0)
        assert check(b"", fq, 1, 0, last, wave64) == ((0, 0), (0, 0), 0)
    assert check(b"", b"", 0, 1, 1, wave64) == ((0, 0), (0, 0), 0)
    # an empty text that is last holds 0 records: the other side waits, whatever it holds
    assert check(fa, b"", 0, 1, 1, wave64) == ((0, 0), (0, 0), 0)
    # the side with fewer records decides: one record of either goes through, the rest of the other is tail
    assert check(fa, b">x\nA\n>y\nC\n", 0, 0, 1, wave64) == ((12, 2), (10, 2), 0)
    assert check(fa, b">x\nA\n", 0, 0, 1, wave64) == ((6, 1), (5, 1), 0)
    assert check(fq, b"@x\nA\n+\nI\n", 1, 0, 1, wave64) == ((11, 4), (9, 4), 0)
    # both last, as many records: the single-file cuts (the texts' ends)
    assert check(fa, fa, 0, 1, 1, wave64) == ((len(fa), 3), (len(fa), 3), 0)
    # a FASTA marker n that does not start a line: the block is irregular, nothing is guessed
    odd = b">a x>y\nAC\n>b\nGG\n>c\nT\n"
    got = check(odd, b">x\nA\n>y\nC", 0, 0, 0, wave64)
    assert got[2] == E.bad_start(wave64) and got[1] == (5, 1)
    # ... and the same text where the odd marker lies behind the cut is fine
    assert check(b">a\nAC\n>b x>y\nGG\n>c\nT\n", b">x\nA\n>y\nC", 0, 0, 0, wave64) == ((6, 1), (5, 1), 0)


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("fastq", [0, 1])
def test_more_markers_than_are_kept(fastq, wave64):
    rng = random.Random(5)
    make = fastq_records if fastq else fasta_records
    f0, f1 = b"".join(make(9, rng, 1)), b"".join(make(6, rng, 2))
    m0, m1 = len(markers(f0, fastq)), len(markers(f1, fastq))
    for cap in [(m0 - 1, BIG), (BIG, m1 - 1), (3, 3), (0, BIG), (m0, m1), (m0 - 1, m1 - 1)]:
        for last0 in (0, 1):
            for last1 in (0, 1):
                got = check(f0, f1, fastq, last0, last1, wave64, cap)
                # the block with too many markers is not cut: the record pass sees the count and refuses it
                if m0 > cap[0]:
                    assert got[0] == (len(f0), m0)
                if m1 > cap[1]:
                    assert got[1] == (len(f1), m1)


def split_records(text, fastq):
    if fastq:
        lines = text.split(b"\n")
        assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
        return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]
    if not text:
        return []
    assert text[:1] == b">" and text[-1:] == b"\n"
    starts = [i for i in range(len(text)) if text[i] == 62 and (i == 0 or text[i - 1] == 10)]
    return [text[x:y] for x, y in zip(starts, starts[1:] + [len(text)])]


def pieces_of(text, rng):
    cuts = sorted(rng.randrange(len(text) + 1) for _ in range(rng.randrange(0, 7)))
    return [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]


@pytest.mark.parametrize("wave64", WAVES)
@pytest.mark.parametrize("fastq", [0, 1])
def test_induction_over_pieces(fastq, wave64):
    rng = random.Random(77 + fastq)
    make = fastq_records if fastq else fasta_records
    for trial in range(40):
        n0 = rng.randrange(0, 14)
        n1 = n0 if trial % 2 == 0 else rng.randrange(0, 14)
        r0, r1 = make(n0, rng, 1), make(n1, rng, 2)
        p = [pieces_of(b"".join(r0), rng), pieces_of(b"".join(r1), rng)]
        head, out = [b"", b""], [[], []]
        for call in range(max(len(p[0]), len(p[1]))):
            text = [head[i] + (p[i][call] if call < len(p[i]) else b"") for i in (0, 1)]
            last = [call + 1 >= len(p[i]) for i in (0, 1)]
            c0, c1, flags = check(text[0], text[1], fastq, last[0], last[1], wave64)
            assert flags == 0
            for i, (cut, k) in enumerate((c0, c1)):
                recs = split_records(text[i][:cut], fastq)
                assert len(recs) == (k // 4 if fastq else k)
                out[i] += recs
                head[i] = text[i][cut:]
            assert len(out[0]) == len(out[1])                 # q with q, call by call
        n = min(n0, n1)
        assert out[0] == r0[:n] and out[1] == r1[:n]          # in order, none lost or doubled
        assert head[0] == b"".join(r0[n:]) and head[1] == b"".join(r1[n:])
        assert (head == [b"", b""]) == (n0 == n1)
