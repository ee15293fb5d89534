"""The device record pass over tabbed blocks (cf_textio.hpp: text_count / mark / record_body's tabbed branch, text_pack_body) on
the CPU — as plain loops and as wavefronts of 64 lanes (tests/emu/emu_texttab.*) — against the HOST parser (`centrifuge-class
--dump-reads --tab5 / --tab6`, parseTabChunk): lengths, seeds, readIDs, packed words and N masks of every read of a plain block,
and the exact refusal bit of every block that is not plain.  Needs no GPU; fails before the change (no such format, no such option)."""
import os
import random
import subprocess
import tempfile

import pytest

import common
from emu import emu_texttab as E

CLI = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-class")
BAD_START, EMPTY_NAME, CR, BAD_BASE, EMPTY_SEQ, QUAL_LEN, BAD_QUAL, LINE_COUNT, FIELD_COUNT = 1, 4, 8, 16, 32, 128, 256, 512, 8192


def host(text, fmt, t5=0, t3=0, seed=0):
    """the host parser: (readID, bases, qualities, seed) per read"""
    with tempfile.NamedTemporaryFile(suffix=".tab") as f:
        f.write(text); f.flush()
        r = subprocess.run([CLI, "--dump-reads", "--tab5" if fmt == E.TAB5 else "--tab6", f.name, "--seed", str(seed), "-5", str(t5), "-3", str(t3)], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = []
    for ln in r.stdout.split(b"\n")[:-1]:
        n, s, q, sd = ln.split(b"\t")
        if n[-2:] in (b"/1", b"/2", b"/3"):
            n = n[:-2]
        out.append((n.split()[0] if n.split() else b"", s, q, int(sd)))
    return out


def device(text, fmt, wave64, **kw):
    fl, o = E.upload(text, fmt, wave64=wave64, **kw)
    if fl:
        return fl, None, None
    reads = []
    for r in range(o["n_reads"]):
        L = int(o["rlen"][r])
        seq = bytes(b"N"[0] if (o["nmask"][r][i >> 5] >> (i & 31)) & 1 else b"ACGT"[(o["bases"][r][i >> 5] >> (2 * (i & 31))) & 3] for i in range(L))
        assert o["buf"][o["seqOff"][r]:o["seqOff"][r] + L].upper() == seq
        reads.append((o["buf"][o["idOff"][r]:o["idOff"][r] + o["idLen"][r]], seq, o["buf"][o["qualOff"][r]:o["qualOff"][r] + L], int(o["seeds"][r])))
    total, longest = sum(len(r[1]) for r in reads), max([len(r[1]) for r in reads] or [0])
    if kw.get("max_reads"):                                           # (the sums cover the reads max_reads cuts off as well: upper bounds)
        assert o["n_bases"] >= total and o["max_len"] >= longest
    else:
        assert o["n_bases"] == total and o["max_len"] == longest
    return 0, o["paired"], reads


def rnd_seq(rng, n, odd=False):
    return bytes(rng.choice(b"ACGTacgtNn" if odd else b"ACGT") for _ in range(n))


def rnd_qual(rng, n):
    return bytes(rng.randrange(33, 127) for _ in range(n))


def line(rng, fmt, pair, len1, len2=0, name_len=3, odd=False):
    nm = bytes(rng.choice(b"abcxyz_019") for _ in range(name_len))
    f = [nm, rnd_seq(rng, len1, odd), rnd_qual(rng, len1)]
    if pair:
        f += ([nm[:-1] + b"Z"] if fmt == E.TAB6 else []) + [rnd_seq(rng, len2, odd), rnd_qual(rng, len2)]
    return b"\t".join(f) + b"\n"


@pytest.mark.parametrize("wave64", [False, True], ids=["loop", "wave64"])
@pytest.mark.parametrize("fmt,pair", [(E.TAB5, False), (E.TAB5, True), (E.TAB6, True)], ids=["single", "tab5", "tab6"])
def test_every_field_start_meets_every_place_of_an_8_byte_word(fmt, pair, wave64):
    """read lengths 1..33 x name lengths 1..9 (mates of unequal length, lower case and N in either), in one block of many 64-byte pieces"""
    rng = random.Random(7)
    text = b"".join(line(rng, fmt, pair, L, 34 - L, n, odd=True) for L in range(1, 34) for n in range(1, 10))
    fl, paired, got = device(text, fmt, wave64, seed=5)
    assert fl == 0 and paired == pair
    assert got == host(text, fmt, seed=5)


@pytest.mark.parametrize("wave64", [False, True], ids=["loop", "wave64"])
def test_small_shapes_trim_skip_and_max_reads(wave64):
    rng = random.Random(11)
    one = line(rng, E.TAB6, True, 40, 37, 5)
    fl, paired, got = device(one, E.TAB6, wave64)                     # a block of one record
    assert fl == 0 and paired and got == host(one, E.TAB6)
    long = b"".join(line(rng, E.TAB5, True, 70 + i, 90 - i, 4, odd=True) for i in range(9))     # every line straddles 64-byte pieces
    for t5, t3 in ((0, 0), (7, 11), (3, 0), (0, 5)):
        want = host(long, E.TAB5, t5, t3)
        fl, paired, got = device(long, E.TAB5, wave64, trim5=t5, trim3=t3)
        assert fl == 0 and paired and got == want
        fl, paired, got = device(long, E.TAB5, wave64, trim5=t5, trim3=t3, skip=2, max_reads=3)   # records: a pair is one
        assert fl == 0 and got == want[4:10]
    fl, paired, got = device(long, E.TAB5, wave64, skip=50)           # a skip beyond the block
    assert fl == 0 and got == []
    # a trim that empties only mate 2
    text = b"a\t" + b"ACGT" * 10 + b"\t" + b"I" * 40 + b"\t" + b"ACGT" * 3 + b"\t" + b"I" * 12 + b"\n"
    assert device(text, E.TAB5, wave64, trim5=7, trim3=11)[0] == EMPTY_SEQ
    assert device(text, E.TAB5, wave64, trim5=7, trim3=4)[0] == 0


@pytest.mark.parametrize("wave64", [False, True], ids=["loop", "wave64"])
def test_each_block_outside_the_plain_form_is_refused_with_its_bit(wave64):
    ok5 = b"n\tACGT\tIIII\tGGCC\tJJJJ\n"
    ok3 = b"m\tACGT\tIIII\n"
    assert device(ok5 + ok5, E.TAB5, wave64)[0] == 0 and device(ok3 * 3, E.TAB5, wave64)[0] == 0
    cases = [
        (ok5 + ok5[:-1], LINE_COUNT),                                        # the last line lacks its '\n'
        (ok5 + b"n\tACGT\tIIII\tGGCC\tJJJJ\r\n", CR | QUAL_LEN),            # ('\r' is no line end here: it also makes the last field one long)
        (ok5 + b"n\r\tACGT\tIIII\tGGCC\tJJJJ\n", CR),
        (ok5 + b"n\tACGT\tIIII\tGGCC\n", LINE_COUNT),                       # 4 fields
        (ok5 + b"n\tACGT\tIIII\tn2\tGGCC\tJJJJ\tX\n", LINE_COUNT),           # 7
        (ok5 + b"\n" + ok5, LINE_COUNT),                                     # an empty line
        (ok5 + b"n\tACGT\tIII\tGGCC\tJJJJ\n", QUAL_LEN),                     # one short
        (ok5 + b"n\tACGT\tIIII\tGGCC\tJJJJJ\n", QUAL_LEN),                   # one long
        (ok5 + b"n\tACGT\tII I\tGGCC\tJJJJ\n", BAD_QUAL),                    # a space (32)
        (ok5 + b"n\tACGT\tIIII\tGGCC\tJJ\x1fJ\n", BAD_QUAL),
        (ok5 + b"n\tACRT\tIIII\tGGCC\tJJJJ\n", BAD_BASE),
        (ok5 + b"n\tAC.T\tIIII\tGGCC\tJJJJ\n", BAD_BASE),
        (ok5 + b"\tACGT\tIIII\tGGCC\tJJJJ\n", EMPTY_NAME),
        (ok5 + b"n\t\t\tGGCC\tJJJJ\n", EMPTY_SEQ),
        (ok5 + ok3, FIELD_COUNT),                                            # a mixed block
        (ok3 + ok5 * 70, FIELD_COUNT),                                       # ... over more than one wavefront
    ]
    for text, bit in cases:
        assert device(text, E.TAB5, wave64)[0] == bit, (text[-40:], bit)
    ok6 = b"n/1\tACGT\tIIII\tn/2\tGGCC\tJJJJ\n"
    assert device(ok6, E.TAB6, wave64)[0] == 0
    assert device(ok6 + b"n\tACGT\tIIII\t\tGGCC\tJJJJ\n", E.TAB6, wave64)[0] == EMPTY_NAME     # the second name empty
    assert device(ok6 + ok5, E.TAB6, wave64)[0] == LINE_COUNT                                    # 5 fields under tab6
    assert device(b"", E.TAB5, wave64)[0] == 0


def test_synth_small_inputs_are_plain_and_equal_the_host_parser():
    import tabcases as T
    d, _ = common.golden("synth_small")
    se, pe = T.records(d)
    for inp, fmt in (("se", E.TAB5), ("pe5", E.TAB5), ("pe6", E.TAB6)):
        text = T.text_of(inp, se, pe)[:30000]
        text = text[:text.rindex(b"\n") + 1]
        fl, paired, got = device(text, fmt, True)
        assert fl == 0 and paired == (inp != "se") and got == host(text, fmt)
    assert device(T.text_of("mix", se, pe), E.TAB5, False)[0] == FIELD_COUNT
