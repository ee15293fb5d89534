"""-5 / -3 / -s on the device text path in the CPU harness (tests/emu/emu_texttrim.cpp): the record pass of
centrifuge_amd/csrc/cf_textio.hpp with DTextRec's trim5 / trim3 / skip set, and the pack pass behind it — in the one-lane build and
as wavefronts of 64 lanes — against

* an independent Python statement of what the parsers leave of a plain record (parseFastaChunk / parseFastqChunk, cf_ingest.cpp,
  after pat.cpp: the bases behind the first trim5 and in front of the last trim3, the same stretch of the qualities) with the seed
  from cf_gen_rand_seed through the C ABI (no device needed): per kept read its length, seed, packed words, N mask and the bytes
  its readID and quality places point at;
* the HOST parser itself (`centrifuge-class --dump-reads -5 .. -3 ..`) under random damage: a block is either refused or gives
  the very reads the host parser gives with the same trims;
* the untouched entry of tests/emu/emu.cpp for no trim and no skip: bit for bit what it was."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common
from centrifuge_amd import capi
from emu import emu, emu_texttrim

CLI = os.path.join(common.ROOT, "centrifuge_amd", "bin", "centrifuge-class")
FASTA, FASTQ = 0, 1
EMPTY_SEQ = 32                                                   # kTxEmptySeq
TRIMS = [(0, 0), (1, 0), (0, 1), (5, 0), (0, 7), (13, 9), (31, 33), (64, 0)]
# read lengths on both sides of the 8-byte fast path (of the record pass and of the pack pass) and of the 32-base words
LENGTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 63, 64, 65, 66, 71, 72, 73, 95, 96, 97, 100, 127, 128, 129, 150, 199, 200]
N_REC = 131                                                      # two wavefronts and a bit
VARIANTS = [(FASTQ, 0), (FASTA, 0), (FASTA, 7), (FASTA, 60)]


@pytest.fixture(params=[False, True], ids=["lane1", "wave64"])
def wave64(request):
    return request.param


def read_id(name):
    """aln_sink.h:2203-2217"""
    if len(name) >= 2 and name[-2:] in (b"/1", b"/2", b"/3"):
        name = name[:-2]
    for i, c in enumerate(name):
        if c in b" \t\n\v\f\r":
            return name[:i]
    return name


def make_records(rng, n, min_len, lengths=LENGTHS):
    """n records (name, bases, qualities) of every length of `lengths` above min_len at least once: mixed case, Ns, names of all styles"""
    pool = [x for x in lengths if x > min_len] or [min_len + 1]
    recs = []
    for i in range(n):
        ln = pool[i] if i < len(pool) else int(rng.choice(pool))
        alphabet = "ACGTN" if rng.random() < 0.4 else "ACGT"
        seq = "".join(rng.choice(list(alphabet), ln))
        if rng.random() < 0.3:
            seq = seq.lower()
        elif rng.random() < 0.3:
            seq = "".join(c.lower() if rng.random() < 0.5 else c for c in seq)
        name = ("r%d" % i).encode()
        style = int(rng.integers(0, 6))
        name += [b"", b" some comment/here", b"/1", b"\tx/2", b"/3", bytes([200, 255]) + b"x"][style]
        qual = bytes(int(q) for q in rng.integers(33, 127, ln))
        recs.append((name, seq, qual))
    order = rng.permutation(n)
    return [recs[i] for i in order]


def as_text(recs, fmt, wrap=0):
    out = []
    for name, seq, qual in recs:
        if fmt == FASTA:
            body = seq if not wrap else "\n".join(seq[k:k + wrap] for k in range(0, len(seq), wrap))
            out.append(b">" + name + b"\n" + body.encode() + b"\n")
        else:
            out.append(b"@" + name + b"\n" + seq.encode() + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def expected(recs, fmt, trim5, trim3, seed):
    """per record what the parsers make of it: (readID, window's bases in upper case, its qualities or None, seed, packed words, N masks)"""
    L = capi.lib()
    out = []
    for name, seq, qual in recs:
        a = min(trim5, len(seq))
        ln = max(0, max(0, len(seq) - trim5) - trim3)
        win = seq[a:a + ln].upper()
        q = qual[a:a + ln] if fmt == FASTQ else None
        codes = np.array(["ACGTN".index(c) for c in win], dtype=np.uint8)
        qa = np.frombuffer(q, dtype=np.uint8) if q else None
        sd = L.cf_gen_rand_seed(codes.ctypes.data if ln else None, qa.ctypes.data if qa is not None else None, ln, name, len(name), seed)
        words, masks = [0] * ((ln + 31) // 32), [0] * ((ln + 31) // 32)
        for i, c in enumerate(codes):
            if c == 4:
                masks[i // 32] |= 1 << (i % 32)
            else:
                words[i // 32] |= int(c) << (2 * (i % 32))
        out.append((read_id(name), win, q, int(sd), words, masks))
    return out


def check_reads(got, want, fmt):
    """the batch `got` (emu_texttrim.upload) holds the reads `want`, in that order"""
    assert got["n_reads"] == len(want)
    buf = got["buf"]
    for r, (rid, win, q, sd, words, masks) in enumerate(want):
        assert int(got["rlen"][r]) == len(win), r
        assert int(got["seeds"][r]) == sd, r
        assert got["bases"][r] == words and got["nmask"][r] == masks, r
        assert buf[int(got["idOff"][r]):int(got["idOff"][r]) + int(got["idLen"][r])] == rid, r
        if fmt == FASTQ:
            assert buf[int(got["qualOff"][r]):int(got["qualOff"][r]) + len(win)] == q, r
        # seqOff is the byte of the first kept base (in mid-line as it may be)
        if win:
            assert chr(buf[int(got["seqOff"][r])]).upper() == win[0], r


def skips(n):
    return [0, 1, 63, 64, 65, n - 1, n, n + 5]


@pytest.mark.parametrize("fmt,wrap", VARIANTS, ids=["fastq", "fasta", "fasta-wrap7", "fasta-wrap60"])
@pytest.mark.parametrize("trim", TRIMS, ids=["%d-%d" % t for t in TRIMS])
def test_windows_and_skips_of_plain_blocks(wave64, fmt, wrap, trim):
    t5, t3 = trim
    rng = np.random.default_rng(1000 * fmt + 10 * wrap + t5 + 3 * t3)
    recs = make_records(rng, N_REC, t5 + t3)
    text = as_text(recs, fmt, wrap)
    seed = 12345 if t5 & 1 else 0
    want = expected(recs, fmt, t5, t3, seed)
    assert all(w[1] for w in want)
    for skip in skips(N_REC):
        for max_reads in (0, 40):
            flags, got = emu_texttrim.upload([text], fmt, t5, t3, skip, max_reads, seed, wave64)
            assert flags == 0, (skip, max_reads, flags)
            kept = want[skip:]
            check_reads(got, kept[:max_reads] if max_reads else kept, fmt)
            # the block's sums speak of the kept records' windows (with max_reads: of a few reads too many, as ever)
            n_words, n_bases, max_len = sum(len(w[4]) for w in kept), sum(len(w[1]) for w in kept), max([len(w[1]) for w in kept] + [0])
            assert (got["n_words"], got["n_bases"], got["max_len"]) == (n_words, n_bases, max_len), (skip, max_reads)


@pytest.mark.parametrize("fmt,wrap", [(FASTQ, 0), (FASTA, 9)], ids=["fastq", "fasta-wrap9"])
def test_both_mates_with_stride_two(wave64, fmt, wrap):
    rng = np.random.default_rng(77 + fmt)
    for t5, t3 in [(0, 0), (5, 0), (13, 9), (31, 33)]:
        r1, r2 = make_records(rng, 97, t5 + t3), make_records(rng, 97, t5 + t3)
        t1, t2 = as_text(r1, fmt, wrap), as_text(r2, fmt, 0)
        w1, w2 = expected(r1, fmt, t5, t3, 7), expected(r2, fmt, t5, t3, 7)
        for skip in (0, 1, 64, 96, 97, 102):
            for max_reads in (0, 20):
                flags, got = emu_texttrim.upload([t1, t2], fmt, t5, t3, skip, max_reads, 7, wave64)
                assert flags == 0
                pairs = list(zip(w1, w2))[skip:]
                if max_reads:
                    pairs = pairs[:max_reads]
                check_reads(got, [m for p in pairs for m in p], fmt)


@pytest.mark.parametrize("fmt,wrap", VARIANTS, ids=["fastq", "fasta", "fasta-wrap7", "fasta-wrap60"])
def test_an_empty_window_refuses_the_block(wave64, fmt, wrap):
    """empty reads are the host parser's: a record of which the trims leave nothing — wherever it is, skipped or not — flags the block"""
    rng = np.random.default_rng(5 + fmt + wrap)
    for t5, t3, short in [(10, 5, 12), (10, 5, 15), (0, 7, 7), (5, 0, 3), (64, 0, 64), (31, 33, 40)]:
        for where in (0, 70, 130):
            recs = make_records(rng, 130, t5 + t3)
            name, seq, qual = recs[0]
            recs.insert(where, (b"short", seq[:1] * short, qual[:1] * short))
            for skip in (0, where + 1):
                flags, got = emu_texttrim.upload([as_text(recs, fmt, wrap)], fmt, t5, t3, skip, 0, 0, wave64)
                assert flags & EMPTY_SEQ and got is None, (t5, t3, short, where, skip)
        # ... and one base left is a read
        recs = make_records(rng, 70, t5 + t3)
        recs.insert(3, (b"one", "g" * (t5 + t3 + 1), b"5" * (t5 + t3 + 1)))
        flags, got = emu_texttrim.upload([as_text(recs, fmt, wrap)], fmt, t5, t3, 0, 0, 0, wave64)
        assert flags == 0 and int(got["rlen"][3]) == 1
        check_reads(got, expected(recs, fmt, t5, t3, 0), fmt)


@pytest.mark.parametrize("fmt,wrap", VARIANTS, ids=["fastq", "fasta", "fasta-wrap7", "fasta-wrap60"])
def test_the_checks_cover_the_trimmed_parts(wave64, fmt, wrap):
    """a character outside the plain form refuses the block even where the trims would drop it"""
    rng = np.random.default_rng(9)
    recs = make_records(rng, 70, 40, lengths=[100])
    for at, bad_bit in ((2, 16), (97, 16)):
        name, seq, qual = recs[5]
        damaged = list(recs)
        damaged[5] = (name, seq[:at] + "R" + seq[at + 1:], qual)
        assert emu_texttrim.upload([as_text(damaged, fmt, wrap)], fmt, 10, 10, 0, 0, 0, wave64)[0] & bad_bit
        assert emu_texttrim.upload([as_text(damaged, fmt, wrap)], fmt, 10, 10, 20, 0, 0, wave64)[0] & bad_bit      # (skipped records are checked)
        if fmt == FASTQ:
            damaged[5] = (name, seq, qual[:at] + b" " + qual[at + 1:])
            assert emu_texttrim.upload([as_text(damaged, fmt)], fmt, 10, 10, 0, 0, 0, wave64)[0] & 256
            damaged[5] = (name, seq, qual + b"I")
            assert emu_texttrim.upload([as_text(damaged, fmt)], fmt, 10, 10, 0, 0, 0, wave64)[0] & 128


def host_parse(text, fmt, t5, t3, seed=0):
    """the host parser through --dump-reads: None when it refuses the input, else (readID, bases, qualities, seed) per read"""
    with tempfile.NamedTemporaryFile(suffix=".fa" if fmt == FASTA else ".fq") as f:
        f.write(text)
        f.flush()
        r = subprocess.run([CLI, "--dump-reads", "-f" if fmt == FASTA else "-q", "--seed", str(seed), "-5", str(t5), "-3", str(t3), "-U", f.name], capture_output=True)
    if r.returncode != 0:
        return None
    out = []
    for ln in r.stdout.split(b"\n")[:-1]:
        name, seq, qual, sd = ln.rsplit(b"\t", 3)
        out.append((read_id(name), seq.decode(), qual, int(sd)))
    return out


def device_reads(got, fmt):
    out = []
    buf = got["buf"]
    for r in range(got["n_reads"]):
        n = int(got["rlen"][r])
        s = "".join("N" if (got["nmask"][r][i // 32] >> (i % 32)) & 1 else "ACGT"[(got["bases"][r][i // 32] >> (2 * (i % 32))) & 3] for i in range(n))
        q = buf[int(got["qualOff"][r]):int(got["qualOff"][r]) + n] if fmt == FASTQ else b"I" * n
        out.append((buf[int(got["idOff"][r]):int(got["idOff"][r]) + int(got["idLen"][r])], s, q, int(got["seeds"][r])))
    return out


@pytest.mark.parametrize("fmt", [FASTA, FASTQ], ids=["fasta", "fastq"])
def test_damaged_blocks_are_either_refused_or_parsed_as_the_host_parser_does(wave64, fmt):
    """the safety property of the plain form, with trims: if the device takes a block, its reads are the host parser's"""
    rng = np.random.default_rng(2025 + fmt)
    junk = [b"\r", b">", b"@", b"+", b"\n", b".", b"-", b"R", b"n", b" ", b"\t", b"/", b"/1", b"\n\n", b"*", b"a", b"\x00", b"\xff"]
    taken = 0
    for trial in range(120):
        t5, t3 = [(1, 0), (0, 1), (5, 0), (3, 4), (13, 9)][trial % 5]
        recs = make_records(rng, int(rng.integers(1, 8)), t5 + t3 + 2, lengths=[20, 33, 40, 64, 70])
        text = bytearray(as_text(recs, fmt, int(rng.choice([0, 0, 5])) if fmt == FASTA else 0))
        for _ in range(int(rng.integers(0, 3))):
            at = int(rng.integers(0, len(text) + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                text[at:at] = junk[int(rng.integers(0, len(junk)))]
            elif kind == 1 and at < len(text):
                del text[at:at + int(rng.integers(1, 4))]
            elif at < len(text):
                text[at:at + 1] = junk[int(rng.integers(0, len(junk)))]
        text = bytes(text)
        flags, got = emu_texttrim.upload([text], fmt, t5, t3, 0, 0, 0, wave64, rec_cap=text.count(b">") + text.count(b"\n") + 16)
        if flags:
            continue
        taken += 1
        want = host_parse(text, fmt, t5, t3)
        assert want is not None and device_reads(got, fmt) == want, (trial, text)
    assert taken >= 20                                         # (the comparison did run)


@pytest.mark.parametrize("fmt,wrap", VARIANTS, ids=["fastq", "fasta", "fasta-wrap7", "fasta-wrap60"])
def test_no_trim_and_no_skip_is_what_it_was(wave64, fmt, wrap):
    """the fields at zero: the outputs of the harness that builds DTextRec without them (tests/emu/emu.cpp), bit for bit"""
    was = emu.use_wave64(wave64)
    try:
        L = emu.lib()
        L.emu_text_parse.restype = C.c_uint32
        L.emu_text_parse.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32] + [C.c_void_p] * 6
        L.emu_text_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rng = np.random.default_rng(3 + fmt + wrap)
        text = as_text(make_records(rng, N_REC, 0), fmt, wrap)
        flags, got = emu_texttrim.upload([text], fmt, 0, 0, 0, 0, 99, wave64)
        assert flags == 0
        buf = np.zeros(len(got["buf"]), dtype=np.uint8)
        buf[:len(text)] = np.frombuffer(text, dtype=np.uint8)
        cap = N_REC + 16
        arr = [np.zeros(cap + 80, dtype=np.uint32) for _ in range(5)]
        status = np.zeros(4, dtype=np.uint64)
        n = L.emu_text_parse(buf.ctypes.data, len(text), fmt, 99, cap if fmt == FASTA else 4 * cap, cap, *[a.ctypes.data for a in arr], status.ctypes.data)
        assert n == N_REC == got["n_reads"] and not status[3]
        for k, a in zip(("rlen", "seeds", "seqOff", "idOff", "idLen"), arr):
            assert (a[:n] == got[k]).all(), k
        assert (int(status[0]), int(status[1]), int(status[2])) == (got["n_words"], got["n_bases"], got["max_len"])
        nw = got["n_words"]
        bases, nmask = np.zeros(nw + 1, dtype=np.uint64), np.zeros(nw + 1, dtype=np.uint32)
        L.emu_text_pack(buf.ctypes.data, n, arr[2].ctypes.data, arr[0].ctypes.data, bases.ctypes.data, nmask.ctypes.data)
        assert bases[:nw].tolist() == [w for r in got["bases"] for w in r] and nmask[:nw].tolist() == [m for r in got["nmask"] for m in r]
    finally:
        emu.use_wave64(was)
