"""What cf_batch_upload_text and the plan stage's pack pass do with FASTA / FASTQ blocks, in the CPU harness (tests/emu/emu.cpp:
emu_text_parse2, emu_text_pack; TEST ONLY): the calls tests/test_textio_emu.py and tests/test_gpu_textcases.py share."""
import ctypes as C

import numpy as np

from . import emu

PAD = 128
FASTA, FASTQ = 0, 1
FILL = 0xdeadbeef
MARGIN = 80
POS_MARGIN_HIT = 1 << 63                                   # emu_text_parse2: a marker was written behind posCap


def lib(wave64=False):
    """the harness build asked for (and emu's setting left as it was)"""
    was = emu.use_wave64(wave64)
    try:
        L = emu.lib()
    finally:
        emu.use_wave64(was)
    L.emu_text_parse.restype = C.c_uint32
    L.emu_text_parse.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32] + [C.c_void_p] * 6
    L.emu_text_parse2.restype = C.c_uint32
    L.emu_text_parse2.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32] * 3
    L.emu_text_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def padded(text):
    a = np.zeros(len(text) + PAD + 64, dtype=np.uint8)
    a[:len(text)] = np.frombuffer(text, dtype=np.uint8)
    return a


def decode(words, nmask, rlen):
    """the reads' bases (str each) from the packed 2-bit words and the N masks, read r's words behind those of the reads before it"""
    words, nmask = np.asarray(words, dtype=np.uint64), np.asarray(nmask, dtype=np.uint32)
    sh = np.arange(32, dtype=np.uint64)
    code = ((words[:, None] >> (2 * sh)) & np.uint64(3)).astype(np.uint8)
    isn = ((nmask[:, None].astype(np.uint64) >> sh) & np.uint64(1)).astype(bool)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[code]
    letters[isn] = ord("N")
    flat = letters.reshape(-1).tobytes()
    out, w = [], 0
    for n in (int(x) for x in rlen):
        out.append(flat[32 * w:32 * w + n].decode())
        w += (n + 31) // 32
    return out


def encode(seqs):
    """the packed words and N masks of reads given as strings of A C G T N (an N's field of the word is zero)"""
    words, masks = [], []
    for s in seqs:
        a = np.frombuffer(s.encode(), dtype=np.uint8)
        code = np.zeros(len(a), dtype=np.uint64)
        for k, c in enumerate(b"ACGT"):
            code[a == c] = k
        n = (a == ord("N"))
        pad = -len(a) % 32
        code = np.concatenate([code, np.zeros(pad, dtype=np.uint64)]).reshape(-1, 32)
        n = np.concatenate([n, np.zeros(pad, dtype=bool)]).reshape(-1, 32)
        sh = np.arange(32, dtype=np.uint64)
        words.append((code << (2 * sh)).sum(axis=1, dtype=np.uint64))
        masks.append((n.astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64).astype(np.uint32))
    if not words:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    return np.concatenate(words), np.concatenate(masks)


def flags_of(L, text, fmt, seed=0, rec_cap=None, pos_cap=None):
    return parse(L, text, fmt, seed, rec_cap, pos_cap)[0]


def parse(L, text, fmt, seed=0, rec_cap=None, pos_cap=None):
    """-> (flags, reads) with reads = list of (readID bytes, bases str, seed) made from the bodies' outputs; the per-record arrays
    hold rec_cap records and a filled margin behind them, which must come back as it was"""
    buf = padded(text)
    rec_cap = rec_cap if rec_cap is not None else (text.count(b">") if fmt == FASTA else text.count(b"\n") // 4) + 16
    pos_cap = pos_cap if pos_cap is not None else (rec_cap if fmt == FASTA else 4 * rec_cap)
    arr = [np.full(rec_cap + MARGIN, FILL, dtype=np.uint32) for _ in range(5)]
    status = np.zeros(4, dtype=np.uint64)
    n = L.emu_text_parse(vp(buf), len(text), fmt, seed, pos_cap, rec_cap, *[vp(a) for a in arr], vp(status))
    flags = int(status[3])
    assert not flags & POS_MARGIN_HIT, "a marker was written behind posCap"
    for a in arr:
        assert (a[rec_cap:] == FILL).all(), "a record was written behind recCap"
    if flags:
        return flags, None
    assert n <= rec_cap
    rlen, seeds, seq_off, id_off, id_len = [a[:n] for a in arr]
    assert int(status[0]) == int(((rlen.astype(np.uint64) + 31) // 32).sum()) and int(status[1]) == int(rlen.sum())
    assert int(status[2]) == (int(rlen.max()) if n else 0)
    n_words = int(status[0])
    bases, nmask = np.zeros(n_words + 1, dtype=np.uint64), np.zeros(n_words + 1, dtype=np.uint32)
    L.emu_text_pack(vp(buf), n, vp(seq_off), vp(rlen), vp(bases), vp(nmask))
    seqs = decode(bases[:n_words], nmask[:n_words], rlen)
    ew, em = encode(seqs)
    assert np.array_equal(ew, bases[:n_words]) and np.array_equal(em, nmask[:n_words])      # (an N's field of the word is zero)
    return 0, [(bytes(text[int(id_off[r]):int(id_off[r]) + int(id_len[r])]), seqs[r], int(seeds[r])) for r in range(n)]


def parse_mates(L, t1, t2, fmt, seed=0):
    """two blocks of mates in one buffer, as cf_batch_upload_text lays them out -> (flags, reads): record r of block m is read 2 r + m"""
    at2 = (len(t1) + 63) // 64 * 64 + PAD
    buf = np.zeros(at2 + len(t2) + PAD + 64, dtype=np.uint8)
    buf[:len(t1)] = np.frombuffer(t1, dtype=np.uint8)
    buf[at2:at2 + len(t2)] = np.frombuffer(t2, dtype=np.uint8)
    caps = [len(t) // 32 + 1024 for t in (t1, t2)]
    arr = [np.full(2 * max(caps) + MARGIN, FILL, dtype=np.uint32) for _ in range(5)]
    status = np.zeros(4, dtype=np.uint64)
    got = []
    for m, (t, at) in enumerate(((t1, 0), (t2, at2))):
        got.append(L.emu_text_parse2(buf.ctypes.data + at, len(t), fmt, seed, caps[m] if fmt == FASTA else 4 * caps[m], caps[m], *[vp(a) for a in arr], vp(status), at, 2, m))
    flags = int(status[3])
    assert not flags & POS_MARGIN_HIT
    if flags:
        return flags, None
    assert got[0] == got[1]
    n = 2 * got[0]
    for a in arr:
        assert (a[n:] == FILL).all()
    rlen, seeds, seq_off, id_off, id_len = [a[:n] for a in arr]
    n_words = int(((rlen.astype(np.uint64) + 31) // 32).sum())
    assert int(status[0]) == n_words and int(status[1]) == int(rlen.sum()) and int(status[2]) == int(rlen.max())
    bases, nmask = np.zeros(n_words + 1, dtype=np.uint64), np.zeros(n_words + 1, dtype=np.uint32)
    L.emu_text_pack(vp(buf), n, vp(seq_off), vp(rlen), vp(bases), vp(nmask))
    seqs = decode(bases[:n_words], nmask[:n_words], rlen)
    whole = bytes(buf)
    return 0, [(whole[int(id_off[r]):int(id_off[r]) + int(id_len[r])], seqs[r], int(seeds[r])) for r in range(n)]
