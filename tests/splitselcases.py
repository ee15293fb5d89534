"""What --un / --al / --un-conc / --al-conc write under --split-taxids, as a Python statement — shared by the tests of the read
splitter's size pass by a selection of taxa (split_sel_size_body): the CPU harness (tests/test_splitsel_emu.py) and the device
(tests/test_gpu_splitsel.py).

The rule: every PRINTED row has a class of its own — `al` when the selection's mask holds a 1 for the row's dense taxon (the one row
of a query without rows: the mask's last entry, taxID 0's), `un` otherwise — and its record goes to the sinks of that class.  The
batches are splitcases.make_batch's with a dense taxon per row, the files are splitcases.contract's of the rows so classed."""
import numpy as np

import splitcases
from splitcases import AL, UN, UNWRITTEN, sink_keys      # noqa: F401

N_TAXA = 37
# the taxa of a query's first row, of the rows between, of the last row of a query with several: three ranges that do not meet, so
# that a mask can select "the first row of each query only" or "the last row only"
FIRST, MIDDLE, LAST = range(0, 12), range(12, 24), range(24, 36)
# rows per query: none, one, two, five and the narrow rows' six-bit limit
PATTERNS = dict(splitcases.PATTERNS)
PATTERNS["rows0_1_2_5_63"] = lambda q: (0, 1, 2, 5, 63)[q % 5]


def taxon_of(seed, q, i, n):
    """the dense taxon of row i of query q's n rows.  Now and then one that is no taxon of the table (the formatter prints such a
    row as taxon 0, and so the splitter classes it)"""
    group = FIRST if i == 0 else LAST if i == n - 1 else MIDDLE
    if (q * 7 + i * 3 + seed) % 29 == 0:
        return N_TAXA + 1 + (q & 1) * 1000000
    return group[(q * 5 + i * 11 + seed) % len(group)]


def make_batch(nq, pattern, paired, fastq, seed, **kw):
    """splitcases.make_batch and the rows' 16 bytes -> batch, rows (one tuple OBJECT per query, repeated per printed row), rows16
    (u32 [n, 4]: uniqueID, dense taxon, score, hitLength), printed (per printed row its place in a mask)"""
    batch, rows = splitcases.make_batch(nq, pattern, paired, fastq, seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    rows16, printed = [], []
    for q in range(nq):
        n = int(batch["qinfo"][q]) & 0x3f
        if n == 0:
            printed.append(N_TAXA)
        for i in range(n):
            t = taxon_of(seed, q, i, n)
            rows16.append((int(rng.integers(0, 1 << 32)), t, int(rng.integers(0, 1 << 20)), int(rng.integers(0, 300))))
            printed.append(t if t < N_TAXA else 0)
    assert len(printed) == len(rows)
    return batch, rows, np.array(rows16, dtype=np.uint32).reshape(-1, 4), printed


def _mask(pred, zero):
    return np.array([1 if pred(t) else 0 for t in range(N_TAXA)] + [int(zero)], dtype=np.uint8)


MASKS = {
    "all": _mask(lambda t: True, True),
    "none": _mask(lambda t: False, False),
    "only-zero": _mask(lambda t: False, True),
    "all-but-zero": _mask(lambda t: True, False),          # today's split: a row is `al` when its read has an assignment
    "every-other": _mask(lambda t: t & 1, False),
    "first-row-only": _mask(lambda t: t in FIRST, False),
    "last-row-only": _mask(lambda t: t in LAST, True),
}


def classed(rows, printed, mask):
    """the printed rows with the class the rule gives each: what splitcases.contract reads"""
    return [(rid, seq, qual, bool(mask[t])) for (rid, seq, qual, _), t in zip(rows, printed)]


def check(run, batch, rows, rows16, printed, mask, sinks, cap=None):
    """one batch through one runner — callable (batch, rows16, mask, sinks, cap) -> per sink (the first min(bytes sized, room) bytes
    of its room, the bytes sized, the records, sized) — against the contract.  cap: the room of every sink or four of them (None:
    plenty); a query's records in a sink lie wholly inside its room or are left out together, every other byte is UNWRITTEN"""
    mine = classed(rows, printed, mask)
    per_query, i = [], 0                                     # the contract query by query (a query: a run of one tuple object)
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j] is rows[i]:
            j += 1
        per_query.append(splitcases.contract(mine[i:j]))
        i = j
    want = {k: b"".join(p[k] for p in per_query) for k in splitcases.KEYS}
    caps = [1 << 22] * 4 if cap is None else [cap] * 4 if np.isscalar(cap) else list(cap)
    got = run(batch, rows16, mask, sinks, caps)
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
        assert n_rec == want[key].count(b"\n") // 4, "sink %d (%s): %d records, %d expected" % (s, key, n_rec, want[key].count(b"\n") // 4)
        room = min(caps[s], len(want[key]))
        assert len(text) == room
        img, at = bytearray([UNWRITTEN]) * room, 0
        for p in per_query:
            recs = p[key]
            if recs and at + len(recs) <= room:
                img[at:at + len(recs)] = recs
            at += len(recs)
        assert text == bytes(img), "sink %d (%s) differs" % (s, key)
    return got
