"""Worker of tests/test_gpu_classify_edges.py: ONE process = one group of tests/classifycases.py under one table configuration
(and the kernel knobs of its environment): `python classify_edge_worker.py spec.json`.  For each case of the group it builds the
index on the GPU (capi.build_index), stops unless the files are the reference builder's (tests/golden/build_edges.json), opens the
index with the configuration and classifies the case's reads; rows, counters, launch records, op counters, `info` and
cf_index_describe go into one .npz.  Nothing about the rows is asserted here: the parent compares.

The reads of a run are classified one strand-record class at a time (<= 128, <= 192, <= 256 bases, longer: sizeBatch picks the
record size from a batch's longest read, and one 300-base read would send every read to the byte-window kernel), through the byte
form (clf.batch, twice: the second pass plans again over the resident batch) and through the packed slot form (Slot.submit / wait);
under configuration A the ten random 100-base reads also go through submit_dense + wait_narrow.  At -t 1 the 193 ... 256 class is
classified again with every read cut to 217, 219 and 220 bases: sizeBatch gives up the 8-bit hit count of the strand records at
0.15 L + L / ftabChars + 3 >= 255, which at -t 1 is L = 220."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import buildcases as B  # noqa: E402
import classifycases as K  # noqa: E402
from centrifuge_amd import capi  # noqa: E402
from variant_worker import load_result, ops_dict, save_result  # noqa: E402,F401

CUTS = (217, 219, 220)

# ---- table configurations: name -> (cf_index_options of a case, environment)
GENERAL = {"CF_POST_FAST": "0", "CF_SCORE_FAST": "0"}
CONFIGS = {
    "A": ("A", {}), "B": ("B", {}), "C": ("C", {}), "D": ("D", {}), "W1": ("W1", {}), "W6": ("W6", {}),
    "A_general": ("A", GENERAL), "B_general": ("B", GENERAL), "A_v1": ("A", {"CF_SEARCH_V": "1"}),
}


def wide_asked(tables, ftab_chars):
    return ftab_chars + 1 if tables == "W1" else min(ftab_chars + 6, 12) if tables == "W6" else 0


def index_opts(tables, ftab_chars):
    """cf_index_options: 0 = automatic, -1 = off; resolve_rate holds rate + 1"""
    if tables == "A":
        return dict(small_range_rows=-1)
    if tables == "B":
        return dict(wide_ftab_chars=-1, text_verify_rate=-1, occ_planes=-1, resolve_rate=-1, pair_planes=-1, small_range_rows=-1)
    if tables == "C":
        return dict(small_range_rows=4)
    if tables == "D":
        return dict(text_verify_rate=3, resolve_rate=4, small_range_rows=-1)
    k = wide_asked(tables, ftab_chars)
    return dict(wide_ftab_chars=k if k > ftab_chars else -1, small_range_rows=-1)


def expected_tables(tables, n, ftab_chars, off_rate):
    """what planTablesIn (cf_device.hip) realises for a text of n bases with room to spare, from its thresholds alone: text tables
    only for n >= 64; an automatic wide ftab of kAuto = floor(log4 n) characters where that exceeds the file's; a resolve rate only
    below offRate; a fixed wide ftab whenever it is wider than the file's"""
    k_auto, m = 0, n
    while m >= 4:
        k_auto, m = k_auto + 1, m >> 2
    if tables == "B":
        return dict(wide_ftab_chars=0, text_verify_rate=-1, occ_planes=0, pair_planes=0, resolve_rate=off_rate, small_range_rows=0)
    e = dict(occ_planes=1, pair_planes=1, small_range_rows=4 if tables == "C" and n >= 64 else 0)      # (small ranges are finished against the text)
    e["text_verify_rate"] = -1 if n < 64 else 3 if tables == "D" else 0
    e["resolve_rate"] = min(3, off_rate) if tables == "D" else 0
    k = wide_asked(tables, ftab_chars)
    e["wide_ftab_chars"] = (k if k > ftab_chars else 0) if tables.startswith("W") else (k_auto if k_auto > ftab_chars else 0)
    return e


def class_batches(lens):
    """[(class, read indices)] of an unpaired run: the reads of each strand-record class, in order"""
    cls = np.array([K.length_class(int(x)) for x in lens])
    return [(k, np.nonzero(cls == k)[0]) for k in range(len(K.CLASS_EDGES)) if np.any(cls == k)]


def subset(seq, off, seeds, idx, per=1, cut=None):
    """the reads idx (queries of `per` reads) as arrays of their own, each cut to `cut` bases"""
    rs = []
    for q in idx:
        for r in range(per * int(q), per * int(q) + per):
            x = seq[int(off[r]):int(off[r + 1])]
            rs.append(x[:cut] if cut else x)
    o = np.zeros(len(rs) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in rs])
    s = np.concatenate(rs).astype(np.uint8) if o[-1] else np.zeros(1, dtype=np.uint8)
    ridx = np.concatenate([np.arange(per * int(q), per * int(q) + per) for q in idx]) if len(idx) else np.zeros(0, dtype=np.int64)
    return np.ascontiguousarray(s), o, np.ascontiguousarray(seeds[ridx])


def run_arrays(c, paired):
    return K.load_arrays(c.reads, c.mate2 if paired else None)


def classify_run(ix, c, rid, paired, tables, pre, arrays):
    names, qlens, seq, off, seeds, pr = run_arrays(c, paired)
    nq, k = len(names), K.RUN_KW[rid]["k"]
    lens = (off[1:] - off[:-1]).astype(np.int64)
    parts = [(0, np.arange(nq))] if paired else class_batches(lens)
    per = 2 if paired else 1
    m = {"nq": nq, "batches": []}
    rows, n_rows, score2 = np.zeros((nq, k), dtype=capi.ROW_DTYPE), np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    rows2, n_rows2, score22 = rows.copy(), n_rows.copy(), score2.copy()
    rows3, n_rows3, score23 = rows.copy(), n_rows.copy(), score2.copy()
    clf = capi.Classifier(ix, **K.RUN_KW[rid])
    live = []
    for cls, idx in parts:
        s, o, sd = subset(seq, off, seeds, idx, per)
        b = clf.batch(s, o, sd, pr)
        b.classify()
        rows[idx], n_rows[idx], score2[idx] = b.results()
        m["batches"].append(dict(cls=int(cls), nq=len(idx), max_len=int(lens.max(initial=0) if paired else lens[idx].max()), info=b.info(), launch=b.launch_record(),
                                 ops=ops_dict(b.opcounts())))
        live.append((b, idx))
    arrays[pre + "counts_reads"], arrays[pre + "counts_uniq"] = clf.counts()
    for j, (b, idx) in enumerate(live):               # the second pass over the resident batches
        b.plan()
        b.classify()
        rows2[idx], n_rows2[idx], score22[idx] = b.results()
        m["batches"][j]["info2"], m["batches"][j]["launch2"] = b.info(), b.launch_record()
    arrays[pre + "counts2_reads"], arrays[pre + "counts2_uniq"] = clf.counts()
    for b, _ in live:
        b.close()
    clf.close()
    # the packed slot form
    clf = capi.Classifier(ix, **K.RUN_KW[rid])
    slot = capi.Slot(clf)
    for cls, idx in parts:
        s, o, sd = subset(seq, off, seeds, idx, per)
        bs, mk, ln = capi.pack_reads(s, o)
        slot.submit(bs, mk, ln, sd, paired=pr)
        r, first, nr, s2, _ms, _info = slot.wait()
        rows3[idx], n_rows3[idx], score23[idx] = capi.unpack_rows(r, first, nr, k), nr, s2
    # reads of one length, four bases a byte, narrow results
    if tables == "A" and rid == "k5" and not paired:
        idx = np.array([i for i, (nm, r) in enumerate(c.reads) if nm.startswith(b"rand") and len(r) == 100])
        s, o, sd = subset(seq, off, seeds, idx)
        slot.set_result_format(capi.RESULTS_NARROW)
        b4, ni, nm = capi.dense_pack(s[:int(o[-1])].reshape(len(idx), 100))
        slot.submit_dense(b4, sd, 100, nwords=(ni, nm))
        r, nr, s2, _ms, _info = slot.wait_narrow(expand=(None, 100, False))
        first = np.concatenate([[0], np.cumsum(nr)]).astype(np.uint64)
        arrays[pre + "dense_idx"], arrays[pre + "dense_rows"], arrays[pre + "dense_n_rows"], arrays[pre + "dense_score2"] = idx, capi.unpack_rows(r, first, nr, k), nr, s2
    slot.close()
    # either side of the 8-bit hit count of the strand records (-t 1)
    if c.build.ftab_chars == 1 and rid == "k5" and not paired:
        idx = dict(parts)[2]
        m["cuts"] = {}
        for cut in CUTS:
            s, o, sd = subset(seq, off, seeds, idx, cut=cut)
            b = clf.batch(s, o, sd, False)
            b.classify()
            arrays[pre + "cut%d_rows" % cut], arrays[pre + "cut%d_n_rows" % cut], arrays[pre + "cut%d_score2" % cut] = b.results()
            m["cuts"][str(cut)] = b.launch_record()
            b.close()
        arrays[pre + "cut_idx"] = idx
    clf.close()
    for nm, a in (("rows", rows), ("n_rows", n_rows), ("score2", score2), ("rows2", rows2), ("n_rows2", n_rows2), ("score22", score22),
                  ("rows3", rows3), ("n_rows3", n_rows3), ("score23", score23)):
        arrays[pre + nm] = a
    return m


def main(spec_path):
    spec = json.load(open(spec_path))
    t0 = time.time()
    tables = CONFIGS[spec["config"]][0]
    golden = B.load_golden()
    meta = {"id": spec["id"], "knobs": {k: v for k, v in os.environ.items() if k.startswith("CF_")}, "cases": {}}
    arrays = {}
    for name in spec["cases"]:
        c = K.BY_NAME[name]
        t1 = time.time()
        d = os.path.join(spec["index_dir"], name)
        tax = c.build.write(d)
        via = c.build.vias[0]
        src = dict(fasta=[os.path.join(d, "genomes.fa")]) if via == "fasta" else c.build.memory()
        base = os.path.join(d, "idx")
        os.environ.update({k: str(v) for k, v in c.build.env.items()})
        try:
            capi.build_index(base, **src, **tax, **c.build.build_kwargs())
        finally:
            for k in c.build.env:
                del os.environ[k]
        if B.index_digest(base) != golden[name]["files"]:
            raise SystemExit("%s: the index built here is not the reference builder's" % name)
        ix = capi.Index(base, device=0, **index_opts(tables, c.build.ftab_chars))
        m = dict(describe=dict(ix.describe(), walk_bound=int(ix.L.cf_index_walk_bound(ix.h)), wide_ftab_chars=int(ix.L.cf_index_wide_ftab_chars(ix.h))),
                 num_taxa=int(ix.num_taxa), runs={})
        for rid, _args, paired in c.runs():
            m["runs"][rid] = classify_run(ix, c, rid, paired, tables, "%s.%s." % (name, rid), arrays)
        ix.close()
        m["seconds"] = time.time() - t1
        meta["cases"][name] = m
    meta["seconds"] = time.time() - t0
    save_result(spec["out"], meta, arrays)


if __name__ == "__main__":
    main(sys.argv[1])
