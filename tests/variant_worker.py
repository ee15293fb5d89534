"""Worker of tests/test_gpu_variants.py: ONE process = one kernel variant.  The library reads its kernel-variant knobs
(centrifuge_amd/csrc/cf_knobs.hpp) once per process, so the parent starts this script with the variant's CF_* variables in the
environment: `python variant_worker.py spec.json`.  It opens the indexes the spec names, classifies the listed inputs through
centrifuge_amd.capi and writes rows, counters, op counts, the `info` dict and the launch record (cf_batch_debug_launch) into one
.npz.  Nothing is asserted about correctness here: the parent compares, so that a failure shows in pytest's output.

The spec (JSON): {"id", "out", "index_opts": {cf_index_options field: value}, "kreport": bool, "in_flight": bool,
"rows_per_pass_div": int, "planned_per_query": [input id, ...], "inputs": [input, ...]} with an input one of
    {"kind": "golden", "arch": ..., "name": ...}      a golden case's reads and options
    {"kind": "edge", "idx": i}                        common.EDGE_CASES[i] (seeds as tests/test_gpu_parity.py)
    {"kind": "replicated", "copies": R}               synth_small's reads.fa R times, each copy shuffled
build_input() makes the arrays; the parent imports it to compute what it compares against."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import common  # noqa: E402
from centrifuge_amd import capi, reads  # noqa: E402

OPS = ("n_ftab", "n_pair", "n_pair2", "n_single", "n_walk", "n_rows", "n_ftab_wide", "n_verify", "n_text_loads", "n_pos_hits")


def input_id(inp):
    if inp["kind"] == "golden":
        return "%s/%s" % (inp["arch"], inp["name"])
    if inp["kind"] == "edge":
        return "edge%d" % inp["idx"]
    return "rep%d" % inp["copies"]


def pack(rs):
    """list of code arrays -> (seq u8, off u64)"""
    off = np.zeros(len(rs) + 1, dtype=np.uint64)
    if rs:
        off[1:] = np.cumsum([len(r) for r in rs])
    seq = np.concatenate(rs).astype(np.uint8) if rs and off[-1] else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(seq), off


def build_input(inp):
    """-> dict(arch, kw (classifier options), seq, off, seeds, paired, nq; names, qlens for a golden case; perm for a replicated one)"""
    if inp["kind"] == "golden":
        d, cases = common.golden(inp["arch"])
        c = [x for x in cases if x["name"] == inp["name"]][0]
        kw, fastq = common.case_kwargs(c["args"])
        names, qlens, seq, off, seeds, paired = reads.load([os.path.join(d, f) for f in c["reads"]], fastq)
        return dict(arch=inp["arch"], kw=kw, seq=seq, off=off, seeds=np.ascontiguousarray(seeds, dtype=np.uint32), paired=bool(paired),
                    nq=len(names), names=names, qlens=qlens, case=c, dir=d)
    d, _ = common.golden("synth_small")
    if inp["kind"] == "edge":
        lengths, paired, k = common.EDGE_CASES[inp["idx"]]
        recs = reads.read_fasta(os.path.join(d, "reads.fa")) + reads.read_fasta(os.path.join(d, "reads250.fa"))
        rng = np.random.default_rng(11)
        rs = common.edge_reads(recs, lengths, rng)
        if paired and len(rs) % 2:
            rs.append(rs[0])
        seq, off = pack(rs)
        seeds = rng.integers(0, 2 ** 32, size=len(rs), dtype=np.uint32)
        return dict(arch="synth_small", kw={"k": k}, seq=seq, off=off, seeds=seeds, paired=paired, nq=len(rs) // 2 if paired else len(rs), dir=d)
    names, qlens, seq, off, seeds, paired = reads.load([os.path.join(d, "reads.fa")], False)
    n = len(names)
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(n) for _ in range(inp["copies"])])
    lens = (off[1:] - off[:-1]).astype(np.int64)
    off2 = np.zeros(len(perm) + 1, dtype=np.uint64)
    off2[1:] = np.cumsum(lens[perm])
    seq2 = np.concatenate([seq[int(off[i]):int(off[i + 1])] for i in perm])
    return dict(arch="synth_small", kw={}, seq=seq2, off=off2, seeds=np.ascontiguousarray(seeds, dtype=np.uint32)[perm], paired=False, nq=len(perm), perm=perm,
                base=dict(kind="golden", arch="synth_small", name="k5"), dir=d)


def save_result(path, meta, arrays):
    """meta (JSON-able) and arrays (name -> ndarray, structured dtypes included) into one .npz, written whole or not at all"""
    tmp = path + ".tmp.npz"
    np.savez(tmp, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    os.replace(tmp, path)


def load_result(path):
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files if k != "__meta__"}
        meta = json.loads(z["__meta__"].tobytes().decode())
    return meta, arrays


def ops_dict(o):
    return {f: int(getattr(o, f)) for f in OPS}


def run_input(ix, x, spec, pre, arrays):
    """the one-shot path twice (classify; plan + classify again), then what the spec asks for on top -> the input's meta"""
    m = {}
    clf = capi.Classifier(ix, **x["kw"])
    if spec.get("kreport"):
        clf.enable_kreport()
    b = clf.batch(x["seq"], x["off"], x["seeds"], x["paired"])
    b.classify()
    arrays[pre + "rows"], arrays[pre + "n_rows"], arrays[pre + "score2"] = b.results()
    m["info"], m["launch"] = b.info(), b.launch_record()
    arrays[pre + "counts_reads"], arrays[pre + "counts_uniq"] = clf.counts()
    arrays[pre + "counts_single"] = clf.counts_single()
    if spec.get("kreport"):
        arrays[pre + "kreport"], m["kreport_reads"] = clf.kreport_counts()
    m["ops"] = ops_dict(b.opcounts())
    # a second pass over the resident batch: plan and strand records made again, then the stages; the packed egress
    m["plan_ms"] = b.plan()
    b.classify()
    arrays[pre + "rows2"], arrays[pre + "n_rows2"], arrays[pre + "score22"] = b.results()
    arrays[pre + "crows"], _first, arrays[pre + "cn_rows"], arrays[pre + "cscore2"] = b.results_compact()
    m["info2"], m["launch2"] = b.info(), b.launch_record()
    arrays[pre + "counts2_reads"], arrays[pre + "counts2_uniq"] = clf.counts()
    b.close(); clf.close()

    bs, mk, ln = None, None, None
    if spec.get("rows_per_pass_div") or spec.get("in_flight"):
        bs, mk, ln = capi.pack_reads(x["seq"], x["off"])
    if spec.get("rows_per_pass_div"):
        # a row workspace of a fraction of what the batch plans: cf_batch_wait finishes it in further passes of the row stage
        clf = capi.Classifier(ix, **x["kw"])
        slot = capi.Slot(clf)
        slot.set_limits(rows_per_pass=max(1, int(m["info"]["planned_sa_rows"]) // int(spec["rows_per_pass_div"])))
        slot.submit(bs, mk, ln, x["seeds"], paired=x["paired"])
        rows, first, n_rows, score2, _ms, info = slot.wait()
        arrays[pre + "lim_rows"], arrays[pre + "lim_n_rows"], arrays[pre + "lim_score2"] = rows, n_rows, score2
        m["lim_info"], m["lim_launch"] = info, slot.launch_record()
        arrays[pre + "lim_counts_reads"], arrays[pre + "lim_counts_uniq"] = clf.counts()
        slot.close(); clf.close()
    if spec.get("in_flight"):
        # two slots on one stream, each three times.  The ABI refuses an upload into a slot whose batch has not been waited for
        # ("the slot still has a batch in flight": the next batch would overwrite buffers the kernels still read), so a slot cannot
        # take its own next batch without a host sync; what it allows is a second slot: a slot is submitted again as soon as it was
        # waited for, while the other's batch is still in flight behind it — every event join of a batch is crossed by the batch
        # that follows on the stream
        clf = capi.Classifier(ix, **x["kw"])
        st = capi.C.c_void_p()
        capi._check(clf.L.cf_stream_create(0, capi.C.byref(st)))
        slots = [capi.Slot(clf), capi.Slot(clf)]
        for s in slots:
            s.submit(bs, mk, ln, x["seeds"], paired=x["paired"], stream=st)
        runs = 0
        m["fl_info"], m["fl_launch"] = [], []
        for rnd in range(3):
            for s in slots:
                rows, first, n_rows, score2, _ms, info = s.wait()
                arrays[pre + "fl%d_rows" % runs], arrays[pre + "fl%d_n_rows" % runs], arrays[pre + "fl%d_score2" % runs] = rows, n_rows, score2
                m["fl_info"].append(info); m["fl_launch"].append(s.launch_record())
                runs += 1
                if rnd < 2:
                    s.submit(bs, mk, ln, x["seeds"], paired=x["paired"], stream=st)
        m["fl_runs"] = runs
        arrays[pre + "fl_counts_reads"], arrays[pre + "fl_counts_uniq"] = clf.counts()
        for s in slots:
            s.close()
        clf.close()
        clf.L.cf_stream_destroy(st)
    return m


def planned_per_query(ix, x, n=300):
    """planned SA rows of each of the input's first n queries: every query once more as a batch of its own, through one slot"""
    clf = capi.Classifier(ix, **x["kw"])
    slot = capi.Slot(clf)
    per = 2 if x["paired"] else 1
    off = x["off"]
    out = np.zeros(min(n, x["nq"]), dtype=np.uint64)
    for q in range(len(out)):
        r0, r1 = q * per, (q + 1) * per
        o = (off[r0:r1 + 1] - off[r0]).astype(np.uint64)
        s = x["seq"][int(off[r0]):int(off[r1])] if off[r1] > off[r0] else np.zeros(1, dtype=np.uint8)
        slot.submit_bytes(s, o, x["seeds"][r0:r1], x["paired"])
        out[q] = slot.wait()[5]["planned_sa_rows"]
    slot.close(); clf.close()
    return out


def main(spec_path):
    spec = json.load(open(spec_path))
    t0 = time.time()
    meta = {"id": spec["id"], "knobs": {k: v for k, v in os.environ.items() if k.startswith("CF_")}, "inputs": [], "index": {}}
    arrays, idx = {}, {}
    for i, inp in enumerate(spec["inputs"]):
        x = build_input(inp)
        if x["arch"] not in idx:
            ix = capi.Index(os.path.join(x["dir"], "idx"), device=0, **spec.get("index_opts", {}))
            idx[x["arch"]] = ix
            meta["index"][x["arch"]] = dict(ix.describe(), num_taxa=int(ix.num_taxa), walk_bound=int(ix.L.cf_index_walk_bound(ix.h)),
                                            wide_ftab_chars=int(ix.L.cf_index_wide_ftab_chars(ix.h)))
        t1 = time.time()
        m = run_input(idx[x["arch"]], x, spec, "in%d." % i, arrays)
        if input_id(inp) in spec.get("planned_per_query", []):
            arrays["in%d.planned" % i] = planned_per_query(idx[x["arch"]], x)
        m.update(id=input_id(inp), nq=int(x["nq"]), n_reads=int(len(x["off"]) - 1), seconds=time.time() - t1)
        meta["inputs"].append(m)
    for ix in idx.values():
        ix.close()
    meta["seconds"] = time.time() - t0
    save_result(spec["out"], meta, arrays)


if __name__ == "__main__":
    main(sys.argv[1])
