#!/usr/bin/env python3
"""End-to-end wall time of the centrifuge-class front ends (ours vs the reference binary) on one
FASTA file: index built by the GPU builder, reads sampled from the genomes.
usage: cli_e2e.py <genomes> <genome length> <reads> [noref | outbgzf [other centrifuge-class] | kreport [other centrifuge-class] | split [other centrifuge-class]]
(split: --un / --al on the device text path and with --host-io, the run without them, another build's run with them beside those;
outbgzf: our plain output against --out-bgzf, another build's plain run beside them, and gzip -1 of the TSV on 16 cores;
kreport: our plain run against --kreport-file, another build's plain run beside them, then centrifuge-kreport on the TSV)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import bench  # noqa: E402
import synth  # noqa: E402
from centrifuge_amd import capi  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    G, L, n = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    d = "/tmp/cf_e2e"
    os.makedirs(d, exist_ok=True)
    g = bench.gpu_genomes(torch, G, L)
    codes = bench.gpu_sample_reads(torch, g, n, 100, seed=5).cpu().numpy()
    host = g.cpu().numpy()
    del g
    torch.cuda.empty_cache()
    synth.write_taxonomy(d, G)
    capi.build_index(os.path.join(d, "idx"), codes=host.reshape(-1), seq_off=np.arange(G + 1, dtype=np.uint64) * np.uint64(L),
                     seq_names=[b"seq%d x" % i for i in range(G)], conversion_table=os.path.join(d, "conv.tsv"),
                     taxonomy_tree=os.path.join(d, "nodes.dmp"), name_table=os.path.join(d, "names.dmp"))
    bench.write_fasta(os.path.join(d, "reads.fa"), bench.read_names(n), codes)
    ours = os.path.join(ROOT, "centrifuge_amd", "bin", "centrifuge-class")
    ref = os.path.join(O.REF_DIR, "centrifuge-class")
    if len(sys.argv) > 4 and sys.argv[4] == "outbgzf":
        # the plain output against --out-bgzf (rows deflated on the device), three runs of each in turn: whole process, the -t lines
        # (search phase, k_deflate's HIP-event time), the output's bytes = what crosses the link for the rows; then, with a fifth
        # argument, another build's binary (the parent commit's) on the same job; then the plain TSV through gzip -1 on 16 cores
        import shutil
        keep = ("ime", "search", "Device text", "Device deflate")
        forms = [("plain", ours, []), ("out-bgzf", ours, ["--out-bgzf"])] + ([("parent", sys.argv[5], [])] if len(sys.argv) > 5 else [])
        for tag, exe, extra in forms * 3:
            out = os.path.join(d, tag + ".out")
            t0 = time.time()
            r = subprocess.run([exe, "-f", "-t", "-p", "8", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "-S", out,
                                "--report-file", os.path.join(d, tag + ".rep")] + extra, capture_output=True, text=True)
            dt = time.time() - t0
            print("%-9s wall %.2fs -> %.3g reads/s  rc=%d  output %d bytes (%.1f per read) | %s" % (tag, dt, n / dt, r.returncode, os.path.getsize(out), os.path.getsize(out) / n,
                  " ; ".join(l for l in r.stderr.splitlines() if any(k in l for k in keep))), flush=True)
        same = subprocess.run("gzip -dc %s | cmp - %s" % (os.path.join(d, "out-bgzf.out"), os.path.join(d, "plain.out")), shell=True).returncode == 0
        print("inflated output identical to the plain one: %s" % same, flush=True)
        if shutil.which("gzip") and shutil.which("split"):
            parts = os.path.join(d, "parts")
            shutil.rmtree(parts, ignore_errors=True)
            os.makedirs(parts)
            t0 = time.time()
            subprocess.check_call(["split", "-n", "l/16", os.path.join(d, "plain.out"), os.path.join(parts, "p")])
            t1 = time.time()
            ps = [subprocess.Popen(["gzip", "-1", os.path.join(parts, f)]) for f in sorted(os.listdir(parts))]
            ok = all(p.wait() == 0 for p in ps)
            size = sum(os.path.getsize(os.path.join(parts, f)) for f in os.listdir(parts))
            print("gzip -1 of the plain TSV in 16 pieces at once: split %.2fs + gzip %.2fs, %d bytes (%.1f per read) ok=%s" % (t1 - t0, time.time() - t1, size, size / n, ok), flush=True)
            shutil.rmtree(parts, ignore_errors=True)
        return
    if len(sys.argv) > 4 and sys.argv[4] == "kreport":
        # the run without and with --kreport-file (the Kraken-style tally on the device), three runs of each in turn — with a fifth
        # argument another build's binary (the parent commit's) beside them: whole process, the -t lines (search phase, k_kreport's
        # HIP-event time) —, then the second pass the flag replaces: centrifuge-kreport on the TSV the same run wrote
        keep = ("ime", "search", "Device text", "Kraken")
        kr = os.path.join(d, "kreport.txt")
        forms = [("plain", ours, []), ("kreport", ours, ["--kreport-file", kr])] + ([("parent", sys.argv[5], [])] if len(sys.argv) > 5 else [])
        for tag, exe, extra in forms * 3:
            out = os.path.join(d, tag + ".out")
            t0 = time.time()
            r = subprocess.run([exe, "-f", "-t", "-p", "8", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "-S", out,
                                "--report-file", os.path.join(d, tag + ".rep")] + extra, capture_output=True, text=True, timeout=300)
            dt = time.time() - t0
            print("%-9s wall %.2fs -> %.3g reads/s  rc=%d  output %d bytes | %s" % (tag, dt, n / dt, r.returncode, os.path.getsize(out),
                  " ; ".join(l for l in r.stderr.splitlines() if any(k in l for k in keep))), flush=True)
            if r.returncode != 0:
                print(r.stderr[-2000:], flush=True)
                sys.exit(1)
        tool = os.path.join(ROOT, "centrifuge_amd", "bin", "centrifuge-kreport")
        for i in range(2):
            t0 = time.time()
            with open(os.path.join(d, "tool.txt"), "wb") as f:
                rc = subprocess.run([tool, "-x", os.path.join(d, "idx"), os.path.join(d, "kreport.out")], stdout=f, stderr=subprocess.DEVNULL, timeout=900).returncode
            print("centrifuge-kreport on the TSV (%d bytes): wall %.2fs rc=%d" % (os.path.getsize(os.path.join(d, "kreport.out")), time.time() - t0, rc), flush=True)
        same = open(os.path.join(d, "tool.txt"), "rb").read() == open(kr, "rb").read()
        print("--kreport-file identical to centrifuge-kreport's output: %s (%d bytes); TSV identical to the plain run's: %s" % (
            same, os.path.getsize(kr), subprocess.run(["cmp", "-s", os.path.join(d, "plain.out"), os.path.join(d, "kreport.out")]).returncode == 0), flush=True)
        return
    if len(sys.argv) > 4 and sys.argv[4] == "split":
        # --un / --al: another build's binary (the parent commit's, which ignores the two options) with them, this tree with them on the
        # device text path and with --host-io, and this tree without them, three runs of each in turn: whole process, the -t lines
        # (search wall, k_split_*'s HIP-event time per batch), the bytes of the TSV and of the two read files
        keep = ("search wall", "Device text", "Read split")
        un, al = os.path.join(d, "un.fq"), os.path.join(d, "al.fq")
        opts = ["--un", un, "--al", al]
        forms = ([("parent", sys.argv[5], opts)] if len(sys.argv) > 5 else []) + [("split", ours, opts), ("split-host-io", ours, opts + ["--host-io"]), ("plain", ours, [])]
        for tag, exe, extra in forms * 3:
            out = os.path.join(d, tag + ".out")
            for f in (un, al):
                if os.path.exists(f):
                    os.remove(f)
            t0 = time.time()
            r = subprocess.run([exe, "-f", "-t", "-p", "8", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"), "-S", out,
                                "--report-file", os.path.join(d, tag + ".rep")] + extra, capture_output=True, text=True, timeout=600)
            dt = time.time() - t0
            sizes = [os.path.getsize(f) if os.path.exists(f) else -1 for f in (un, al)]
            print("%-13s wall %.2fs -> %.3g reads/s  rc=%d  TSV %d bytes, --un %d, --al %d bytes | %s" % (tag, dt, n / dt, r.returncode, os.path.getsize(out), sizes[0], sizes[1],
                  " ; ".join(l for l in r.stderr.splitlines() if any(k in l for k in keep))), flush=True)
            if r.returncode != 0:
                print(r.stderr[-2000:], flush=True)
                sys.exit(1)
            if tag == "split":
                os.replace(un, un + ".dev"); os.replace(al, al + ".dev")
            if tag == "split-host-io":
                same = all(subprocess.run(["cmp", "-s", f, f + ".dev"]).returncode == 0 for f in (un, al))
                print("read files of the device path and of --host-io identical: %s; TSV identical to the parent's / the plain run's: %s" % (
                    same, all(subprocess.run(["cmp", "-s", os.path.join(d, "split.out"), os.path.join(d, t + ".out")]).returncode == 0
                              for t in ("parent", "plain") if os.path.exists(os.path.join(d, t + ".out")))), flush=True)
        for f in (un, al, un + ".dev", al + ".dev"):          # (some twenty gigabytes)
            if os.path.exists(f):
                os.remove(f)
        return
    noref = len(sys.argv) > 4 and sys.argv[4] == "noref"
    runs = [("ours -p 8", ours, 8), ("ours -p 1", ours, 1)] + ([] if noref else [("reference -p 8", ref, 8)])
    for tag, exe, p in runs:
        t0 = time.time()
        r = subprocess.run([exe, "-f", "-t", "-p", str(p), "--reorder", "-x", os.path.join(d, "idx"), "-U", os.path.join(d, "reads.fa"),
                            "-S", os.path.join(d, tag.split()[0] + ".tsv"), "--report-file", os.path.join(d, tag.split()[0] + ".rep")],
                           capture_output=True, text=True)
        dt = time.time() - t0
        print("%-16s wall %.2fs -> %.3g reads/s  rc=%d | %s" % (tag, dt, n / dt, r.returncode,
              " ; ".join(l for l in r.stderr.splitlines() if "ime" in l or "search" in l or "Stage" in l)))
    if noref:
        return
    same = open(os.path.join(d, "ours.tsv")).read() == open(os.path.join(d, "reference.tsv")).read()
    same_rep = open(os.path.join(d, "ours.rep")).read() == open(os.path.join(d, "reference.rep")).read()
    print("TSV identical: %s, report identical: %s (%d reads)" % (same, same_rep, n))


if __name__ == "__main__":
    main()
