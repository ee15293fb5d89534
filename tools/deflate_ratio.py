#!/usr/bin/env python3
"""What the device deflater (centrifuge_amd/csrc/cf_deflate.hpp) makes of a text, in the CPU harness of tests/emu/emu_deflate.cpp (no
GPU needed): compressed size / text for the library's hash table and window and for other choices of the two — each a harness
built with CF_DEF_HASH_BITS / CF_DEF_WINDOW of its own —, beside zlib's raw deflate at levels 1 and 6 on the same 65,280-byte pieces
in the same container.  The table of DESIGN.md §5 is this script's output.
usage: tools/deflate_ratio.py [file ...]        (default: synth_small's golden k5.tsv and fastq.tsv)"""
import gzip
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import common  # noqa: E402
import emu_deflate as D  # noqa: E402

VARIANTS = [(None, None), (7, 1024), (9, 1024), (10, 1024), (8, 512), (8, 2048), (10, 4096), (8, 0)]


def zlib_members(text, level):
    n = 0
    for i in range(0, len(text), D.MEMBER):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        n += len(co.compress(text[i:i + D.MEMBER]) + co.flush()) + 26
    return n


def main():
    files = sys.argv[1:]
    if not files:
        d, _ = common.golden("synth_small")
        files = [os.path.join(d, "k5.tsv"), os.path.join(d, "fastq.tsv")]
    for f in files:
        text = open(f, "rb").read()
        print("%s: %d bytes" % (os.path.basename(f), len(text)))
        for bits, window in VARIANTS:
            L = D.load(D.build(bits, window))
            z, _ = D.deflate(text, L=L)
            assert gzip.decompress(z + D.EOF_MEMBER) == text
            print("  %5d places per lane (%3d KiB per wavefront), window %4d: %8d bytes  ratio %.3f%s" % (
                L.emu_deflate_table_bytes() // 128, L.emu_deflate_table_bytes() >> 10, L.emu_deflate_window(), len(z), len(z) / len(text),
                "   <- the library's" if bits is None else ""))
        for level in (1, 6):
            n = zlib_members(text, level)
            print("  zlib level %d: %8d bytes  ratio %.3f" % (level, n, n / len(text)))


if __name__ == "__main__":
    main()
