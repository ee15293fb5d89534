// tests/emu/emu_matecut.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The common cut of the two texts of a BGZF pair upload (text_cut_pair_body, centrifuge_amd/csrc/cf_inflate.hpp) on the CPU, as
// k_text_cut_pair launches it: the threads of the launch in a plain loop, thread 0 doing the work — one thread per "wavefront"
// (libcfemu_matecut.so) or, built with CF_EMU_WAVE64 (libcfemu_matecut64.so), 64.  The markers are those a plain scan finds; of a
// block with more markers than posCap only the first posCap are kept, followed by a place the body must not read.
#define CF_HOST_EMU 1
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../centrifuge_amd/csrc/cf_platform.hpp"
#include "../../centrifuge_amd/csrc/cf_inflate.hpp"

namespace cfamd { thread_local EmuCtx g_emu; }
using namespace cfamd;

#ifdef CF_EMU_WAVE64
// (the body uses no cross-lane primitive: there is no wavefront of fibers here, the primitives are the one-lane ones)
namespace cfamd {
int emu_wave_lane() { return -1; }
uint64_t emu_collective(int, uint64_t, int) { std::fprintf(stderr, "emu_matecut: a cross-lane primitive outside a wavefront\n"); std::abort(); }
}  // namespace cfamd
#endif

extern "C" {
int emu_matecut_wave_lanes() { return CF_WAVE; }
uint32_t emu_matecut_bad_start() { return kCutBadStart; }

// out: cut 0, markers in front of it, cut 1, markers in front of it; returns the flags the body set
uint32_t emu_text_cut_pair(const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, uint32_t fastq, uint32_t last0, uint32_t last1,
                           uint64_t posCap0, uint64_t posCap1, uint64_t *out) {
    const uint8_t *text[2] = {text0, text1};
    const uint64_t nB[2] = {n0, n1}, cap[2] = {posCap0, posCap1};
    const uint32_t last[2] = {last0, last1};
    std::vector<uint32_t> pos[2];
    uint64_t total[2];
    uint32_t flags = 0;
    DTextCutPair c{};
    for (int i = 0; i < 2; i++) {
        for (uint64_t b = 0; b < nB[i]; b++) if (text[i][b] == (fastq ? '\n' : '>')) pos[i].push_back((uint32_t)b);
        total[i] = pos[i].size();
        if (pos[i].size() > cap[i]) pos[i].resize(cap[i]);
        pos[i].push_back(0xffffffffu);
        out[2 * i] = out[2 * i + 1] = ~0ull;
        c.blk[i] = DTextCut{text[i], nB[i], pos[i].data(), &total[i], cap[i], fastq, last[i], out + 2 * i};
    }
    c.flags = &flags;
    g_emu.nthreads = CF_WAVE;
    for (uint32_t t = 0; t < (uint32_t)CF_WAVE; t++) { g_emu.tid = t; if (cf_global_thread() == 0) text_cut_pair_body(c); }
    g_emu.tid = 0; g_emu.nthreads = 1;
    return flags;
}
}  // extern "C"
