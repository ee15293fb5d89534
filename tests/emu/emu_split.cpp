// tests/emu/emu_split.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The read splitter of centrifuge_amd/csrc/cf_textio.hpp (split_size_body / split_write_body) on the CPU, over synthetic inputs: the
// launches of cf_batch_wait_text_split — size pass, exclusive sums per sink, write pass — one body call per thread.  Built with
// CF_EMU_WAVE64 as well (libcfemu_split64.so) both passes run as wavefronts of 64 fibers that meet at the cross-lane primitives
// (cf_platform.hpp), as in emu_cols.cpp; this library includes nothing but the two headers.
#define CF_HOST_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../../centrifuge_amd/csrc/cf_platform.hpp"
#include "../../centrifuge_amd/csrc/cf_textio.hpp"

namespace cfamd { thread_local EmuCtx g_emu; }
using namespace cfamd;

#ifdef CF_EMU_WAVE64
// the 64-lane wavefront of emu.cpp: one fiber per lane, a scheduler that runs every lane up to its next cross-lane primitive (or
// its return) and then forms that primitive's results over the lanes still alive
#include <ucontext.h>
namespace {
struct EmuWaveRt {
    static constexpr int N = CF_WAVE;
    static constexpr size_t kStack = 256u << 10;
    ucontext_t sched{}, lane[N]{};
    std::vector<char> stacks;
    bool done[N]{}, waiting[N]{};
    int cur = -1;
    int op[N]{}, src[N]{};
    uint64_t in[N]{}, out[N]{};
    std::function<void()> fn;
};
thread_local EmuWaveRt *g_wave = nullptr;
void emuLaneMain() {
    EmuWaveRt *w = g_wave;
    const int me = w->cur;
    w->fn();
    w->done[me] = true;
    swapcontext(&w->lane[me], &w->sched);         // never resumed
}
}  // namespace
namespace cfamd {
int emu_wave_lane() { return g_wave ? g_wave->cur : -1; }
uint64_t emu_collective(int op, uint64_t v, int src) {
    EmuWaveRt *w = g_wave;
    const int me = w->cur;
    w->op[me] = op; w->in[me] = v; w->src[me] = src; w->waiting[me] = true;
    swapcontext(&w->lane[me], &w->sched);
    w->cur = me;
    return w->out[me];
}
}  // namespace cfamd
static void emu_run_wave(std::function<void()> fn) {
    auto w = std::make_unique<EmuWaveRt>();
    w->fn = std::move(fn);
    w->stacks.assign(EmuWaveRt::kStack * EmuWaveRt::N, 0);
    for (int l = 0; l < EmuWaveRt::N; l++) {
        getcontext(&w->lane[l]);
        w->lane[l].uc_stack.ss_sp = w->stacks.data() + EmuWaveRt::kStack * (size_t)l;
        w->lane[l].uc_stack.ss_size = EmuWaveRt::kStack;
        w->lane[l].uc_link = nullptr;
        makecontext(&w->lane[l], emuLaneMain, 0);
    }
    g_wave = w.get();
    for (;;) {
        for (int l = 0; l < EmuWaveRt::N; l++) {
            if (w->done[l] || w->waiting[l]) continue;
            w->cur = l;
            swapcontext(&w->sched, &w->lane[l]);   // runs until the lane waits at a primitive or returns
            w->cur = -1;
        }
        // the lanes at a fence first: every lane has reached a fence, a primitive or its end — the lockstep the fence stands for
        bool released = false;
        for (int l = 0; l < EmuWaveRt::N; l++)
            if (!w->done[l] && w->waiting[l] && w->op[l] == EMU_OP_FENCE) { w->waiting[l] = false; w->op[l] = 0; released = true; }
        if (released) continue;
        int first = -1;
        for (int l = 0; l < EmuWaveRt::N; l++) if (!w->done[l]) { first = l; break; }
        if (first < 0) break;                      // every lane has returned
        uint64_t mask = 0;
        for (int l = 0; l < EmuWaveRt::N; l++) {
            if (w->done[l]) continue;
            if (w->op[l] != w->op[first]) { std::fprintf(stderr, "emu_split: divergent collective (lane %d at op %d, lane %d at op %d)\n", first, w->op[first], l, w->op[l]); std::abort(); }
            if (w->in[l] & 1ull) mask |= 1ull << l;
        }
        for (int l = 0; l < EmuWaveRt::N; l++) {
            if (w->done[l]) continue;
            switch (w->op[l]) {
                case EMU_OP_BALLOT: w->out[l] = mask; break;
                case EMU_OP_FIRST: w->out[l] = w->in[first]; break;
                default: { const int s = w->src[l] & (EmuWaveRt::N - 1); w->out[l] = w->done[s] ? w->in[l] : w->in[s]; break; }
            }
            w->waiting[l] = false;
        }
    }
    g_wave = nullptr;
}
#endif

template <typename F>
static void emuThreads(uint64_t n, F body) {
#ifdef CF_EMU_WAVE64
    for (uint64_t base = 0; base < n; base += CF_WAVE) emu_run_wave([&, base] { body((uint32_t)(base + (uint64_t)emu_wave_lane())); });
#else
    for (uint64_t t = 0; t < n; t++) body((uint32_t)t);
#endif
}

extern "C" {
int emu_split_wave_lanes() { return CF_WAVE; }

// everything the two passes read (tests/emu/emu_split.py mirrors the layout)
struct EmuSplitIn {
    const uint8_t *text;                  // the block, followed by >= 128 zero bytes
    const uint32_t *idOff, *idLen, *rlen; // per read
    const uint32_t *qualOff;              // per read, or null (FASTA)
    const uint64_t *bases;                // the reads' packed words one behind the other (ceil(len / 32) each)
    const uint32_t *nmask;
    const uint8_t *qinfo;
    uint32_t nQueries, paired, sinks, pad;
    uint8_t *out[4];                      // room for outCap[s] bytes each
    uint64_t outCap[4];
    uint64_t bytes[4], records[4];        // results
    uint32_t sized[4];                    // results: the sink had a size array (it was on)
};
// 0, or 1: a byte outside a sink's room was written
int emu_split_run(EmuSplitIn *in) {
    const uint32_t nq = in->nQueries, nReads = in->paired ? 2 * nq : nq;
    std::vector<uint64_t> woff(nReads + 1, 0);
    for (uint32_t r = 0; r < nReads; r++) woff[r + 1] = woff[r] + ((in->rlen[r] + 31) >> 5);
    DTextSplit d{};
    d.text = in->text; d.idOff = in->idOff; d.idLen = in->idLen; d.rlen = in->rlen; d.qinfo = in->qinfo;
    d.woff = woff.data(); d.bases = in->bases; d.nmask = in->nmask; d.qualOff = in->qualOff;
    d.nQueries = nq; d.paired = in->paired ? 1u : 0u; d.sinks = in->sinks;
    unsigned long long nRec[kSplitSinks] = {};
    d.nRec = nRec;
    std::vector<uint32_t> size[kSplitSinks];
    std::vector<uint64_t> off[kSplitSinks];
    for (uint32_t s = 0; s < kSplitSinks; s++) {
        in->sized[s] = split_sink_on(d, s) ? 1u : 0u;
        if (!in->sized[s]) continue;
        size[s].assign(nq + 1, 0xdeadbeefu); off[s].assign(nq + 1, 0);
        d.size[s] = size[s].data(); d.off[s] = off[s].data();
    }
    emuThreads((uint64_t)nq + 5, [&](uint32_t q) { split_size_body(d, q); });     // (its sums over the wavefront need the wavefront)
    // (every sink starts on a dword boundary, as device memory does; around the room it has: marked bytes that must stay as they are)
    const size_t guard = 256;
    std::vector<uint32_t> buf[kSplitSinks];
    for (uint32_t s = 0; s < kSplitSinks; s++) {
        in->bytes[s] = 0; in->records[s] = nRec[s];
        if (!in->sized[s]) continue;
        for (uint32_t q = 0; q < nq; q++) off[s][q + 1] = off[s][q] + size[s][q];
        in->bytes[s] = off[s][nq];
        const uint64_t cap = in->bytes[s] < in->outCap[s] ? in->bytes[s] : in->outCap[s];
        buf[s].assign((size_t)(cap / 4 + 2) + 2 * guard / 4, 0xA5A5A5A5u);
        d.out[s] = reinterpret_cast<uint8_t *>(buf[s].data()) + guard; d.cap[s] = cap;
        std::memset(d.out[s], 0x5A, (size_t)cap);                      // (a byte of the room that nothing wrote)
    }
    emuThreads((uint64_t)nq + 70, [&](uint32_t q) { split_write_body(d, q); });
    int bad = 0;
    for (uint32_t s = 0; s < kSplitSinks; s++) {
        if (!in->sized[s]) continue;
        const uint8_t *b = reinterpret_cast<const uint8_t *>(buf[s].data());
        for (size_t i = 0; i < buf[s].size() * 4; i++) if ((i < guard || i >= guard + d.cap[s]) && b[i] != 0xA5) bad = 1;
        std::memcpy(in->out[s], d.out[s], (size_t)d.cap[s]);
    }
    return bad;
}
}  // extern "C"
