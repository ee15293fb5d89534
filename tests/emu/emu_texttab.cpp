// tests/emu/emu_texttab.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The passes of cf_batch_upload_text over a TABBED block (CF_TEXT_TAB5 / CF_TEXT_TAB6; centrifuge_amd/csrc/cf_textio.hpp: text_count_body,
// text_mark_body, text_record_body with its tabbed branch, text_tab_kind, text_pack_body) on the CPU, one body call per thread, as
// emu_texttrim.cpp runs them for FASTA / FASTQ.  Built with CF_EMU_WAVE64 as well (libcfemu_texttab64.so) the record pass runs as
// wavefronts of 64 fibers that meet at its cross-lane sums; this library includes nothing but the two headers.
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
            if (w->op[l] != w->op[first]) { std::fprintf(stderr, "emu_texttab: divergent collective (lane %d at op %d, lane %d at op %d)\n", first, w->op[first], l, w->op[l]); std::abort(); }
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
int emu_tab_wave_lanes() { return CF_WAVE; }

// one block of a batch (tests/emu/emu_texttab.py mirrors the layout).  text: the block's first byte, followed by >= kTextPad zero
// bytes, textBase bytes into the 8-byte aligned buffer the pack pass sees; its record r >= skip is read stride * (r - skip) + mate.
struct EmuTabIn {
    const uint8_t *text;
    uint64_t nBytes, posCap;
    uint32_t format, globalSeed, recCap, textBase, stride, mate, trim5, trim3, skip, pad;
    uint32_t *rlen, *seeds, *seqOff, *idOff, *idLen, *qualOff;      // per read of the batch (qualOff: null = not kept)
    uint64_t *status;                                                // nWords, nBases (added to), maxLen (max), flags (or), 1 = the lines are pairs
};
// returns the block's records (0 with flags set: the block is not in the plain form)
uint32_t emu_tab_parse(const EmuTabIn *in) {
    const uint64_t nPieces = (in->nBytes + kTextPiece - 1) / kTextPiece;
    std::vector<uint32_t> cnt(nPieces + 1, 0), pos(in->posCap + 1, 0);
    std::vector<uint64_t> base(nPieces + 1, 0);
    const DTextMark m{in->text, in->nBytes, in->format == kTextFasta ? (uint32_t)'>' : (uint32_t)'\n', cnt.data(), base.data(), pos.data(), in->posCap};
    for (uint64_t t = 0; t < nPieces + 3; t++) text_count_body(m, t);
    for (uint64_t t = 0; t < nPieces; t++) base[t + 1] = base[t] + cnt[t];
    for (uint64_t t = 0; t < nPieces + 3; t++) text_mark_body(m, t);
    TextStatus st{};
    const uint32_t seed0 = (in->globalSeed + 101u) * 59u * 61u * 67u * 71u * 73u * 79u * 83u;
    const DTextRec d{in->text, in->nBytes, pos.data(), &base[nPieces], in->posCap, in->recCap, in->format, seed0, in->rlen, in->seeds, in->seqOff,
                     in->idOff, in->idLen, &st, in->textBase, in->stride, in->mate, in->qualOff, in->trim5, in->trim3, in->skip};
    emuThreads((uint64_t)in->recCap + 70, [&](uint32_t r) { text_record_body(d, r); });
    uint32_t flags = st.flags;
    const bool pairs = text_tab_kind(flags);                           // (what uploadTextBlocks does with the status)
    in->status[0] += st.words(); in->status[1] += st.bases(); in->status[2] = st.maxLen > in->status[2] ? st.maxLen : in->status[2]; in->status[3] |= flags;
    in->status[4] = pairs ? 1 : 0;
    if (flags) return 0;
    return (uint32_t)base[nPieces];
}
// the packed words and N masks of nReads reads (ceil(len / 32) words each, one read behind the other)
void emu_tab_pack(const uint8_t *text, uint32_t nReads, const uint32_t *seqOff, const uint32_t *rlen, uint64_t *bases, uint32_t *nmask) {
    std::vector<uint64_t> woff(nReads + 1, 0);
    for (uint32_t r = 0; r < nReads; r++) woff[r + 1] = woff[r] + ((rlen[r] + 31) >> 5);
    const DTextPack d{text, seqOff, rlen, woff.data(), bases, nmask, nReads};
    for (uint32_t r = 0; r < nReads + 5; r++) text_pack_body(d, r);
}
}  // extern "C"
