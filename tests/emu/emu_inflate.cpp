// tests/emu/emu_inflate.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The DEFLATE decoder of centrifuge_amd/csrc/cf_inflate.hpp (inflate_body) and the cut rule of a BGZF upload (text_cut_body) on the
// CPU: one call of the body per member with one lane (libcfemu_inflate.so) or, built with CF_EMU_WAVE64 (libcfemu_inflate64.so), a
// wavefront of 64 fibers per member that meet at the fences and cross-lane primitives (cf_platform.hpp), as in emu_cols.cpp.  The
// compressed bytes and the text lie between guard bytes here, which have to stay as they are.
#define CF_HOST_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../../centrifuge_amd/csrc/cf_platform.hpp"
#include "../../centrifuge_amd/csrc/cf_inflate.hpp"

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
            if (w->op[l] != w->op[first]) { std::fprintf(stderr, "emu_inflate: divergent collective (lane %d at op %d, lane %d at op %d)\n", first, w->op[first], l, w->op[l]); std::abort(); }
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

extern "C" {
int emu_inflate_wave_lanes() { return CF_WAVE; }
uint32_t emu_inflate_table_bytes() { return (uint32_t)sizeof(InfTables); }

// members: five words each (InfMember).  out: nOut bytes (what no member writes stays 0x5A); err, blocks: one word per member (why it is corrupt; its deflate blocks).
// returns InfStatus::bad; ~0 - 1: a guard byte was changed, ~0 - 2: a member's range lies outside the buffers
uint64_t emu_inflate(const uint8_t *comp, uint64_t nComp, const uint32_t *members, uint32_t n, uint8_t *out, uint64_t nOut, uint32_t *err, uint32_t *blocks) {
    static_assert(sizeof(InfMember) == 20, "InfMember layout");
    constexpr size_t G = 64;
    const InfMember *mb = reinterpret_cast<const InfMember *>(members);
    for (uint32_t m = 0; m < n; m++)
        if ((uint64_t)mb[m].inOff + mb[m].inLen > nComp || (uint64_t)mb[m].outOff + mb[m].outLen > nOut) return ~0ull - 2;
    std::vector<uint64_t> cbuf((G + nComp + G) / 8 + 2), obuf((G + nOut + G) / 8 + 2);
    uint8_t *c = reinterpret_cast<uint8_t *>(cbuf.data()), *o = reinterpret_cast<uint8_t *>(obuf.data());
    std::memset(c, 0xA5, cbuf.size() * 8); std::memset(o, 0xA5, obuf.size() * 8);
    std::memcpy(c + G, comp, nComp); std::memset(o + G, 0x5A, nOut);
    InfStatus st{};
    DInflate d{c + G, mb, n, o + G, err, &st, blocks};
    auto tables = std::make_unique<InfTables>();
    for (uint32_t m = 0; m < n + 2; m++) {
        std::memset(tables.get(), 0xEE, sizeof(InfTables));              // (nothing is carried from member to member)
#ifdef CF_EMU_WAVE64
        emu_run_wave([&, m] { inflate_body<CF_WAVE>(d, m, (uint32_t)emu_wave_lane(), tables.get()); });
#else
        inflate_body<1>(d, m, 0, tables.get());
#endif
    }
    for (size_t i = 0; i < cbuf.size() * 8; i++) {
        const uint8_t want = i >= G && i < G + nComp ? comp[i - G] : 0xA5;
        if (c[i] != want) return ~0ull - 1;
    }
    for (size_t i = 0; i < obuf.size() * 8; i++) if ((i < G || i >= G + nOut) && o[i] != 0xA5) return ~0ull - 1;
    std::memcpy(out, o + G, nOut);
    return st.bad;
}

// the member table the host makes of a BGZF upload (bgzf_member_table); out: five words per member, or nullptr for the count and
// the total alone.  -> kInfOk or kInfHeader (*nMembers: the member refused); ~0: refused by exception (the 32-bit total)
uint32_t emu_bgzf_member_table(const uint8_t *z, uint64_t nBytes, uint64_t inAt, uint64_t textAt, uint32_t *out, uint64_t *nMembers, uint64_t *total) {
    try { return bgzf_member_table(z, nBytes, inAt, textAt, reinterpret_cast<InfMember *>(out), *nMembers, *total); }
    catch (const std::length_error &) { return ~0u; }
}

// the cut of a BGZF upload's text (text_cut_body) over the markers a plain scan finds; ~0: a marker the body must not have read
uint64_t emu_text_cut(const uint8_t *text, uint64_t n, uint32_t fastq, uint32_t last, uint64_t posCap, uint64_t *nMarkers) {
    std::vector<uint32_t> pos;
    for (uint64_t i = 0; i < n; i++) if (text[i] == (fastq ? '\n' : '>')) pos.push_back((uint32_t)i);
    const uint64_t total = pos.size();
    if (pos.size() > posCap) pos.resize(posCap);
    pos.push_back(0xffffffffu);
    uint64_t cut[2] = {~0ull, ~0ull};
    const DTextCut c{text, n, pos.data(), &total, posCap, fastq, last, cut};
    text_cut_body(c);
    *nMarkers = cut[1];
    return cut[0];
}
}  // extern "C"
