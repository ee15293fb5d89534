// tests/emu/emu_deflate.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The DEFLATE encoder of centrifuge_amd/csrc/cf_deflate.hpp (deflate_body, def_compact_body) on the CPU: a wavefront of 64 fibers per
// member that meet at the cross-lane primitives (cf_platform.hpp), as in emu_inflate.cpp — the body has no one-lane form, so this is
// built with CF_EMU_WAVE64 only.  The text and the members lie between guard bytes here, which have to stay as they are; so does
// what lies behind a member's bytes in its room at the stride.
#define CF_HOST_EMU 1
#define CF_EMU_WAVE64 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../../centrifuge_amd/csrc/cf_platform.hpp"
#include "../../centrifuge_amd/csrc/cf_deflate.hpp"

namespace cfamd { thread_local EmuCtx g_emu; }
using namespace cfamd;

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
            if (w->op[l] != w->op[first]) { std::fprintf(stderr, "emu_deflate: divergent collective (lane %d at op %d, lane %d at op %d)\n", first, w->op[first], l, w->op[l]); std::abort(); }
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

extern "C" {
uint32_t emu_deflate_stride(uint32_t member) { return def_stride(member); }
uint32_t emu_deflate_table_bytes() { return kDefTableWords * 2; }
uint32_t emu_deflate_window() { return kDefWindow; }

// text: n bytes; member: text bytes per member; out: room for ceil(n / member) * emu_deflate_stride(member) bytes, the members come
// back together there, *outBytes of them; size: one word per member.  returns 0; ~0 - 1: a guard byte was changed, ~0 - 2: a bad member size
uint64_t emu_deflate(const uint8_t *text, uint64_t n, uint32_t member, uint8_t *out, uint64_t *outBytes, uint32_t *size) {
    constexpr size_t G = 64;
    if (!def_member_ok(member)) return ~0ull - 2;
    const uint32_t nMembers = (uint32_t)((n + member - 1) / member), stride = def_stride(member);
    const uint64_t nOut = (uint64_t)nMembers * stride;
    std::vector<uint64_t> tbuf((G + n + G) / 8 + 2), obuf((G + nOut + G) / 8 + 2), cbuf((G + nOut + G) / 8 + 2);
    uint8_t *t = reinterpret_cast<uint8_t *>(tbuf.data()), *o = reinterpret_cast<uint8_t *>(obuf.data()), *c = reinterpret_cast<uint8_t *>(cbuf.data());
    std::memset(t, 0xA5, tbuf.size() * 8); std::memset(o, 0xA5, obuf.size() * 8); std::memset(c, 0xA5, cbuf.size() * 8);
    std::memcpy(t + G, text, n);
    std::vector<uint32_t> sz(nMembers + 1, 0xA5A5A5A5u);
    const DDeflate d{t + G, n, member, nMembers, o + G, sz.data()};
    std::vector<uint16_t> tab(kDefTableWords);
    for (uint32_t m = 0; m < nMembers + 2; m++) {
        std::memset(tab.data(), 0xEE, tab.size() * 2);                       // (nothing is carried from member to member)
        emu_run_wave([&, m] { deflate_body(d, m, (uint32_t)emu_wave_lane(), tab.data()); });
    }
    if (sz[nMembers] != 0xA5A5A5A5u) return ~0ull - 1;
    for (size_t i = 0; i < tbuf.size() * 8; i++) if (t[i] != (i >= G && i < G + n ? text[i - G] : 0xA5)) return ~0ull - 1;
    std::vector<uint64_t> off(nMembers + 1, 0);
    for (uint32_t m = 0; m < nMembers; m++) {
        if (sz[m] > stride) return ~0ull - 1;
        off[m + 1] = off[m] + sz[m];
    }
    for (size_t i = 0; i < obuf.size() * 8; i++) {
        const bool inside = i >= G && i < G + nOut && (i - G) % stride < sz[(i - G) / stride];
        if (!inside && o[i] != 0xA5) return ~0ull - 1;
    }
    const DDefCompact dc{o + G, stride, nMembers, sz.data(), off.data(), c + G};
    for (uint32_t m = 0; m < nMembers + 2; m++)
        emu_run_wave([&, m] { def_compact_body(dc, m, (uint32_t)emu_wave_lane(), CF_WAVE); });
    for (size_t i = 0; i < cbuf.size() * 8; i++) if ((i < G || i >= G + off[nMembers]) && c[i] != 0xA5) return ~0ull - 1;
    std::memcpy(out, c + G, off[nMembers]);
    std::memcpy(size, sz.data(), nMembers * 4);
    *outBytes = off[nMembers];
    return 0;
}
}  // extern "C"
