// tests/emu/emu_kreport.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The Kraken-style report's tally on the CPU: lca_body and kreport_body of centrifuge_amd/csrc/cf_kernels.hpp over the table
// lcaTable (cf_kreport_tree.hpp) makes, in both harness widths — one lane per block, or (CF_EMU_WAVE64) a block of 64 fibers that
// meet at the body's block barriers.  The LDS a block leaves behind is read here after each call: what a taxon's count holds
// beyond the LDS tallies went through the far atomics.
#define CF_HOST_EMU 1
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../../centrifuge_amd/csrc/cf_index.hpp"
#include "../../centrifuge_amd/csrc/cf_kernels.hpp"
#include "../../centrifuge_amd/csrc/cf_kreport_tree.hpp"

namespace cfamd { thread_local EmuCtx g_emu; }
using namespace cfamd;

#ifdef CF_EMU_WAVE64
// the wavefront of emu.cpp, as far as these bodies need it: one fiber per lane, and the lanes at a fence (cf_block_sync) go on
// once every lane has reached it or returned
#include <ucontext.h>
namespace {
struct EmuWaveRt {
    static constexpr int N = CF_WAVE;
    static constexpr size_t kStack = 256u << 10;
    ucontext_t sched{}, lane[N]{};
    std::vector<char> stacks;
    bool done[N]{}, waiting[N]{};
    int cur = -1;
    int op[N]{};
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
uint64_t emu_collective(int op, uint64_t, int) {
    EmuWaveRt *w = g_wave;
    const int me = w->cur;
    w->op[me] = op; w->waiting[me] = true;
    swapcontext(&w->lane[me], &w->sched);
    w->cur = me;
    return 0;
}
}  // namespace cfamd
static void emu_run_block(std::function<void()> fn) {
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
        bool live = false;
        for (int l = 0; l < EmuWaveRt::N; l++) {
            if (w->done[l] || w->waiting[l]) continue;
            w->cur = l;
            swapcontext(&w->sched, &w->lane[l]);   // runs until the lane waits at the barrier or returns
            w->cur = -1;
        }
        for (int l = 0; l < EmuWaveRt::N; l++) {
            if (w->done[l]) continue;
            live = true;
            if (w->op[l] != EMU_OP_FENCE) { std::fprintf(stderr, "emu_kreport: a cross-lane primitive other than the block barrier (lane %d, op %d)\n", l, w->op[l]); std::abort(); }
            w->waiting[l] = false; w->op[l] = 0;
        }
        if (!live) break;
    }
    g_wave = nullptr;
}
#else
static void emu_run_block(std::function<void()> fn) { fn(); }
#endif

static kreport::Taxonomy treeOf(uint64_t n, const uint64_t *tid, const uint64_t *parent) {
    kreport::Taxonomy tx;
    tx.quiet = true;
    for (uint64_t i = 0; i < n; i++) {                                     // (Taxonomy::load's loop over explicit nodes)
        const uint64_t par = tid[i] == 1 ? 0 : parent[i];
        tx.at[tid[i]] = (uint32_t)tx.tid.size();
        tx.tid.push_back(tid[i]); tx.parent.push_back(par); tx.rank.push_back(0);
        tx.children[par].push_back(tid[i]);
    }
    return tx;
}

extern "C" {
int emu_kreport_lanes() { return CF_WAVE; }
uint32_t emu_kreport_field_rows() { return kFieldRows; }
uint32_t emu_kreport_slot_bits() { return kCountSlotBits; }
uint32_t emu_kreport_probes() { return kCountProbes; }
uint32_t emu_kreport_chunk() { return kCountChunk; }

// the table of a tree given as n (tid, parent) nodes over the dense taxa `taxa` (sorted, 0 and 1 among them).  0; 1: refused
// (msg: the message, 128 bytes of room)
int emu_kreport_table(uint64_t n, const uint64_t *tid, const uint64_t *parent, const uint64_t *taxa, uint64_t nTaxa, uint64_t *tab, char *msg) {
    try {
        const kreport::Taxonomy tx = treeOf(n, tid, parent);
        const std::vector<uint64_t> t = kreport::lcaTable(tx, std::vector<uint64_t>(taxa, taxa + nTaxa), kLcaOutside);
        std::memcpy(tab, t.data(), nTaxa * 8);
        return 0;
    } catch (const std::exception &e) {
        std::snprintf(msg, 128, "%s", e.what());
        return 1;
    }
}
// ... of an index: its dense taxa into taxa (cap entries of room) and their table; returns the number of taxa, 0 on an error
uint64_t emu_kreport_index(const char *base, uint64_t *taxa, uint64_t *tab, uint64_t cap) {
    try {
        HostIndex h;
        h.load(base, nullptr);
        kreport::Taxonomy tx;
        tx.quiet = true;
        tx.load(h, false);
        const std::vector<uint64_t> t = kreport::lcaTable(tx, h.taxa, kLcaOutside);
        if (h.taxa.size() > cap) return 0;
        std::memcpy(taxa, h.taxa.data(), h.taxa.size() * 8);
        std::memcpy(tab, t.data(), t.size() * 8);
        return h.taxa.size();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "emu_kreport_index: %s\n", e.what());
        return 0;
    }
}
// what the fold makes of two rows' taxa (dense indices)
uint32_t emu_kreport_lca(const uint64_t *tab, uint32_t a, uint32_t b) { return lca_body(tab, lca_inside(tab, a), lca_inside(tab, b)); }

// kreport_body over nq queries: query q prints nOut[q] rows with the taxon indices rows[q * k + j]; rows of a query with up to
// kFieldRows of them are laid out by field (o1b), the others in the k slots of `out`, each as the score kernels leave them — and
// the other place holds a taxon index no table has.  window [qLo, qHi); chunk queries per block; counts: nTaxa + 1 (added to);
// ldsPer: nTaxa, what went through the LDS tallies (added to).  returns the number of blocks run
uint32_t emu_kreport(const uint64_t *tab, uint32_t nTaxa, uint32_t nq, const uint32_t *nOut, const uint32_t *rows, uint32_t k, uint32_t qLo, uint32_t qHi,
                     uint32_t chunk, uint32_t slotBits, uint64_t *counts, uint64_t *ldsPer) {
    const uint64_t stride = (uint64_t)nq + 3;
    std::vector<uint64_t> o1b(stride * kFieldRows, ~0ull);
    std::vector<OutRow> out((uint64_t)nq * k + 1);
    for (auto &o : out) { o = OutRow{}; o.tidx = 0xfffffff0u; }
    for (uint32_t q = 0; q < nq; q++)
        for (uint32_t j = 0; j < nOut[q] && j < k; j++) {
            if (nOut[q] <= kFieldRows) o1b[j * stride + q] = ((uint64_t)rows[(uint64_t)q * k + j] << 32) | 77u;
            else out[(uint64_t)q * k + j].tidx = rows[(uint64_t)q * k + j];
        }
    std::vector<uint32_t> no(nOut, nOut + nq);
    BatchStatus st{};
    st.qLo = qLo; st.qHi = qHi;
    DBatch b{};
    b.o1b = o1b.data(); b.oStride = stride; b.out = out.data(); b.nOut = no.data(); b.nTaxa = nTaxa; b.nQueries = nq; b.st = &st;
    std::vector<unsigned long long> cnt(nTaxa + 1, 0);
    const DKreport kr{tab, cnt.data(), k, chunk};
    const uint32_t nSlots = 1u << slotBits;
    const bool direct = nTaxa <= nSlots;
    uint32_t blocks = 0;
    for (uint32_t c = 0; (uint64_t)c * chunk < (uint64_t)nq + 1; c++, blocks++) {
        std::vector<uint32_t> lds(2 * nSlots + 1 + 8, 0xababababu);
        emu_run_block([&] { kreport_body(b, kr, lds.data(), c, slotBits, direct); });
        for (uint32_t s = 0; s < nSlots; s++) if (lds[s] != kCountEmpty && lds[s] < nTaxa) ldsPer[lds[s]] += lds[nSlots + s];
        for (uint32_t s = 2 * nSlots + 1; s < lds.size(); s++) if (lds[s] != 0xababababu) return ~0u;      // (written behind its LDS)
    }
    for (uint32_t i = 0; i <= nTaxa; i++) counts[i] += cnt[i];
    return blocks;
}
}  // extern "C"
