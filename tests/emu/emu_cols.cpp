// tests/emu/emu_cols.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The column-program formatter of centrifuge_amd/csrc/cf_textio.hpp (fmt_cols_size_body / fmt_cols_write_body) on the CPU, over
// synthetic inputs: the launches of cf_batch_wait_text — size pass, exclusive sums, write pass — one body call per thread.  Built
// with CF_EMU_WAVE64 as well (libcfemu_cols64.so) the write pass runs as wavefronts of 64 fibers that meet at the cross-lane
// primitives (cf_platform.hpp), as in emu.cpp; this library includes nothing but the two headers.
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
            if (w->op[l] != w->op[first]) { std::fprintf(stderr, "emu_cols: divergent collective (lane %d at op %d, lane %d at op %d)\n", first, w->op[first], l, w->op[l]); std::abort(); }
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
int emu_cols_wave_lanes() { return CF_WAVE; }
uint32_t emu_cols_lds_bytes() { return kFmtLds; }

// everything the two passes read (tests/emu/emu_cols.py mirrors the layout)
struct EmuColsIn {
    const uint8_t *text;                  // the block, followed by >= 128 zero bytes
    const uint32_t *idOff, *idLen, *rlen; // per read
    const uint32_t *qualOff;              // per read, or null (FASTA)
    const uint64_t *bases;                // the reads' packed words one behind the other (ceil(len / 32) each)
    const uint32_t *nmask;
    const uint8_t *rows;                  // 16-byte rows: uniqueID, taxon index, score, hitLen
    const uint8_t *qinfo;
    const uint32_t *score2, *maxScore;
    uint32_t nQueries, paired;
    const uint8_t *strs;
    const uint32_t *uidOff, *rankOff, *taxOff;
    const uint8_t *taxLeaf;
    uint32_t nRefs, nTaxa, idxZero, nCols;
    const uint8_t *taxStrs;
    const uint32_t *trankOff, *tnameOff;
    const uint8_t *cols;                  // the program (nCols codes); with defaultBodies the DEFAULT bodies run instead (fmt_size_body / fmt_write_body)
    uint32_t defaultBodies, tuplesCap;
    uint8_t *out;
    uint64_t outCap;
    unsigned long long *single;           // per taxon: added to
    uint32_t *tuples;
    uint32_t *tupleWords;
    uint32_t *size;                       // per query: what the size pass left
};
// returns the bytes of text (out holds outCap of them; rows that do not fit are left out, as on the device, and a byte of the room
// that nothing wrote is 0x5A); ~0: too many columns, ~0 - 1: a byte behind the room was written
uint64_t emu_cols_format(const EmuColsIn *in) {
    const uint32_t nq = in->nQueries, nReads = in->paired ? 2 * nq : nq;
    std::vector<uint64_t> rowFirst(nq + 1, 0), outOff(nq + 1, 0), woff(nReads + 1, 0);
    for (uint32_t q = 0; q < nq; q++) rowFirst[q + 1] = rowFirst[q] + (in->qinfo[q] & 0x3fu);
    for (uint32_t r = 0; r < nReads; r++) woff[r + 1] = woff[r] + ((in->rlen[r] + 31) >> 5);
    // (the output starts on a dword boundary, as device memory does; behind the room it has: marked bytes that must stay as they are)
    const size_t outWords = (size_t)(in->outCap / 4 + 2), guardWords = 64;
    std::vector<uint32_t> size(nq + 1, 0), outBuf(outWords + guardWords, 0);
    std::memset(outBuf.data(), 0x5A, (size_t)in->outCap);
    std::memset(reinterpret_cast<uint8_t *>(outBuf.data()) + in->outCap, 0xA5, outBuf.size() * 4 - (size_t)in->outCap);
    TextStatus st{};
    DTextFmt f{};
    f.text = in->text; f.idOff = in->idOff; f.idLen = in->idLen; f.rlen = in->rlen;
    f.rows = reinterpret_cast<const TextRow *>(in->rows); f.rowFirst = rowFirst.data(); f.qinfo = in->qinfo; f.score2 = in->score2; f.maxScore = in->maxScore;
    f.nQueries = nq; f.paired = in->paired ? 1u : 0u;
    f.strs = in->strs; f.uidOff = in->uidOff; f.rankOff = in->rankOff; f.taxOff = in->taxOff; f.taxLeaf = in->taxLeaf;
    f.nRefs = in->nRefs; f.nTaxa = in->nTaxa; f.idxZero = in->idxZero;
    f.size = size.data(); f.outOff = outOff.data(); f.out = reinterpret_cast<uint8_t *>(outBuf.data()); f.outCap = in->outCap;
    f.single = in->single; f.tuples = in->tuples; f.tuplesCap = in->tuplesCap; f.st = &st;
    TextCols pc{};
    if (!in->defaultBodies) {
        f.taxStrs = in->taxStrs; f.trankOff = in->trankOff; f.tnameOff = in->tnameOff;
        f.woff = woff.data(); f.bases = in->bases; f.nmask = in->nmask; f.qualOff = in->qualOff;
        if (in->nCols > kTextMaxCols) return ~0ull;
        for (uint32_t i = 0; i < in->nCols; i++) pc.col[i] = in->cols[i];
        pc.nCols = in->nCols;
    }
    for (uint32_t q = 0; q < nq + 5; q++) { if (in->defaultBodies) fmt_size_body(f, q); else fmt_cols_size_body(f, pc, q); }
    for (uint32_t q = 0; q < nq; q++) outOff[q + 1] = outOff[q] + size[q];
    // a wavefront's LDS: one buffer per wavefront of the 64-lane build, per thread in the one-lane build
    const uint64_t ldsWords = (kFmtLds + 16) / 8 + 1;
    std::vector<uint64_t> ldsAll(((uint64_t)nq + 70 + CF_WAVE) / CF_WAVE * ldsWords);
    emuThreads((uint64_t)nq + 70, [&](uint32_t q) {
        uint8_t *lds = reinterpret_cast<uint8_t *>(ldsAll.data() + (uint64_t)(q / CF_WAVE) * ldsWords);
        if (in->defaultBodies) fmt_write_body(f, q, lds); else fmt_cols_write_body(f, pc, q, lds);
    });
    *in->tupleWords = st.tupleWords;
    const uint64_t total = nq ? st.outBytes : 0;
    for (size_t i = (size_t)in->outCap; i < outBuf.size() * 4; i++) if (reinterpret_cast<const uint8_t *>(outBuf.data())[i] != 0xA5) return ~0ull - 1;
    std::memcpy(in->out, outBuf.data(), (size_t)in->outCap);
    for (uint32_t q = 0; q < nq; q++) in->size[q] = size[q];
    return total;
}
}  // extern "C"
