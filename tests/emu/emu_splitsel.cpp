// tests/emu/emu_splitsel.cpp — TEST HARNESS ONLY (never linked into libcentrifuge_amd.so).
//
// The read splitter's size pass by a selection of taxa (split_sel_size_body, centrifuge_amd/csrc/cf_textio.hpp) on the CPU, with the
// write pass it leaves as it is (split_write_body): the launches of cf_batch_wait_text_split with a selection in force — size pass,
// exclusive sums per sink, write pass — one body call per thread.  The one-lane build and the wavefronts of 64 fibers are those of
// emu_split.cpp, which this file includes for its fibers, its emuThreads and its EmuSplitIn (libcfemu_splitsel.so,
// libcfemu_splitsel64.so with CF_EMU_WAVE64).
#include "emu_split.cpp"

extern "C" {
// in: as emu_split_run takes it; rows: 16 bytes per printed row (uniqueID, dense taxon, score, hitLength), a query's rows behind
// those of the queries before it; mask: nTaxa + 1 bytes.  0, or 1: a byte outside a sink's room was written
int emu_splitsel_run(EmuSplitIn *in, const uint32_t *rows, const uint8_t *mask, uint32_t nTaxa) {
    const uint32_t nq = in->nQueries, nReads = in->paired ? 2 * nq : nq;
    std::vector<uint64_t> woff(nReads + 1, 0), rowFirst(nq + 1, 0);
    for (uint32_t r = 0; r < nReads; r++) woff[r + 1] = woff[r] + ((in->rlen[r] + 31) >> 5);
    for (uint32_t q = 0; q < nq; q++) rowFirst[q + 1] = rowFirst[q] + (in->qinfo[q] & 0x3fu);
    DTextSplit d{};
    d.text = in->text; d.idOff = in->idOff; d.idLen = in->idLen; d.rlen = in->rlen; d.qinfo = in->qinfo;
    d.woff = woff.data(); d.bases = in->bases; d.nmask = in->nmask; d.qualOff = in->qualOff;
    d.nQueries = nq; d.paired = in->paired ? 1u : 0u; d.sinks = in->sinks;
    const DTextSplitSel e{reinterpret_cast<const TextRow *>(rows), rowFirst.data(), mask, nTaxa};
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
    emuThreads((uint64_t)nq + 5, [&](uint32_t q) { split_sel_size_body(d, e, q); });     // (whole wavefronts: the lanes past the end take part)
    for (uint32_t s = 0; s < kSplitSinks; s++) if (in->sized[s] && size[s][nq] != 0xdeadbeefu) return 1;      // (a size behind the last query's)
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
        std::memset(d.out[s], 0x5A, (size_t)cap);
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
