// cf_inflate.hpp — BGZF members inflated ON THE DEVICE: a raw-DEFLATE (RFC 1951) decoder as a kernel body.
//
// A BGZF file (bgzip, htslib) is a gzip file whose members are independent, hold at most 64 KiB of text and carry their own
// compressed size; the host hops their headers and makes one InfMember per member — where its deflate payload lies in the uploaded
// bytes, where its text goes (the sums of the ISIZE trailers) and the CRC32 its trailer names.  ONE WAVEFRONT INFLATES ONE MEMBER:
//   * the bit reader's state is the same in every lane (the symbol loop is wave-uniform: no lane ever waits for another);
//   * the tables of a block — code lengths, the canonical code's counts and sorted symbols, a first-level lookup of 10 (lengths /
//     literals) and 8 (distances) bits — lie in the wavefront's LDS (InfTables, under 4 KiB); the serial steps of their making are
//     lane 0's, the filling of the lookups is spread over the lanes;
//   * a literal is stored by one lane; a match of length L is copied by L lanes at once, lane i from  pos - dist + (i mod dist);
//   * the member's CRC32 (the host reader checks it, so this does): every lane folds its share of the text, lane 0 puts the
//     shares together (crc(A|B) = crc(A) * x^(8|B|) + crc(B) in GF(2)[x] mod the CRC's polynomial).
// The same body with W = 1 is the one-lane-per-member form (tables wherever the caller puts them) and what the CPU harness steps
// through (tests/emu/emu_inflate.cpp; with CF_EMU_WAVE64 the 64-lane form as fibers).
//
// A malformed stream ends in a status, never in an access out of range: a bit beyond the member's payload is never used (the reader
// fetches aligned 8-byte words, so the uploaded bytes start on an 8-byte boundary and are followed by kInfPad bytes that are read
// but not used), a byte is written only below the member's ISIZE, a distance reaches back only over bytes this member has produced.
#pragma once
#include <cstring>
#include <stdexcept>

#include "cf_platform.hpp"

namespace cfamd {

constexpr uint32_t kInfPad = 16;                        // bytes behind the compressed bytes (and behind the text) that may be fetched
constexpr uint32_t kInfMaxOut = 65536;                  // a BGZF member's text
constexpr uint32_t kInfLitBits = 10, kInfDistBits = 8;  // the first-level lookups
// why a member is corrupt (InfStatus / the per-member word; 0 = it is not)
enum : uint32_t {
    kInfOk = 0, kInfBadBlockType = 1, kInfStoredLen = 2, kInfTooManyCodes = 3, kInfOverSubscribed = 4, kInfIncomplete = 5, kInfBadRepeat = 6,
    kInfNoEndCode = 7, kInfBadCode = 8, kInfBadLenSym = 9, kInfBadDistSym = 10, kInfDistTooFar = 11, kInfOutOverrun = 12, kInfInOverrun = 13,
    kInfOutShort = 14, kInfCrc = 15, kInfHeader = 16     // (kInfHeader is the host's: a member whose gzip header or size is not BGZF's)
};
struct InfMember { uint32_t inOff, inLen, outOff, outLen, crc; };
struct InfStatus { uint32_t bad; uint32_t pad; };       // 0, or 0xffffffff - (index of the first corrupt member)
struct InfTables {
    uint16_t lfast[1u << kInfLitBits], dfast[1u << kInfDistBits];     // (symbol << 4) | code length; 0: no code this short
    uint16_t lsym[288], dsym[32];                                     // the symbols in the canonical code's order
    uint16_t lcnt[16], dcnt[16];                                      // codes per length
    uint16_t off[16], base[16];                                       // (while a table is made)
    uint32_t crc[64];
    uint8_t lens[320];
};
struct DInflate {
    const uint8_t *comp;         // the uploaded bytes (8-byte aligned, kInfPad behind them)
    const InfMember *members;
    uint32_t nMembers;
    uint8_t *out;                // the text (8-byte aligned, kInfPad behind it)
    uint32_t *err;               // per member: why it is corrupt (0: it is not)
    InfStatus *st;
    uint32_t *blocks;            // per member: the deflate blocks it held (nullptr: not kept; the CPU harness asks)
};

// ---- the host's part: the table of the whole members in z[0, nBytes), from their headers (the test BgzfImpl::fill applies,
// cf_bytesource.cpp) and trailers.  Member m's payload lies at inAt + (its place in z), its text goes to textAt + (the ISIZEs in
// front of it); the caller sees to it that textAt + total fits the table's 32 bits.  out == nullptr: nothing is written, the call
// yields the count and the total.  -> kInfOk, or kInfHeader with nMembers the number of the member whose header or size is not
// BGZF's.  Members that claim 2^32 - 65536 bytes of text or more are refused by exception: no batch holds them.
inline uint32_t bgzf_member_table(const uint8_t *z, uint64_t nBytes, uint64_t inAt, uint64_t textAt, InfMember *out, uint64_t &nMembers, uint64_t &total) {
    uint64_t at = 0;
    nMembers = 0; total = 0;
    for (; at < nBytes; nMembers++) {
        const uint8_t *h = z + at;
        bool ok = nBytes - at >= 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4);
        const uint64_t xlen = ok ? (uint64_t)(h[10] | (h[11] << 8)) : 0, bsize = ok ? (uint64_t)(h[16] | (h[17] << 8)) + 1 : 0;
        ok = ok && xlen >= 6 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0 && bsize >= 12 + xlen + 8 && bsize <= nBytes - at;
        uint32_t crc = 0, isize = 0;
        if (ok) { std::memcpy(&crc, h + bsize - 8, 4); std::memcpy(&isize, h + bsize - 4, 4); ok = isize <= kInfMaxOut; }
        if (!ok) return kInfHeader;
        if (out) out[nMembers] = InfMember{(uint32_t)(inAt + at + 12 + xlen), (uint32_t)(bsize - 12 - xlen - 8), (uint32_t)(textAt + total), isize, crc};
        total += isize; at += bsize;
        if (total >= 0xffff0000ull) throw std::length_error("the text of a batch holds fewer than 2^32 - 65536 bytes (32-bit places in it)");
    }
    return kInfOk;
}

CF_DEV uint64_t inf_load8(const uint8_t *base, uint64_t off) {
    const uint64_t a = off & ~7ull;
    const uint32_t sh = (uint32_t)(off & 7) * 8;
    const uint64_t lo = cf_load8(base + a);
    if (sh == 0) return lo;
    return (lo >> sh) | (cf_load8(base + a + 8) << (64 - sh));
}
template <uint32_t W> CF_DEV void inf_fence() { if (W > 1) cf_wave_fence(); }

struct InfBits {
    const uint8_t *base;
    uint64_t ip, iend;           // next byte to fetch, the payload's end
    uint64_t bb;
    uint32_t bc;
    bool over;                   // more bits were asked for than the payload holds
};
// at least 33 bits in the buffer, unless the payload ends first (the bits behind its end are zero and are never handed out)
CF_DEV void inf_refill(InfBits &b) {
    if (b.bc <= 32 && b.ip < b.iend) {
        uint64_t v = inf_load8(b.base, b.ip) & 0xffffffffull;
        const uint32_t n = b.iend - b.ip >= 4 ? 4u : (uint32_t)(b.iend - b.ip);
        if (n < 4) v &= (1ull << (8 * n)) - 1;
        b.bb |= v << b.bc; b.bc += 8 * n; b.ip += n;
    }
}
CF_DEV void inf_drop(InfBits &b, uint32_t n) {
    if (n > b.bc) { b.over = true; b.bb = 0; b.bc = 0; return; }
    b.bb >>= n; b.bc -= n;
}
CF_DEV uint32_t inf_take(InfBits &b, uint32_t n) {      // n <= 16
    inf_refill(b);
    const uint32_t v = (uint32_t)b.bb & ((1u << n) - 1u);
    inf_drop(b, n);
    return v;
}
constexpr uint32_t kInfNoSym = 0xffffu;
// the next symbol of a code: through the lookup, or — a longer code — length by length over the counts (the canonical code's
// first code of a length and the place of its symbols follow from them)
CF_DEV uint32_t inf_decode(InfBits &b, const uint16_t *fast, uint32_t fastBits, const uint16_t *cnt, const uint16_t *sym) {
    inf_refill(b);
    const uint32_t e = fast[(uint32_t)b.bb & ((1u << fastBits) - 1u)];
    if (e) { inf_drop(b, e & 15u); return e >> 4; }
    uint32_t code = 0, first = 0, index = 0, bits = (uint32_t)b.bb;
    for (uint32_t len = 1; len <= 15; len++) {
        code |= bits & 1u; bits >>= 1;
        const uint32_t count = cnt[len];
        if (code < first + count) { inf_drop(b, len); return sym[index + (code - first)]; }
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return kInfNoSym;
}
// the tables of one code from the n code lengths at lens (LDS).  codes: the code-length code, which has to be complete; the two
// others may also consist of a single one-bit code (as zlib has it).  A code without any symbol is made — and decodes nothing.
template <uint32_t W>
CF_DEV uint32_t inf_build(InfTables *t, const uint8_t *lens, uint32_t n, uint16_t *cnt, uint16_t *sym, uint16_t *fast, uint32_t fastBits, bool codes, uint32_t lane) {
    inf_fence<W>();
    if (lane == 0) {
        for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
        for (uint32_t i = 0; i < n; i++) cnt[lens[i] & 15u]++;
    }
    for (uint32_t i = lane; i < (1u << fastBits); i += W) fast[i] = 0;
    inf_fence<W>();
    int32_t left = 1;
    uint32_t maxLen = 0;
    for (uint32_t l = 1; l <= 15; l++) {
        left <<= 1; left -= (int32_t)cnt[l];
        if (left < 0) return kInfOverSubscribed;
        if (cnt[l]) maxLen = l;
    }
    if (maxLen && left > 0 && (codes || maxLen != 1)) return kInfIncomplete;
    if (lane == 0) {
        uint32_t o = 0, first = 0;
        for (uint32_t l = 1; l <= 15; l++) { t->off[l] = (uint16_t)o; t->base[l] = (uint16_t)(first - o); o += cnt[l]; first = (first + cnt[l]) << 1; }
        for (uint32_t s = 0; s < n; s++) { const uint32_t l = lens[s] & 15u; if (l) sym[t->off[l]++] = (uint16_t)s; }
    }
    inf_fence<W>();
    const uint32_t total = n - cnt[0];
    for (uint32_t i = lane; i < total; i += W) {
        const uint32_t s = sym[i], l = lens[s] & 15u;
        if (l > fastBits) continue;
        const uint32_t code = (t->base[l] + i) & 0xffffu;              // the i-th code in canonical order
        const uint32_t rev = cf_brev32(code) >> (32u - l);             // (a code's bits come most significant first)
        for (uint32_t k = rev; k < (1u << fastBits); k += 1u << l) fast[k] = (uint16_t)((s << 4) | l);
    }
    inf_fence<W>();
    return kInfOk;
}

// CRC-32 (the gzip trailer's): a * b mod the polynomial, bits reflected as the CRC has them (zlib's multmodp)
CF_DEV uint32_t inf_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (0xedb88320u & (0u - (b & 1u)));
    }
    return p;
}
CF_DEV uint32_t inf_xpow8(uint32_t n) {                  // x^(8 n)
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    for (; n; n >>= 1) { if (n & 1u) p = inf_mulmod(sq, p); sq = inf_mulmod(sq, sq); }
    return p;
}
CF_DEV uint32_t inf_crc_range(const uint8_t *text, uint64_t from, uint64_t to) {
    uint32_t c = 0xffffffffu;
    while (from < to) {
        const uint64_t x = inf_load8(text, from);
        const uint32_t take = to - from >= 8 ? 8u : (uint32_t)(to - from);
        for (uint32_t h = 0; 4 * h < take; h++) {
            const uint32_t nb = take - 4 * h >= 4 ? 4u : take - 4 * h;
            uint32_t v = (uint32_t)(x >> (32 * h));
            if (nb < 4) v &= (1u << (8 * nb)) - 1u;
            c ^= v;
            for (uint32_t k = 0; k < 8 * nb; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
        }
        from += take;
    }
    return ~c;
}

// one member, by the W lanes that call this with the same arguments (lane: the caller's number among them)
template <uint32_t W>
CF_DEV uint32_t inflate_member(const DInflate &d, const InfMember &mb, InfTables *t, uint32_t lane, uint32_t &nBlocks) {
    InfBits b;
    b.base = d.comp; b.ip = mb.inOff; b.iend = (uint64_t)mb.inOff + mb.inLen; b.bb = 0; b.bc = 0; b.over = false;
    uint8_t *const out = d.out + mb.outOff;
    const uint32_t outLen = mb.outLen;
    uint32_t op = 0;
    for (uint32_t last = 0; !last;) {
        last = inf_take(b, 1);
        nBlocks++;
        const uint32_t type = inf_take(b, 2);
        if (b.over) return kInfInOverrun;
        if (type == 3) return kInfBadBlockType;
        if (type == 0) {
            // stored: back to whole bytes (the buffer holds whole bytes beyond the bits in use: they are handed back)
            inf_drop(b, b.bc & 7u);
            b.ip -= b.bc >> 3; b.bb = 0; b.bc = 0;
            const uint32_t len = inf_take(b, 16), nlen = inf_take(b, 16);
            if (b.over) return kInfInOverrun;
            if ((len ^ nlen) != 0xffffu) return kInfStoredLen;
            b.ip -= b.bc >> 3; b.bb = 0; b.bc = 0;
            if (len > b.iend - b.ip) return kInfInOverrun;
            if (len > outLen - op) return kInfOutOverrun;
            for (uint32_t i = lane; i < len; i += W) out[op + i] = d.comp[b.ip + i];
            b.ip += len; op += len;
            continue;
        }
        if (type == 1) {
            inf_fence<W>();
            for (uint32_t i = lane; i < 320; i += W) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            (void)inf_build<W>(t, t->lens, 288, t->lcnt, t->lsym, t->lfast, kInfLitBits, false, lane);
            (void)inf_build<W>(t, t->lens + 288, 32, t->dcnt, t->dsym, t->dfast, kInfDistBits, false, lane);
        } else {
            const uint32_t nlen = inf_take(b, 5) + 257, ndist = inf_take(b, 5) + 1, ncode = inf_take(b, 4) + 4;
            if (b.over) return kInfInOverrun;
            if (nlen > 286 || ndist > 30) return kInfTooManyCodes;
            // the code-length code (its tables take the distance code's place for now); every lane reads the lengths and writes
            // the same bytes
            inf_fence<W>();
            const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // the order their lengths come in
            for (uint32_t i = 0; i < 19; i++) t->lens[i] = 0;
            for (uint32_t i = 0; i < ncode; i++) t->lens[kOrder[i]] = (uint8_t)inf_take(b, 3);
            if (b.over) return kInfInOverrun;
            uint32_t e = inf_build<W>(t, t->lens, 19, t->dcnt, t->dsym, t->dfast, 7, true, lane);
            if (e) return e;
            // (the 19 lengths lay where the code lengths now go: the tables are made, they are not needed any more)
            uint32_t i = 0, prev = 0;
            while (i < nlen + ndist) {
                const uint32_t s = inf_decode(b, t->dfast, 7, t->dcnt, t->dsym);
                if (b.over) return kInfInOverrun;
                if (s == kInfNoSym) return kInfBadCode;
                if (s < 16) { t->lens[i++] = (uint8_t)s; prev = s; continue; }
                uint32_t rep, val = 0;
                if (s == 16) { if (i == 0) return kInfBadRepeat; val = prev; rep = 3 + inf_take(b, 2); }
                else if (s == 17) rep = 3 + inf_take(b, 3);
                else rep = 11 + inf_take(b, 7);
                if (b.over) return kInfInOverrun;
                if (i + rep > nlen + ndist) return kInfBadRepeat;
                for (uint32_t k = 0; k < rep; k++) t->lens[i++] = (uint8_t)val;
                prev = val;
            }
            inf_fence<W>();
            if (t->lens[256] == 0) return kInfNoEndCode;
            // the distance lengths behind the room of 288 length / literal symbols
            uint8_t dl[30];
#pragma unroll
            for (uint32_t k = 0; k < 30; k++) dl[k] = k < ndist ? t->lens[nlen + k] : (uint8_t)0;
            inf_fence<W>();
#pragma unroll
            for (uint32_t k = 0; k < 30; k++) t->lens[288 + k] = dl[k];
            e = inf_build<W>(t, t->lens, nlen, t->lcnt, t->lsym, t->lfast, kInfLitBits, false, lane);
            if (e) return e;
            e = inf_build<W>(t, t->lens + 288, ndist, t->dcnt, t->dsym, t->dfast, kInfDistBits, false, lane);
            if (e) return e;
        }
        for (;;) {
            uint32_t s = inf_decode(b, t->lfast, kInfLitBits, t->lcnt, t->lsym);
            if (b.over) return kInfInOverrun;
            if (s == kInfNoSym) return kInfBadCode;
            if (s < 256) {
                if (op >= outLen) return kInfOutOverrun;
                if (lane == (op & (W - 1u))) out[op] = (uint8_t)s;
                op++;
                continue;
            }
            if (s == 256) break;
            if (s >= 286) return kInfBadLenSym;
            s -= 257;
            uint32_t len;
            if (s < 8) len = 3 + s;
            else if (s == 28) len = 258;
            else { const uint32_t eb = (s >> 2) - 1; len = 3 + ((4 + (s & 3u)) << eb) + inf_take(b, eb); }
            const uint32_t ds = inf_decode(b, t->dfast, kInfDistBits, t->dcnt, t->dsym);
            if (b.over) return kInfInOverrun;
            if (ds == kInfNoSym) return kInfBadCode;
            if (ds >= 30) return kInfBadDistSym;
            uint32_t dist;
            if (ds < 4) dist = 1 + ds;
            else { const uint32_t eb = (ds >> 1) - 1; dist = 1 + ((2 + (ds & 1u)) << eb) + inf_take(b, eb); }
            if (b.over) return kInfInOverrun;
            if (dist > op) return kInfDistTooFar;
            if (len > outLen - op) return kInfOutOverrun;
            // the bytes the match reads were stored before this point, by other lanes too
            inf_fence<W>();
            const uint8_t *src = out + (op - dist);
            if (dist >= len) { for (uint32_t i = lane; i < len; i += W) out[op + i] = src[i]; }
            else { for (uint32_t i = lane; i < len; i += W) out[op + i] = src[i % dist]; }
            op += len;
        }
    }
    if (op != outLen) return kInfOutShort;
    if (outLen) {
        inf_fence<W>();
        const uint32_t chunk = (outLen + W - 1) / W;
        const uint32_t from = lane * chunk < outLen ? lane * chunk : outLen, to = from + chunk < outLen ? from + chunk : outLen;
        t->crc[lane] = inf_crc_range(d.out, (uint64_t)mb.outOff + from, (uint64_t)mb.outOff + to);
        inf_fence<W>();
        uint32_t crc = 0;
        const uint32_t xFull = inf_xpow8(chunk);
        for (uint32_t l = 0; l < W && l * chunk < outLen; l++) {
            const uint32_t n = outLen - l * chunk < chunk ? outLen - l * chunk : chunk;
            crc = inf_mulmod(n == chunk ? xFull : inf_xpow8(n), crc) ^ t->crc[l];
        }
        if (crc != mb.crc) return kInfCrc;
    }
    return kInfOk;
}

// member m by W lanes; t: the tables' room, these lanes' own
template <uint32_t W>
CF_DEV void inflate_body(const DInflate &d, uint32_t m, uint32_t lane, InfTables *t) {
    if (m >= d.nMembers) return;
    const InfMember mb = d.members[m];
    uint32_t nBlocks = 0;
    const uint32_t e = inflate_member<W>(d, mb, t, lane, nBlocks);
    if (lane == 0) {
        if (d.blocks) d.blocks[m] = nBlocks;
        d.err[m] = e;
        if (e) cf_atomic_max(&d.st->bad, 0xffffffffu - m);
    }
}

// ---- where the text of a BGZF upload is cut: everything in front of the cut is whole records (and goes through the record, pack
// and format passes of cf_textio.hpp), what lies behind it is the next upload's head.  Purely syntactic:
//   FASTQ  behind the last '\n' whose count from the text's start is a multiple of 4
//   FASTA  in front of the last '>' that starts the text or follows a '\n'
//   TAB5 / TAB6 (fastq == 2)  behind the last '\n'; with `last` a text that does not end in '\n' is irregular (the record pass says so)
// `last` (no member follows): the text's end.  One thread; pos / total are the marker pass's ('>' or '\n' places, their number).
struct DTextCut {
    const uint8_t *text;
    uint64_t nBytes;
    const uint32_t *pos;
    const uint64_t *total;
    uint64_t posCap;
    uint32_t fastq, last;        // fastq: 0 FASTA, 1 FASTQ, 2 a record a line (the tabbed formats)
    uint64_t *cut;               // [0] the cut, [1] the markers in front of it (what the record pass takes as their number)
};
CF_DEV void text_cut_body(const DTextCut &c) {
    const uint64_t n = *c.total;
    uint64_t cut = 0, k = 0;
    if (n > c.posCap) { cut = c.nBytes; k = n; }         // (more markers than are kept: the record pass refuses the block)
    else if (c.last) { cut = c.nBytes; k = n; }
    else if (c.fastq == 2) { k = n; cut = k ? (uint64_t)c.pos[k - 1] + 1 : 0; }
    else if (c.fastq) { k = n & ~3ull; cut = k ? (uint64_t)c.pos[k - 1] + 1 : 0; }
    else {
        k = n;
        while (k) { const uint32_t p = c.pos[k - 1]; k--; if (p == 0 || c.text[p - 1] == '\n') { cut = p; break; } }
        if (cut == 0) k = 0;
    }
    c.cut[0] = cut; c.cut[1] = k;
}

// ---- mates: the texts of the two files of a BGZF pair upload are cut at a COMMON record.  Block i holds k_i whole records under
// the rule above (with its own `last`); n = min(k_0, k_1) records of either go through, so block i is cut behind its record n:
//   a block with k_i == n   the cut of the rule above (and what that rule says of a last text that does not end a record)
//   FASTQ                   behind '\n' number 4 n (0: the text's start)
//   FASTA                   in front of '>' number n, which has to start the text or follow a '\n': one that does not makes the
//                           block irregular (kCutBadStart into *flags) — nothing is guessed
// A block with more markers than are kept keeps the cut of the rule above, and the record pass refuses it.  One thread, as above.
constexpr uint32_t kCutBadStart = 1u;                   // (kTxBadStart of cf_textio.hpp)
struct DTextCutPair {
    DTextCut blk[2];             // blk[i].cut: [0] block i's cut, [1] the markers in front of it
    uint32_t *flags;             // TextStatus::flags
};
CF_DEV void text_cut_pair_body(const DTextCutPair &c) {
    uint64_t own0[2], own1[2];
    DTextCut s0 = c.blk[0], s1 = c.blk[1];
    s0.cut = own0; s1.cut = own1;
    text_cut_body(s0); text_cut_body(s1);
    const uint64_t k0 = s0.fastq ? own0[1] >> 2 : own0[1], k1 = s1.fastq ? own1[1] >> 2 : own1[1];
    const uint64_t n = k0 < k1 ? k0 : k1;
#pragma unroll
    for (uint32_t i = 0; i < 2; i++) {
        const DTextCut &b = c.blk[i];
        uint64_t cut = i ? own1[0] : own0[0], markers = i ? own1[1] : own0[1];
        if (*b.total <= b.posCap && n != (i ? k1 : k0)) {
            if (b.fastq) { markers = 4 * n; cut = n ? (uint64_t)b.pos[4 * n - 1] + 1 : 0; }
            else {
                const uint32_t p = b.pos[n];
                if (p != 0 && b.text[p - 1] != '\n') cf_atomic_or(c.flags, kCutBadStart);
                markers = n; cut = p;
            }
        }
        b.cut[0] = cut; b.cut[1] = markers;
    }
}

}  // namespace cfamd
