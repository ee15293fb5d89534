// cf_deflate.hpp — the formatted text DEFLATED ON THE DEVICE into BGZF members: the other direction of cf_inflate.hpp.
//
// The text a batch's format pass left on the device is cut into members of `member` text bytes (65,280, htslib's; the last one
// of a batch is shorter).  ONE WAVEFRONT MAKES ONE MEMBER:
//   * the member's text is dealt to the 64 lanes in equal pieces of member / 64 bytes (lanes behind the text's end have none);
//   * every lane runs a greedy LZ77 matcher over its own piece (matches of 3 .. 258 bytes, clipped at the piece's end), through a
//     hash table of its own in LDS — kDefHashSize places of 16 bits, the table of lane l at [h * 64 + l]: the 64 lanes' accesses
//     fall into 32 different banks — that it fills from the kDefWindow bytes in front of its piece (never from in front of the
//     member's first byte: a member inflates alone) before it starts.  What a lane finds depends on the text alone;
//   * one fixed-Huffman block per member (BFINAL = 1, BTYPE = 01).  Two passes, as the formatter has them: the matcher once for the
//     lanes' bit counts, a prefix sum over the wavefront for their bit offsets, the same matcher again to write.  The byte in which
//     one lane's bits end and the next lane's begin is the NEXT lane's: the size pass keeps a lane's last bits, a shuffle hands
//     them on, and the next lane starts its bit buffer with them.  Every byte is stored once, by one lane;
//   * a member whose fixed block would be longer than the stored form (text + 5 bytes) is stored (BTYPE = 00) by the whole
//     wavefront — bytes >= 144 cost 9 bits as literals —, so a member never outgrows BGZF's 65,536 bytes;
//   * the 18-byte BGZF header, the CRC32 (every lane folds its piece; the shares are put together as the inflater does it) and ISIZE.
// Members are written at the fixed stride def_stride(member); their sizes go to `size` and are scanned, and compact_body moves
// them together.  The bytes are a pure function of (text, member): the same on every run, on the device and in the CPU harness
// (tests/emu/emu_deflate.cpp, 64 fibers).
//
// The text is read in aligned 8-byte words: it starts on an 8-byte boundary and kInfPad bytes behind it may be fetched (never used).
#pragma once
#include "cf_inflate.hpp"

namespace cfamd {

constexpr uint32_t kDefLanes = 64;
constexpr uint32_t kDefMember = 65280;                  // text bytes per member (htslib's BGZF_BLOCK_SIZE 0xff00)
// (the two choices below can be overridden when the CPU harness is built — tools/deflate_ratio.py compares them; the library never is)
#ifndef CF_DEF_HASH_BITS
#define CF_DEF_HASH_BITS 8
#endif
#ifndef CF_DEF_WINDOW
#define CF_DEF_WINDOW 1024
#endif
constexpr uint32_t kDefHashBits = CF_DEF_HASH_BITS, kDefHashSize = 1u << kDefHashBits;
constexpr uint32_t kDefWindow = CF_DEF_WINDOW;          // bytes in front of a lane's piece that its matches may reach into
constexpr uint32_t kDefMinMatch = 3, kDefMaxMatch = 258;
constexpr uint32_t kDefHead = 18, kDefTail = 8;         // a member's header and trailer
constexpr uint32_t kDefTableWords = kDefHashSize * kDefLanes;          // 16-bit places: a wavefront's tables
static_assert(kDefWindow + kDefMember / kDefLanes < 0xffffu && kDefWindow + kDefMember / kDefLanes <= 32768u, "a place fits 16 bits, a distance DEFLATE's window");
// a member's room: header, the stored form (5 + text) at most, trailer
constexpr uint32_t def_stride(uint32_t member) { return (kDefHead + 5u + member + kDefTail + 7u) & ~7u; }
constexpr bool def_member_ok(uint64_t member) { return member >= kDefLanes && member <= kDefMember && member % kDefLanes == 0; }

struct DDeflate {
    const uint8_t *text;         // 8-byte aligned, kInfPad behind it
    uint64_t nBytes;
    uint32_t member;             // text bytes per member (def_member_ok)
    uint32_t nMembers;           // ceil(nBytes / member)
    uint8_t *out;                // nMembers * def_stride(member)
    uint32_t *size;              // per member: its bytes
};

CF_DEV uint32_t def_log2(uint32_t x) { return 31u - (uint32_t)cf_ctz32(cf_brev32(x)); }            // x != 0
CF_DEV uint32_t def_hash(uint64_t w) { return (((uint32_t)w & 0xffffffu) * 0x9e3779b1u) >> (32u - kDefHashBits); }

// a lane's bits: counted, and — WRITE — stored as whole bytes at dst.  `last` holds the newest bits, the very last one at bit 63.
template <bool WRITE>
struct DefBits {
    uint8_t *dst;
    uint64_t acc, last;
    uint32_t cnt, bits;
    CF_DEV void put(uint32_t v, uint32_t n) {           // 1 <= n <= 16, v < 2^n; the low bit goes first
        bits += n;
        if (WRITE) {
            acc |= (uint64_t)v << cnt; cnt += n;
            while (cnt >= 8) { *dst++ = (uint8_t)acc; acc >>= 8; cnt -= 8; }
        } else last = (last >> n) | ((uint64_t)v << (64u - n));
    }
    CF_DEV void code(uint32_t c, uint32_t n) { put(cf_brev32(c) >> (32u - n), n); }        // a Huffman code: its high bit goes first
    CF_DEV void literal(uint32_t b) { if (b < 144) code(0x30u + b, 8); else code(0x190u + (b - 144u), 9); }
    CF_DEV void symbol(uint32_t s) { if (s < 280) code(s - 256u, 7); else code(0xc0u + (s - 280u), 8); }   // 256 .. 287
    CF_DEV void match(uint32_t len, uint32_t dist) {
        const uint32_t l = len - 3u;
        if (len == 258) symbol(285);
        else if (l < 8) symbol(257u + l);
        else { const uint32_t eb = def_log2(l) - 2u; symbol(257u + 4u * (eb + 1u) + ((l >> eb) & 3u)); put(l & ((1u << eb) - 1u), eb); }
        const uint32_t d = dist - 1u;
        if (d < 4) code(d, 5);
        else { const uint32_t eb = def_log2(d) - 1u; code(2u * (eb + 1u) + ((d >> eb) & 1u), 5); put(d & ((1u << eb) - 1u), eb); }
    }
};

// the bytes a + i == b + i, i < max, before the first that differs (a < b; the words are fetched beyond max, nothing of them is used)
CF_DEV uint32_t def_match_len(const uint8_t *text, uint64_t a, uint64_t b, uint32_t max) {
    uint32_t n = 0;
    while (n < max) {
        const uint64_t x = inf_load8(text, a + n) ^ inf_load8(text, b + n);
        if (x) { n += (uint32_t)cf_ctz64(x) >> 3; break; }
        n += 8;
    }
    return n < max ? n : max;
}

// the piece [from, to) of the member [m0, m1) by one lane: literals and matches into `o`.  tab: the lane's table, its places
// kDefLanes apart.  A place is 1 + (position - lo), 0: none; lo = the window's start.
template <bool WRITE>
CF_DEV void def_piece(const uint8_t *text, uint64_t m0, uint64_t m1, uint64_t from, uint64_t to, uint16_t *tab, DefBits<WRITE> &o) {
    if (from >= to) return;
    const uint64_t lo = from - m0 > kDefWindow ? from - kDefWindow : m0;
    for (uint32_t h = 0; h < kDefHashSize; h++) tab[h * kDefLanes] = 0;
    for (uint64_t p = lo; p < from && p + kDefMinMatch <= m1; p++) tab[def_hash(inf_load8(text, p)) * kDefLanes] = (uint16_t)(p - lo + 1);
    uint64_t p = from;
    while (p < to) {
        const uint64_t w = inf_load8(text, p);
        if (p + kDefMinMatch > to) { o.literal((uint32_t)w & 0xffu); p++; continue; }
        uint16_t *const e = tab + def_hash(w) * kDefLanes;
        const uint32_t cand = *e;
        *e = (uint16_t)(p - lo + 1);
        uint32_t len = 0;
        if (cand) {
            const uint32_t max = to - p < kDefMaxMatch ? (uint32_t)(to - p) : kDefMaxMatch;
            len = def_match_len(text, lo + cand - 1, p, max);
        }
        if (len < kDefMinMatch) { o.literal((uint32_t)w & 0xffu); p++; continue; }
        o.match(len, (uint32_t)(p - (lo + cand - 1)));
        // the places inside the match are kept too: the next row of a table repeats this one
        for (uint64_t q = p + 1; q < p + len && q + kDefMinMatch <= to; q++) tab[def_hash(inf_load8(text, q)) * kDefLanes] = (uint16_t)(q - lo + 1);
        p += len;
    }
}

// member m by the 64 lanes of a wavefront; tab: kDefTableWords places, the wavefront's own
CF_DEV void deflate_body(const DDeflate &d, uint32_t m, uint32_t lane, uint16_t *tab) {
    if (m >= d.nMembers) return;
    const uint64_t m0 = (uint64_t)m * d.member, m1 = m0 + d.member < d.nBytes ? m0 + d.member : d.nBytes;
    const uint32_t len = (uint32_t)(m1 - m0), piece = d.member / kDefLanes;
    const uint32_t nl = (len + piece - 1) / piece;        // the lanes that have text; the last of them ends the block
    const uint64_t from = m0 + (uint64_t)lane * piece < m1 ? m0 + (uint64_t)lane * piece : m1, to = from + piece < m1 ? from + piece : m1;
    uint8_t *const out = d.out + (uint64_t)m * def_stride(d.member);
    uint16_t *const mine = tab + lane;

    // the size pass: this lane's bits (the block's three header bits are lane 0's, the end code the last lane's) and its last ones
    DefBits<false> s{nullptr, 0, 0, 0, 0};
    if (lane == 0) s.put(3, 3);                            // BFINAL = 1, BTYPE = 01
    def_piece<false>(d.text, m0, m1, from, to, mine, s);
    if (lane + 1 == nl) s.symbol(256);
    uint32_t incl = s.bits;
    for (uint32_t k = 1; k < kDefLanes; k <<= 1) { const uint32_t t = cf_shfl(incl, (int)(lane - k)); if (lane >= k) incl += t; }
    const uint32_t total = cf_shfl(incl, (int)(kDefLanes - 1)), at = incl - s.bits;
    // (a lane with text has 8 bits or more, so the bits of the byte it shares with the next lane are all its own)
    const uint32_t endBits = incl & 7u;
    const uint32_t carry = cf_shfl(endBits ? (uint32_t)(s.last >> (64u - endBits)) : 0u, (int)(lane - 1));

    const uint32_t fixedBytes = (total + 7u) >> 3;
    uint32_t payload;
    if (fixedBytes > len + 5u) {
        payload = len + 5u;
        if (lane == 0) { out[kDefHead] = 1; out[kDefHead + 1] = (uint8_t)len; out[kDefHead + 2] = (uint8_t)(len >> 8); out[kDefHead + 3] = (uint8_t)~len; out[kDefHead + 4] = (uint8_t)(~len >> 8); }
        for (uint32_t i = lane; i < len; i += kDefLanes) out[kDefHead + 5 + i] = d.text[m0 + i];
    } else {
        payload = fixedBytes;
        if (lane < nl) {
            DefBits<true> w{out + kDefHead + (at >> 3), lane ? carry : 0u, 0, at & 7u, 0};
            if (lane == 0) w.put(3, 3);
            def_piece<true>(d.text, m0, m1, from, to, mine, w);
            if (lane + 1 == nl) { w.symbol(256); if (w.cnt) *w.dst = (uint8_t)w.acc; }
        }
    }

    // the CRC32 of the text: every lane its piece, then crc(A|B) = crc(A) * x^(8|B|) + crc(B)
    const uint32_t share = from < to ? inf_crc_range(d.text, from, to) : 0u;
    const uint32_t xFull = inf_xpow8(piece);
    uint32_t crc = 0;
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t n = len - l * piece < piece ? len - l * piece : piece;
        crc = inf_mulmod(n == piece ? xFull : inf_xpow8(n), crc) ^ cf_shfl(share, (int)l);
    }
    if (lane == 0) {
        const uint32_t size = kDefHead + payload + kDefTail, bsize = size - 1u;
        const uint8_t head[kDefHead] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
        for (uint32_t i = 0; i < kDefHead; i++) out[i] = head[i];
        uint8_t *t = out + kDefHead + payload;
        for (uint32_t i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(len >> (8 * i)); }
        d.size[m] = size;
    }
}

// the members moved together: member m's bytes from its place at the stride to off[m] (the scan of the sizes), by the threads of a block
struct DDefCompact {
    const uint8_t *in;
    uint32_t stride, nMembers;
    const uint32_t *size;
    const uint64_t *off;
    uint8_t *out;
};
CF_DEV void def_compact_body(const DDefCompact &c, uint32_t m, uint32_t thread, uint32_t threads) {
    if (m >= c.nMembers) return;
    const uint8_t *src = c.in + (uint64_t)m * c.stride;
    uint8_t *dst = c.out + c.off[m];
    for (uint32_t i = thread, n = c.size[m]; i < n; i += threads) dst[i] = src[i];
}

}  // namespace cfamd
