// cf_textio.hpp — the front end's ingest and egress ON THE DEVICE (round 6).
//
// Ingest: a block of whole FASTA / FASTQ records goes up as the file holds it (113 bytes per 100-base read); the kernels below find
// the records, check that every one of them has the PLAIN form — the one form in which this file and the host parser
// (cf_ingest.cpp: FastaPatternSource::read pat.cpp:725-850, FastqPatternSource::read pat.cpp:852-1100) cannot disagree —, and make
// what the batch needs: lengths, the per-read seeds (genRandSeed, pat.h:55-91), the 2-bit words and N masks.  A block with ANY
// record outside the plain form is not parsed here at all: the status says so and the caller hands that block to the host parser
// (whose semantics are the reference's, record by record).  The plain form:
//   FASTA  the block starts with '>'; every '>' starts a record; a record is a non-empty name line without '\r', then one or more
//          lines whose characters are A C G T N in either case, at least one of them
//   FASTQ  four lines per record: '@' + non-empty name without '\r'; a non-empty line of A C G T N in either case; a line that
//          starts with '+'; as many quality characters (all >= 33) as bases; the block ends with the last record's '\n'
//   TAB5 / TAB6 (--tab5 / --12 / --tab6; the host side: parseTabChunk after TabbedPatternSource::readPair, pat.cpp:1217-1503)
//          the block ends with '\n'; no '\r' anywhere and no empty line; EVERY line has the same number of tab-separated fields — 3
//          (an unpaired read: name seq qual) or the pair count (5: name seq1 qual1 seq2 qual2; TAB6, 6: name1 seq1 qual1 name2 seq2
//          qual2) — a block with both kinds is refused with kTxFieldCount, a line with any other count with kTxLineCount; names are
//          non-empty; a sequence field is non-empty and holds A C G T N in either case only (a tab is neither a base nor a
//          quality: the fields are delimited first, by every tab of the line); each quality field is exactly as long as its
//          sequence, every character of it >= 33.  A 3-field record r is read r - skip of the batch, a pair record reads
//          2 (r - skip) and 2 (r - skip) + 1; under TAB5 the second mate's readID is the first's; a mate's seed starts from seed0
//          with its own name, bases and qualities; trim5 / trim3 window each mate's fields as they window a FASTQ record's lines.
// Egress: the default eight columns of AlnSinkSam::appendMate — or any other list of its columns, by the same two bodies —
// (aln_sink.h:2279-2337; centrifuge.cpp:520) are formatted here from the narrow rows the batch leaves on the device, the readID
// copied out of the uploaded block (aln_sink.h:2203-2217), into a buffer the host only write()s; and the part of SpeciesMetrics (aln_sink.h:142-172) the per-taxon counters of count_body do not
// hold — the perfect single assignments and the perfect multi-assignment tuples the EM runs on — is tallied by the same pass.
//
// Every body is one thread per item and runs in the CPU harness (tests/emu) as a plain loop; the cross-lane parts are sums only.
#pragma once
#include "cf_platform.hpp"

namespace cfamd {

constexpr uint32_t kTextPiece = 64;                     // bytes per thread of the two marker passes
constexpr uint32_t kTextPad = 128;                      // zero bytes the uploaded block is followed by (whole-piece and whole-word loads)
enum : uint32_t { kTextFasta = 0, kTextFastq = 1, kTextTab5 = 2, kTextTab6 = 3 };
// why a block is not in the plain form (TextStatus::flags; any bit = the host parses it)
enum : uint32_t {
    kTxBadStart = 1u, kTxNoNameEnd = 2u, kTxEmptyName = 4u, kTxCarriageReturn = 8u, kTxBadBase = 16u, kTxEmptySeq = 32u,
    kTxBadPlus = 64u, kTxQualLen = 128u, kTxBadQual = 256u, kTxLineCount = 512u, kTxTooMany = 1024u,
    kTxMateCount = 2048u,                                // (made by the host: the two blocks of a paired upload hold different numbers of records)
    kTxTailRoom = 4096u,                                 // (made by the host: a BGZF upload leaves more text behind its last whole record than the slot keeps room for)
    kTxFieldCount = 8192u,                               // a tabbed block holds pair lines AND three-field lines (made by text_tab_kind from the two bits below)
    kTxTabSingle = 1u << 30, kTxTabPair = 1u << 31       // the record pass: a line of three fields / of the pair count was seen.  Never reported: text_tab_kind takes them out
};
// what a tabbed block's record pass left in TextStatus::flags -> the flags to report; true: the block's lines are pairs
inline bool text_tab_kind(uint32_t &flags) {                        // (host code: after the status came back)
    const bool pairs = (flags & kTxTabPair) != 0;
    if (pairs && (flags & kTxTabSingle)) flags |= kTxFieldCount;
    flags &= ~(kTxTabSingle | kTxTabPair);
    return pairs;
}

constexpr uint32_t kTextStripes = 64;                   // the block's sums are kept in that many places (a wavefront adds to one of them:
                                                        // ten thousand atomics on ONE address took most of the record pass), added up by the host
struct TextStatus {
    unsigned long long nWords[kTextStripes], nBases[kTextStripes];   // sums over the records: packed words, bases
    unsigned long long outBytes;                        // egress: bytes of the formatted rows
    uint32_t maxLen, flags;
    uint32_t tupleWords, dupNames;                      // egress: words of the tuple list that are filled; queries whose readID equals their predecessor's
                                                        // (text_dup_body, with the Kraken-style tally on: no bit of `flags` — the block is still the device's)
    unsigned long long words() const { unsigned long long t = 0; for (uint32_t i = 0; i < kTextStripes; i++) t += nWords[i]; return t; }
    unsigned long long bases() const { unsigned long long t = 0; for (uint32_t i = 0; i < kTextStripes; i++) t += nBases[i]; return t; }
};

CF_DEV uint64_t tx_load8(const uint8_t *base, uint64_t off) {
    const uint64_t a = off & ~7ull;
    const uint32_t sh = (uint32_t)(off & 7) * 8;
    const uint64_t lo = cf_load8(base + a);
    if (sh == 0) return lo;
    return (lo >> sh) | (cf_load8(base + a + 8) << (64 - sh));
}
// the bytes of a block one after the other, fetched as aligned 8-byte words
struct TxCursor {
    const uint8_t *base;
    uint64_t at, w;
    CF_DEV void seek(const uint8_t *b, uint64_t p) { base = b; at = p; w = cf_load8(b + (p & ~7ull)) >> ((p & 7) * 8); }
    CF_DEV uint32_t next() {
        const uint32_t c = (uint32_t)w & 0xffu;
        at++;
        if ((at & 7) == 0) w = cf_load8(base + at); else w >>= 8;
        return c;
    }
};
// 0x80 in every byte of x that equals the marker (exact: no carries between bytes)
CF_DEV uint64_t tx_match8(uint64_t x, uint32_t marker) {
    const uint64_t y = x ^ (0x0101010101010101ull * marker);
    const uint64_t t = (y & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full;
    return ~(t | y | 0x7f7f7f7f7f7f7f7full);
}

// ---- pass 1 and 2: where the markers are ('>' of FASTA: the record starts; '\n' of FASTQ: the line ends), in file order.
// Thread t owns the bytes [64 t, 64 t + 64): it counts its markers (cnt), and — after the exclusive sums of the counts (base) —
// writes their positions.  The block is followed by zero bytes, which are no marker.
struct DTextMark {
    const uint8_t *text;
    uint64_t nBytes;
    uint32_t marker;
    uint32_t *cnt;               // per piece
    const uint64_t *base;        // exclusive sums of cnt (nPieces + 1)
    uint32_t *pos;               // marker positions
    uint64_t posCap;
};
CF_DEV void text_count_body(const DTextMark &m, uint64_t t) {
    const uint64_t o = t * kTextPiece;
    if (o >= m.nBytes) return;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTextPiece / 16; k++) {
        const u64x2 v = cf_load16(m.text + o + 16 * k);
        n += (uint32_t)cf_popc64(tx_match8(v.x, m.marker)) + (uint32_t)cf_popc64(tx_match8(v.y, m.marker));
    }
    m.cnt[t] = n;
}
CF_DEV void text_mark_body(const DTextMark &m, uint64_t t) {
    const uint64_t o = t * kTextPiece;
    if (o >= m.nBytes) return;
    uint64_t at = m.base[t];
#pragma unroll
    for (uint32_t k = 0; k < kTextPiece / 16; k++) {
        const u64x2 v = cf_load16(m.text + o + 16 * k);
        uint64_t a = tx_match8(v.x, m.marker), b = tx_match8(v.y, m.marker);
        while (a) { const int i = cf_ctz64(a) >> 3; if (at < m.posCap) m.pos[at] = (uint32_t)(o + 16 * k + (uint32_t)i); at++; a &= a - 1; }
        while (b) { const int i = cf_ctz64(b) >> 3; if (at < m.posCap) m.pos[at] = (uint32_t)(o + 16 * k + 8 + (uint32_t)i); at++; b &= b - 1; }
    }
}

// ---- pass 3: one thread per record — the plain-form checks, its length, its seed, where its bases and its readID lie.
struct DTextRec {
    const uint8_t *text;
    uint64_t nBytes;
    const uint32_t *pos;         // FASTA: record starts; FASTQ: line ends (four per record)
    const uint64_t *total;       // the number of markers (the last of pass 1's exclusive sums): known on the device only
    uint64_t posCap;             // markers `pos` holds: a block with more is left to the host
    uint32_t recCap;             // records the per-record arrays hold
    uint32_t format;
    uint32_t seed0;              // (globalSeed + 101) * 59 * 61 * 67 * 71 * 73 * 79 * 83 (pat.h:60-68)
    uint32_t *rlen, *seeds;
    uint32_t *seqOff;            // first byte of the record's sequence line(s)
    uint32_t *idOff, *idLen;     // the readID: the name up to the first white space, a trailing /1 /2 /3 removed (aln_sink.h:2203-2217)
    TextStatus *st;
    // mates: two blocks in one buffer (text = this block's first byte, textBase = its place in the buffer: the places left for the
    // later passes count from the buffer's start), record r of block `mate` is read stride * r + mate of the batch
    uint32_t textBase, stride, mate;
    uint32_t *qualOff;           // FASTQ: first byte of the record's quality line (nullptr: not kept; the readQual columns of fmt_rows_write)
    // -5 / -3 / -s (cf_batch_set_text_trim, cf_batch_set_text_skip; all zero: none of it).  A read is the window of its record's
    // bases behind the first trim5 and in front of the last trim3 of them (pat.cpp: the parsers' trimming) — rlen, seeds, seqOff,
    // qualOff and the block's sums speak of the window, the plain-form checks of the whole record.  The block's first `skip`
    // records are checked and leave nothing else behind: record r >= skip is read stride * (r - skip) + mate of the batch.
    uint32_t trim5, trim3, skip;
};
CF_DEV bool tx_isspace(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }
// base letter -> 0..3, 4 = N, 5 = not a plain base letter
CF_DEV uint32_t tx_code(uint32_t c) {
    const uint32_t u = c & 0xdfu;                          // upper case
    const uint32_t v = (u >> 1) & 3u;                      // A C T G -> 0 1 2 3
    if (u == 'A' || u == 'C' || u == 'G' || u == 'T') return v ^ (v >> 1);
    return u == 'N' ? 4u : 5u;
}
// Eight bytes at once (the sequence lines are nearly all of a block): their 2-bit codes gathered into 16 bits (an N and anything
// else as 0), which of them are N, which are no plain base letter at all, which are a '\n' — one bit per byte each.
CF_DEV uint32_t tx_movemask(uint64_t m80) { return (uint32_t)(((m80 >> 7) * 0x0102040810204080ull) >> 56); }
CF_DEV void tx_codes8(uint64_t x, uint32_t &c16, uint32_t &n8, uint32_t &bad8, uint32_t &nl8) {
    const uint64_t u = x & 0xdfdfdfdfdfdfdfdfull;                     // upper case
    const uint64_t mA = tx_match8(u, 'A'), mC = tx_match8(u, 'C'), mG = tx_match8(u, 'G'), mT = tx_match8(u, 'T'), mN = tx_match8(u, 'N');
    uint64_t c = ((mC | mT) >> 7) | ((mG | mT) >> 6);                 // A C G T -> 0 1 2 3 in the low bits of every byte
    c = (c | (c >> 6)) & 0x000f000f000f000full;
    c = (c | (c >> 12)) & 0x000000ff000000ffull;
    c = (c | (c >> 24)) & 0xffffull;
    c16 = (uint32_t)c;
    n8 = tx_movemask(mN);
    bad8 = tx_movemask(~(mA | mC | mG | mT | mN) & 0x8080808080808080ull);
    nl8 = tx_movemask(tx_match8(x, '\n'));
}
CF_DEV uint32_t tx_rotl32(uint32_t v, uint32_t s) { s &= 31u; return s ? (v << s) | (v >> (32u - s)) : v; }
// the seed's term of eight bases that start at base number i (genRandSeed, pat.h:69-75: r ^= code << 2(i mod 16), in 32-bit
// arithmetic): the 2-bit codes land in their fields cyclically; an N is code 4, whose bit lies one field up and falls off the top
CF_DEV uint32_t tx_seed8(uint32_t c16, uint32_t n8, uint32_t i) {
    uint32_t r = tx_rotl32(c16, 2u * (i & 15u));
    while (n8) { const uint32_t j = (uint32_t)cf_ctz32(n8); r ^= 4u << (((i + j) & 15u) << 1); n8 &= n8 - 1; }
    return r;
}
// 0x80 in every byte of x that is below 33 (no carries between bytes)
CF_DEV uint64_t tx_below33(uint64_t x) {
    const uint64_t t = (x & 0x7f7f7f7f7f7f7f7full) + 0x5f5f5f5f5f5f5f5full;       // >= 0x80 where the low seven bits are >= 33
    return ~(t | x) & 0x8080808080808080ull;
}
// the bases of a record from byte `pos` to byte `e` (line ends skipped): their number, their term of the seed, the plain-form check
CF_DEV uint32_t tx_bases(const uint8_t *text, uint64_t pos, uint64_t e, uint32_t &seed, uint32_t &len) {
    while (pos < e) {
        const uint64_t x = tx_load8(text, pos);
        if (e - pos >= 8) {
            uint32_t c16, n8, bad8, nl8;
            tx_codes8(x, c16, n8, bad8, nl8);
            if (nl8 == 0) {
                if (bad8) return kTxBadBase;
                seed ^= tx_seed8(c16, n8, len);
                len += 8; pos += 8;
                continue;
            }
        }
        const uint32_t ch = (uint32_t)x & 0xffu;
        pos++;
        if (ch == '\n') continue;
        const uint32_t code = tx_code(ch);
        if (code > 4) return kTxBadBase;
        seed ^= code << ((len & 15u) << 1);
        len++;
    }
    return 0;
}
// the byte of base number n of a record whose bases start at byte `pos` (line ends stepped over; `e` when it has no more than n)
CF_DEV uint64_t tx_skip_bases(const uint8_t *text, uint64_t pos, uint64_t e, uint32_t n) {
    uint32_t i = 0;
    while (pos < e) {
        const uint64_t x = tx_load8(text, pos);
        if (n - i >= 8 && e - pos >= 8 && tx_match8(x, '\n') == 0) { i += 8; pos += 8; continue; }
        if (((uint32_t)x & 0xffu) == '\n') { pos++; continue; }
        if (i == n) break;                                               // (the first kept base, not a line end in front of it)
        i++; pos++;
    }
    return pos;
}
// the seed's term of the n bases from byte `pos` on (line ends skipped; never past `e`), the first of them base number 0: the window
// of a trimmed record, whose letters tx_bases has checked
CF_DEV uint32_t tx_bases_window(const uint8_t *text, uint64_t pos, uint64_t e, uint32_t n, uint32_t &seed) {
    uint32_t i = 0;
    while (i < n && pos < e) {
        const uint64_t x = tx_load8(text, pos);
        if (n - i >= 8 && e - pos >= 8) {
            uint32_t c16, n8, bad8, nl8;
            tx_codes8(x, c16, n8, bad8, nl8);
            if (nl8 == 0) { seed ^= tx_seed8(c16, n8, i); i += 8; pos += 8; continue; }
        }
        const uint32_t ch = (uint32_t)x & 0xffu;
        pos++;
        if (ch == '\n') continue;
        const uint32_t code = tx_code(ch);
        seed ^= (code > 4 ? 0u : code) << ((i & 15u) << 1);               // (no plain letter: the block is refused anyway)
        i++;
    }
    return i;
}
// the quality characters from byte `pos` to byte `e` of one line: their term of the seed (r ^= q[j] << 8(j mod 4), the first of them
// j = 0: the string's little-endian dwords folded together), kTxBadQual when one of them is below 33
CF_DEV uint32_t tx_quals(const uint8_t *text, uint64_t pos, uint64_t e, uint32_t &seed) {
    uint32_t flags = 0, j = 0;
    while (pos < e) {
        uint64_t x = tx_load8(text, pos);
        const uint32_t take = e - pos >= 8 ? 8u : (uint32_t)(e - pos);
        if (take < 8) x = (x & ((1ull << (8 * take)) - 1)) | (0x2121212121212121ull << (8 * take));   // (the bytes past the line: no offence, and folded out again)
        if (tx_below33(x)) flags |= kTxBadQual;
        if (take < 8) x &= (1ull << (8 * take)) - 1;
        seed ^= tx_rotl32((uint32_t)x ^ (uint32_t)(x >> 32), 8u * (j & 3u));
        j += take; pos += take;
    }
    return flags;
}
// the name line from `from` to its '\n' (which must lie before `lim`): the name's term of the seed, the readID's length
// (stop: what ends the name — the tab behind a tabbed record's name field)
CF_DEV uint32_t tx_name(TxCursor &c, uint64_t lim, uint32_t &r, uint32_t &nameLen, uint32_t &idLen, uint32_t stop = '\n') {
    uint32_t flags = 0, j = 0, ws = 0xffffffffu, p1 = 0, p2 = 0;
    bool slash = false;
    for (;;) {
        if (c.at >= lim) { flags |= kTxNoNameEnd; break; }
        const uint32_t ch = c.next();
        if (ch == stop) break;
        if (ch == '\r') flags |= kTxCarriageReturn;
        if (ch == '/') slash = true;
        if (!slash) r ^= (uint32_t)(int32_t)(int8_t)ch << ((j & 3u) << 3);
        if (ws == 0xffffffffu && tx_isspace(ch)) ws = j;
        p2 = p1; p1 = ch;
        j++;
    }
    nameLen = j;
    uint32_t nl = j;
    if (j >= 2 && p2 == '/' && (p1 == '1' || p1 == '2' || p1 == '3')) nl -= 2;
    idLen = ws < nl ? ws : nl;
    if (j == 0) flags |= kTxEmptyName;
    return flags;
}
struct TextCounts { uint64_t nMarkers; uint32_t nRec; bool fits; };
CF_DEV TextCounts text_counts(const DTextRec &d) {
    TextCounts c;
    c.nMarkers = *d.total;
    const uint64_t rec = d.format == kTextFastq ? c.nMarkers >> 2 : c.nMarkers;          // (a tabbed record is a line)
    c.fits = c.nMarkers <= d.posCap && rec <= d.recCap;
    c.nRec = c.fits ? (uint32_t)rec : 0u;
    return c;
}
// one mate of a tabbed record: its bases [s0, s1) and qualities [q0, q1), fields the caller has delimited by the line's tabs (so
// the 8-byte paths of tx_bases / tx_quals, which never read a field's last bytes as part of a whole word beyond its end, see no
// tab).  trim5 / trim3 window both as they window a FASTQ record's lines.  -> flags; len, seed (^=), where the window starts
CF_DEV uint32_t tx_tab_mate(const DTextRec &d, uint64_t s0, uint64_t s1, uint64_t q0, uint64_t q1, uint32_t &seed, uint32_t &len, uint32_t &seqOff, uint32_t &qualOff) {
    uint32_t flags = 0;
    const uint64_t all = s1 > s0 ? s1 - s0 : 0;
    const uint64_t t5 = d.trim5 < all ? d.trim5 : all, keep = all - t5 > d.trim3 ? all - t5 - d.trim3 : 0;
    const uint64_t b0 = s0 + t5, b1 = b0 + keep;
    uint32_t unused = 0, cnt = 0;
    len = 0;
    seqOff = (uint32_t)b0; qualOff = (uint32_t)(q0 + t5);
    if (all == 0) return kTxEmptySeq;
    if (b0 > s0) flags |= tx_bases(d.text, s0, b0, unused, cnt);
    flags |= tx_bases(d.text, b0, b1, seed, len);
    if (s1 > b1) flags |= tx_bases(d.text, b1, s1, unused, cnt);
    if (q1 < q0 || q1 - q0 != all) return flags | kTxQualLen;
    const uint64_t w0 = q0 + t5, w1 = w0 + keep;
    if (w0 > q0) flags |= tx_quals(d.text, q0, w0, unused);
    flags |= tx_quals(d.text, w0, w1, seed);
    if (q1 > w1) flags |= tx_quals(d.text, w1, q1, unused);
    if (len == 0) flags |= kTxEmptySeq;
    return flags;
}
// a tabbed record: line r of the block, one thread.  -> flags; len: the bases kept of both mates; words: their packed words
CF_DEV uint32_t text_tab_record(const DTextRec &d, uint32_t r, bool kept, uint32_t &len, uint32_t &words, uint32_t &mx) {
    uint32_t flags = 0;
    const uint64_t ls = r ? (uint64_t)d.pos[r - 1] + 1 : 0, le = d.pos[r];
    // the line's tabs (and any '\r'), eight bytes at a time; the places of the first five in scalars of their own
    uint32_t nt = 0;
    uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    for (uint64_t p = ls; p < le; p += 8) {
        const uint64_t x = tx_load8(d.text, p);
        const uint64_t in = le - p >= 8 ? ~0ull : (1ull << (8 * (le - p))) - 1;
        uint64_t m = tx_match8(x, '\t') & in;
        if (tx_match8(x, '\r') & in) flags |= kTxCarriageReturn;
        while (m) {
            const uint64_t at = p + (uint64_t)(cf_ctz64(m) >> 3);
            if (nt == 0) t0 = at; else if (nt == 1) t1 = at; else if (nt == 2) t2 = at; else if (nt == 3) t3 = at; else if (nt == 4) t4 = at;
            nt++; m &= m - 1;
        }
    }
    const uint32_t pairTabs = d.format == kTextTab6 ? 5u : 4u;
    const bool pair = nt == pairTabs;
    if (nt != 2 && !pair) return flags | kTxLineCount;
    flags |= pair ? kTxTabPair : kTxTabSingle;
    // names: a term of the seed each (from 0: XORed into the mate's seed below), the readID's length
    TxCursor c;
    uint32_t term1 = 0, term2, nameLen = 0, idLen1 = 0, idLen2, idOff1 = (uint32_t)ls, idOff2;
    c.seek(d.text, ls);
    flags |= tx_name(c, t0 + 1, term1, nameLen, idLen1, '\t');
    term2 = term1; idLen2 = idLen1; idOff2 = idOff1;
    uint64_t s2 = t2 + 1, e2 = t3, q2 = t3 + 1;                            // TAB5: seq2 and qual2 behind the third tab
    if (pair && d.format == kTextTab6) {
        term2 = 0;
        c.seek(d.text, t2 + 1);
        flags |= tx_name(c, t3 + 1, term2, nameLen, idLen2, '\t');
        idOff2 = (uint32_t)(t2 + 1);
        s2 = t3 + 1; e2 = t4; q2 = t4 + 1;
    }
    uint32_t seed1 = d.seed0 ^ term1, len1 = 0, so1, qo1;
    flags |= tx_tab_mate(d, t0 + 1, t1, t1 + 1, pair ? t2 : le, seed1, len1, so1, qo1);
    const uint64_t w = pair ? 2 * (uint64_t)(r - d.skip) : (uint64_t)(r - d.skip);
    if (kept) {
        d.idOff[w] = d.textBase + idOff1; d.idLen[w] = idLen1; d.seqOff[w] = d.textBase + so1;
        if (d.qualOff) d.qualOff[w] = d.textBase + qo1;
        d.rlen[w] = len1; d.seeds[w] = seed1;
    }
    len = len1; words = (len1 + 31u) >> 5; mx = len1;
    if (pair) {
        uint32_t seed2 = d.seed0 ^ term2, len2 = 0, so2, qo2;
        flags |= tx_tab_mate(d, s2, e2, q2, le, seed2, len2, so2, qo2);
        if (kept) {
            d.idOff[w + 1] = d.textBase + idOff2; d.idLen[w + 1] = idLen2; d.seqOff[w + 1] = d.textBase + so2;
            if (d.qualOff) d.qualOff[w + 1] = d.textBase + qo2;
            d.rlen[w + 1] = len2; d.seeds[w + 1] = seed2;
        }
        len += len2; words += (len2 + 31u) >> 5; mx = len2 > mx ? len2 : mx;
    }
    return flags;
}
// FMT: the body for FASTA / FASTQ (false: d.format says which, the pass as it was) or for the tabbed formats (true) — two
// instantiations, so that the first keeps its registers
template <bool TAB>
CF_DEV void text_record_body_t(const DTextRec &d, uint32_t r) {
    uint32_t flags = 0, len = 0;
    const TextCounts tc = text_counts(d);
    const bool live = r < tc.nRec;
    if (r == 0) {
        // the checks on the block as a whole
        if (!tc.fits) flags |= kTxTooMany;
        else if (d.nBytes) {
            if (!TAB && d.text[0] != (d.format == kTextFasta ? '>' : '@')) flags |= kTxBadStart;
            if (!TAB && d.format == kTextFastq && ((tc.nMarkers & 3u) || d.text[d.nBytes - 1] != '\n')) flags |= kTxLineCount;
            if (TAB && d.text[d.nBytes - 1] != '\n') flags |= kTxLineCount;
            if (tc.nRec == 0) flags |= kTxBadStart;
        }
    }
    // -s: the block's first records are checked like the others and leave nothing behind
    const bool kept = live && r >= d.skip;
    const uint64_t w = (uint64_t)d.stride * (r - d.skip) + d.mate;      // the read's number in the batch
    const bool trim = (d.trim5 | d.trim3) != 0;                         // (the same for every thread of the launch)
    uint32_t tabWords = 0, tabMax = 0;
    if (TAB) { if (live) flags |= text_tab_record(d, r, kept, len, tabWords, tabMax); }
    else if (live) {
        uint32_t seed = d.seed0, nameLen = 0, idLen = 0, idOff, seqOff, qualOff = 0;
        TxCursor c;
        if (d.format == kTextFasta) {
            const uint64_t s = d.pos[r], e = r + 1 < tc.nRec ? (uint64_t)d.pos[r + 1] : d.nBytes;
            c.seek(d.text, s + 1);
            flags |= tx_name(c, e, seed, nameLen, idLen);
            idOff = (uint32_t)(s + 1);
            if (!trim) {
                seqOff = (uint32_t)c.at;
                flags |= tx_bases(d.text, c.at, e, seed, len);
            } else {
                // -3 needs the record's length first: once over the record for the checks and the count, once over the window
                uint32_t all = 0, unused = 0;
                flags |= tx_bases(d.text, c.at, e, unused, all);
                const uint32_t t5 = d.trim5 < all ? d.trim5 : all, keep = all - t5 > d.trim3 ? all - t5 - d.trim3 : 0u;
                const uint64_t first = tx_skip_bases(d.text, c.at, e, t5);
                seqOff = (uint32_t)first;
                len = tx_bases_window(d.text, first, e, keep, seed);
            }
            // the qualities of a FASTA read are 'I' throughout: their term depends on the length only
            uint32_t q = ((len >> 2) & 1u) ? 0x49494949u : 0u;
            for (uint32_t j = 0; j < (len & 3u); j++) q ^= 0x49u << (j << 3);
            seed ^= q;
        } else {
            const uint64_t ls = r ? (uint64_t)d.pos[4 * (uint64_t)r - 1] + 1 : 0;
            const uint64_t n0 = d.pos[4 * (uint64_t)r], n1 = d.pos[4 * (uint64_t)r + 1], n2 = d.pos[4 * (uint64_t)r + 2], n3 = d.pos[4 * (uint64_t)r + 3];
            if (d.text[ls] != '@') flags |= kTxBadStart;
            c.seek(d.text, ls + 1);
            flags |= tx_name(c, n0 + 1, seed, nameLen, idLen);
            idOff = (uint32_t)(ls + 1);
            if (n2 <= n1 + 1 || d.text[n1 + 1] != '+') flags |= kTxBadPlus;
            if (!trim) {
                seqOff = (uint32_t)(n0 + 1); qualOff = (uint32_t)(n2 + 1);
                flags |= tx_bases(d.text, n0 + 1, n1, seed, len);
                if (n3 - n2 != n1 - n0) flags |= kTxQualLen;
                else flags |= tx_quals(d.text, n2 + 1, n3, seed);
            } else {
                // one line each: the window is a stretch of it — its terms of the seed start over at the window's first base; the
                // parts in front of it and behind it are checked only
                const uint64_t all = n1 > n0 ? n1 - n0 - 1 : 0;
                const uint64_t t5 = d.trim5 < all ? d.trim5 : all, keep = all - t5 > d.trim3 ? all - t5 - d.trim3 : 0;
                const uint64_t b0 = n0 + 1 + t5, b1 = b0 + keep;
                uint32_t unused = 0, cnt = 0;
                seqOff = (uint32_t)b0; qualOff = (uint32_t)(n2 + 1 + t5);
                flags |= tx_bases(d.text, n0 + 1, b0, unused, cnt);
                flags |= tx_bases(d.text, b0, b1, seed, len);
                flags |= tx_bases(d.text, b1, n1, unused, cnt);
                if (n3 - n2 != n1 - n0) flags |= kTxQualLen;
                else {
                    const uint64_t q0 = n2 + 1 + t5, q1 = q0 + keep;
                    flags |= tx_quals(d.text, n2 + 1, q0, unused);
                    flags |= tx_quals(d.text, q0, q1, seed);
                    flags |= tx_quals(d.text, q1, n3, unused);
                }
            }
        }
        if (len == 0) flags |= kTxEmptySeq;
        if (kept) {
            d.idOff[w] = d.textBase + idOff; d.idLen[w] = idLen;
            d.seqOff[w] = d.textBase + seqOff;
            if (d.format != kTextFasta && d.qualOff) d.qualOff[w] = d.textBase + qualOff;
            d.rlen[w] = len; d.seeds[w] = seed;
        }
    }
    // the block's sums: over the wavefront first, one set of atomics per wavefront
    unsigned long long words = kept ? (TAB ? tabWords : (len + 31u) >> 5) : 0u, bases = kept ? len : 0u;
    uint32_t mx = kept ? (TAB ? tabMax : len) : 0u;
    for (int m = CF_WAVE / 2; m > 0; m >>= 1) {
        words += cf_shfl_xor(words, m); bases += cf_shfl_xor(bases, m);
        const uint32_t o = cf_shfl_xor(mx, m); mx = o > mx ? o : mx;
        flags |= cf_shfl_xor(flags, m);
    }
    if (cf_lane() == 0) {
        const uint32_t stripe = (r / CF_WAVE) & (kTextStripes - 1);
        if (words) cf_atomic_add(&d.st->nWords[stripe], words);
        if (bases) cf_atomic_add(&d.st->nBases[stripe], bases);
        if (mx > d.st->maxLen) cf_atomic_max(&d.st->maxLen, mx);      // (the plain read only spares atomics that would change nothing)
        if (flags) cf_atomic_or(&d.st->flags, flags);
    }
}

// ---- with the Kraken-style tally on (cf_kreport_enable): centrifuge-kreport merges NEIGHBOURING rows of equal readID, so two
// neighbouring reads of one name are one read to it and two to the tally.  One thread per query compares its readID with its
// predecessor's and counts the equal ones (TextStatus::dupNames); the batch's first and last readID (their lengths, up to 255 bytes
// of each) and the first such pair's go back to the host, which compares neighbouring batches (cf_batch_text_names).
constexpr uint32_t kTextNameBytes = 255;
struct TextNames {
    uint32_t nDup, dupKey;                              // dupKey = ~(the lowest query that repeats its predecessor's readID); 0: none
    uint32_t firstLen, lastLen, dupLen, pad;
    uint8_t first[kTextNameBytes + 1], last[kTextNameBytes + 1], dup[kTextNameBytes + 1];
};
struct DTextDup {
    const uint8_t *text;
    const uint32_t *idOff, *idLen;
    uint32_t nQueries, paired;                          // (mates: the row carries mate 1's readID)
    TextStatus *st;
    TextNames *names;
};
CF_DEV void text_name_copy(const DTextDup &d, uint32_t q, uint8_t *to, uint32_t &len) {
    const uint32_t r = d.paired ? 2 * q : q, n = d.idLen[r];
    const uint8_t *p = d.text + d.idOff[r];
    for (uint32_t i = 0; i < n && i < kTextNameBytes; i++) to[i] = p[i];
    len = n;
}
CF_DEV void text_dup_body(const DTextDup &d, uint32_t q) {
    if (q >= d.nQueries) return;
    if (q == 0) text_name_copy(d, q, d.names->first, d.names->firstLen);
    if (q == d.nQueries - 1) text_name_copy(d, q, d.names->last, d.names->lastLen);
    if (q == 0) return;
    const uint32_t r = d.paired ? 2 * q : q, rp = d.paired ? 2 * (q - 1) : q - 1, n = d.idLen[r];
    if (d.idLen[rp] != n) return;
    const uint8_t *a = d.text + d.idOff[r], *b = d.text + d.idOff[rp];
    for (uint32_t i = 0; i < n; i++) if (a[i] != b[i]) return;
    cf_atomic_add(&d.st->dupNames, 1u);
    cf_atomic_add(&d.names->nDup, 1u);
    cf_atomic_max(&d.names->dupKey, ~q);
}
// ... behind it, one thread: the readID of the first pair found
CF_DEV void text_dup_name_body(const DTextDup &d) {
    if (d.names->dupKey == 0) return;
    text_name_copy(d, ~d.names->dupKey, d.names->dup, d.names->dupLen);
}

CF_DEV void text_record_body(const DTextRec &d, uint32_t r) {
    if (d.format >= kTextTab5) text_record_body_t<true>(d, r); else text_record_body_t<false>(d, r);
}

// ---- pass 4 (behind the exclusive sums of the reads' word counts): the 2-bit words and the N masks, one thread per record.
struct DTextPack {
    const uint8_t *text;
    const uint32_t *seqOff, *rlen;
    const uint64_t *woff;
    uint64_t *bases;
    uint32_t *nmask;
    uint32_t nReads;
};
CF_DEV void text_pack_body(const DTextPack &d, uint32_t r) {
    if (r >= d.nReads) return;
    const uint32_t L = d.rlen[r];
    const uint64_t wo = d.woff[r];
    uint64_t pos = d.seqOff[r];
    uint32_t i = 0;
    for (uint32_t k = 0; 32 * k < L; k++) {
        uint64_t w = 0;
        uint32_t m = 0;
        uint32_t j = 0;
        while (j < 32 && i < L) {
            const uint64_t x = tx_load8(d.text, pos);
            if ((j & 7u) == 0 && L - i >= 8) {                        // eight bases at once, unless a line ends among them
                uint32_t c16, n8, bad8, nl8;
                tx_codes8(x, c16, n8, bad8, nl8);
                if (nl8 == 0) { w |= (uint64_t)c16 << (2 * j); m |= n8 << j; j += 8; i += 8; pos += 8; continue; }
            }
            const uint32_t ch = (uint32_t)x & 0xffu;
            pos++;
            if (ch == '\n') continue;                                // (a FASTA sequence over several lines)
            const uint32_t code = tx_code(ch);
            if (code > 3) m |= 1u << j; else w |= (uint64_t)code << (2 * j);
            j++; i++;
        }
        d.bases[wo + k] = w;
        d.nmask[wo + k] = m;
    }
}

// ---- egress: a batch's rows as text.  The columns are a program: any list of the fields of AlnSinkSam::appendMate (--tab-fmt-cols,
// --out-fmt sam: centrifuge.cpp:484-520; aln_sink.h:2279-2337), the default one being
//   readID seqID taxID score 2ndBestScore hitLength queryLength numMatches   (centrifuge.cpp:520)
// One thread per query: the size pass (fmt_rows_size) leaves the bytes its rows take, the write pass (fmt_rows_write, behind the
// exclusive sums) writes them; fmt_col_len / fmt_col_put are the one place that knows a column's width and text.
struct TextRow { uint32_t uniqueID, tidx, score, hitLen; };          // = NarrowRow
struct DTextFmt {
    const uint8_t *text;
    const uint32_t *idOff, *idLen, *rlen;
    const TextRow *rows;
    const uint64_t *rowFirst;
    const uint8_t *qinfo;        // rows of the query (six bits), "took part" bits of its mates
    const uint32_t *score2, *maxScore;
    uint32_t nQueries, paired;
    // the strings a row repeats: per reference its uid, per taxon its seqID when the row names no reference (the rank's name) and its taxID
    const uint8_t *strs;
    const uint32_t *uidOff, *rankOff, *taxOff;
    const uint8_t *taxLeaf;
    uint32_t nRefs, nTaxa, idxZero;
    uint32_t *size;              // per query
    const uint64_t *outOff;      // exclusive sums of size
    uint8_t *out;
    uint64_t outCap;
    // the tally that is not in the per-taxon counters (aln_sink.h:142-172): perfect single assignments per taxon, and the list of
    // perfect multi-assignment tuples (n, then n taxon indices)
    unsigned long long *single;
    uint32_t *tuples;
    uint32_t tuplesCap;
    TextStatus *st;
    // what the columns beyond the default eight need (the default program reads none of it, and for it all of this may be null):
    // per taxon its rank's and its name's string — nTaxa + 1 of each, the last one tax ID 0's, which an unclassified row prints —,
    // the batch's packed reads (readSeq is printed from them: the uploaded text may be wrapped or lower case), and per read the
    // place of its quality line in `text` (nullptr: FASTA, whose qualities are 'I' throughout)
    const uint8_t *taxStrs;
    const uint32_t *trankOff, *tnameOff;     // places in taxStrs
    const uint64_t *woff, *bases;
    const uint32_t *nmask, *qualOff;
};
CF_DEV uint32_t tx_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
CF_DEV uint8_t *tx_put(uint8_t *w, uint32_t v) {
    const uint32_t n = tx_digits(v);
    for (uint32_t i = n; i-- > 0;) { w[i] = (uint8_t)('0' + v % 10u); v /= 10u; }
    return w + n;
}
CF_DEV uint8_t *tx_copy(uint8_t *w, const uint8_t *s, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) w[i] = s[i];
    return w + n;
}
// The write pass's lds: kFmtLds + 8 bytes of LDS of the thread's WAVEFRONT (or nullptr).  A lane writes its rows a byte at a time,
// its neighbour's rows start ~41 bytes further on: straight to HBM that is one store instruction per byte and 64 scattered bytes per
// instruction.  The 64 queries of a wavefront print one contiguous stretch of the text, so the rows are put together in LDS — at the
// stretch's own phase within a dword — and go out as whole aligned dwords, 256 bytes per store instruction (a stretch that does not
// fit goes the old way).
constexpr uint32_t kFmtLds = 8192;
#ifndef CF_HOST_EMU
// (the kernel is launched in blocks of 256 threads: cf_device.hip k_fmt_write)
CF_DEV uint8_t *fmt_wave_lds() { __shared__ __attribute__((aligned(16))) uint8_t lds[256 / CF_WAVE][kFmtLds + 16]; return lds[threadIdx.x / CF_WAVE]; }
#endif

// The columns.  The short fields (names, numbers) are printed lane by lane; the LONG ones (readSeq*, readQual*: a read's length
// each) are not: a 150-base row would be 150 one-byte stores per lane, scattered over the wavefront's stretch.  They are written by
// the WHOLE wavefront, one field after the other, in aligned dwords — the sequence expanded from the batch's 2-bit words in
// registers, 16 bases per lane.
constexpr uint32_t kTextMaxCols = 32;
enum : uint32_t {
    kColReadId = 0, kColSeqId, kColTaxId, kColTaxRank, kColTaxName, kColScore, kColScore2, kColHitLen, kColQueryLen, kColNumMatches,
    kColSeq, kColQual, kColSeq1, kColQual1, kColSeq2, kColQual2, kColPlaceholder, kColZero, kColCount
};
struct TextCols { uint8_t col[kTextMaxCols]; uint32_t nCols; };
CF_DEV bool tx_col_long(uint32_t c) { return c >= kColSeq && c <= kColQual2; }
CF_DEV bool tx_col_qual(uint32_t c) { return c == kColQual || c == kColQual1 || c == kColQual2; }
// what a query's rows share
struct FmtQuery { uint32_t ra, len1, len2, qlen, n, idn, s2; uint64_t f0; };
CF_DEV FmtQuery fmt_query(const DTextFmt &f, uint32_t q) {
    FmtQuery Q;
    Q.ra = f.paired ? 2 * q : q;
    Q.len1 = f.rlen[Q.ra]; Q.len2 = f.paired ? f.rlen[Q.ra + 1] : 0u;
    Q.qlen = Q.len1 + Q.len2;
    Q.n = f.qinfo[q] & 0x3fu; Q.idn = f.idLen[Q.ra]; Q.s2 = f.score2[q];
    Q.f0 = Q.n ? f.rowFirst[q] : 0;
    return Q;
}
CF_DEV uint32_t fmt_long_len(const DTextFmt &f, const FmtQuery &Q, uint32_t c) {
    if (c == kColSeq || c == kColQual) return f.paired ? Q.len1 + 1 + Q.len2 : Q.len1;        // seq1_seq2
    if (c == kColSeq1 || c == kColQual1) return Q.len1;
    return f.paired ? Q.len2 : 0u;                                                                // (no second mate: empty)
}
// bytes of column c in a row of the query (uncl: the one row of a query without rows — seqID "unclassified", taxID, score, hitLength 0)
CF_DEV uint32_t fmt_col_len(const DTextFmt &f, const FmtQuery &Q, uint32_t c, bool uncl, const TextRow &row) {
    const uint32_t t = row.tidx < f.nTaxa ? row.tidx : 0u, tz = uncl ? f.nTaxa : t;
    switch (c) {
        case kColReadId: return Q.idn;
        case kColSeqId:
            if (uncl) return 12u;
            return f.taxLeaf[t] && row.uniqueID < f.nRefs ? f.uidOff[row.uniqueID + 1] - f.uidOff[row.uniqueID] : f.rankOff[t + 1] - f.rankOff[t];
        case kColTaxId: return uncl ? 1u : f.taxOff[t + 1] - f.taxOff[t];
        case kColTaxRank: return f.trankOff[tz + 1] - f.trankOff[tz];
        case kColTaxName: return f.tnameOff[tz + 1] - f.tnameOff[tz];
        case kColScore: return uncl ? 1u : tx_digits(row.score);
        case kColScore2: return tx_digits(Q.s2);
        case kColHitLen: return uncl ? 1u : tx_digits(row.hitLen);
        case kColQueryLen: return tx_digits(Q.qlen);
        case kColNumMatches: return tx_digits(Q.n ? Q.n : 1u);
        case kColPlaceholder: return 2u;
        case kColZero: return 1u;
        default: return fmt_long_len(f, Q, c);
    }
}
// a short column printed at w
CF_DEV uint8_t *fmt_col_put(const DTextFmt &f, const FmtQuery &Q, uint32_t c, bool uncl, const TextRow &row, uint8_t *w) {
    const uint32_t t = row.tidx < f.nTaxa ? row.tidx : 0u, tz = uncl ? f.nTaxa : t;
    switch (c) {
        case kColReadId: return tx_copy(w, f.text + f.idOff[Q.ra], Q.idn);
        case kColSeqId: {
            if (uncl) { const uint8_t kU[] = {'u', 'n', 'c', 'l', 'a', 's', 's', 'i', 'f', 'i', 'e', 'd'}; for (uint32_t i = 0; i < sizeof kU; i++) *w++ = kU[i]; return w; }
            if (f.taxLeaf[t] && row.uniqueID < f.nRefs) return tx_copy(w, f.strs + f.uidOff[row.uniqueID], f.uidOff[row.uniqueID + 1] - f.uidOff[row.uniqueID]);
            return tx_copy(w, f.strs + f.rankOff[t], f.rankOff[t + 1] - f.rankOff[t]);
        }
        case kColTaxId: if (uncl) { *w++ = '0'; return w; } return tx_copy(w, f.strs + f.taxOff[t], f.taxOff[t + 1] - f.taxOff[t]);
        case kColTaxRank: return tx_copy(w, f.taxStrs + f.trankOff[tz], f.trankOff[tz + 1] - f.trankOff[tz]);
        case kColTaxName: return tx_copy(w, f.taxStrs + f.tnameOff[tz], f.tnameOff[tz + 1] - f.tnameOff[tz]);
        case kColScore: return tx_put(w, uncl ? 0u : row.score);
        case kColScore2: return tx_put(w, Q.s2);
        case kColHitLen: return tx_put(w, uncl ? 0u : row.hitLen);
        case kColQueryLen: return tx_put(w, Q.qlen);
        case kColNumMatches: return tx_put(w, Q.n ? Q.n : 1u);
        case kColPlaceholder: *w++ = '*'; *w++ = '0'; return w;      // (the reference's switch falls through "" -> "*" -> "0": aln_sink.h:2322-2324)
        case kColZero: *w++ = '0'; return w;
        default: return w + fmt_long_len(f, Q, c);                   // a long column: left to the wavefront
    }
}
// The program of the two passes, a template parameter in two forms.  FmtListCols: a list that came by value.  FmtDefaultCols: the
// default eight, known to the compiler — the passes unroll their column loops for it (kUnroll), so fmt_col_len / fmt_col_put see
// constant codes and their switches are gone; it has no long column, so the write pass's whole-wavefront part is gone as well, and
// none of its columns reads what DTextFmt keeps for the others (taxStrs, trankOff, tnameOff, woff, bases, nmask, qualOff).
struct FmtListCols {
    const TextCols &pc;
    static constexpr uint32_t kUnroll = 1;
    CF_DEV uint32_t nCols() const { return pc.nCols; }
    CF_DEV uint32_t col(uint32_t k) const { return pc.col[k]; }
};
struct FmtDefaultCols {
    static constexpr uint32_t kUnroll = 8;
    static constexpr uint32_t nCols() { return 8; }
    static constexpr uint32_t col(uint32_t k) {
        constexpr uint8_t kDefault[8] = {kColReadId, kColSeqId, kColTaxId, kColScore, kColScore2, kColHitLen, kColQueryLen, kColNumMatches};
        return kDefault[k];
    }
};
template <typename P>
CF_DEV void fmt_rows_size(const DTextFmt &f, const P &p, uint32_t q) {
    if (q >= f.nQueries) return;
    const FmtQuery Q = fmt_query(f, q);
    const bool uncl = Q.n == 0;
    uint32_t total = 0;
    for (uint32_t i = 0; i < (uncl ? 1u : Q.n); i++) {
        const TextRow row = uncl ? TextRow{0, 0, 0, 0} : f.rows[Q.f0 + i];
        total += p.nCols();                                              // the tabs between the columns and the '\n'
#pragma unroll P::kUnroll
        for (uint32_t k = 0; k < p.nCols(); k++) total += fmt_col_len(f, Q, p.col(k), uncl, row);
    }
    f.size[q] = total;
}
// ---- the long fields: every lane of the wavefront calls these with the same arguments (lane: its number).  The field goes to dst, whose
// place in the output is `at` bytes past a dword boundary (dst itself may point into the LDS stage, which keeps that phase): the
// ragged ends byte by byte, the dwords between them whole.
// n bytes from text[src..) — or, text == nullptr, that many 'I'
CF_DEV void fmt_wave_bytes(uint8_t *dst, uint32_t at, const uint8_t *text, uint64_t src, uint32_t n, uint32_t lane) {
    uint32_t head = (4u - (at & 3u)) & 3u;
    if (head > n) head = n;
    const uint32_t mid = (n - head) >> 2, tail = (n - head) & 3u;
    for (uint32_t i = lane; i < head; i += CF_WAVE) dst[i] = text ? text[src + i] : (uint8_t)'I';
    for (uint32_t j = lane; j < mid; j += CF_WAVE) {
        const uint32_t v = text ? (uint32_t)tx_load8(text, src + head + 4 * j) : 0x49494949u;
        __builtin_memcpy(__builtin_assume_aligned(dst + head + 4 * j, 4), &v, 4);
    }
    for (uint32_t i = head + 4 * mid + lane; i < head + 4 * mid + tail; i += CF_WAVE) dst[i] = text ? text[src + i] : (uint8_t)'I';
}
CF_DEV uint32_t tx_letter(uint32_t code, uint32_t isN) { return isN ? (uint32_t)'N' : (0x54474341u >> (8u * code)) & 0xffu; }   // "ACGT"
CF_DEV uint32_t tx_base_at(const uint64_t *w, const uint32_t *m, uint32_t i) {
    return tx_letter((uint32_t)(w[i >> 5] >> (2u * (i & 31u))) & 3u, (m[i >> 5] >> (i & 31u)) & 1u);
}
// four letters from four 2-bit codes (c8) and their four N bits
CF_DEV uint32_t tx_letters4(uint32_t c8, uint32_t m4) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) v |= tx_letter((c8 >> (2u * d)) & 3u, (m4 >> d) & 1u) << (8u * d);
    return v;
}
// the n bases of a read (w, m: its packed words and N masks) as A C G T N: a lane takes 16 bases at a time — one 32-bit stretch of
// the 2-bit codes, expanded in registers into four dwords of letters
CF_DEV void fmt_wave_seq(uint8_t *dst, uint32_t at, const uint64_t *w, const uint32_t *m, uint32_t n, uint32_t lane) {
    uint32_t head = (4u - (at & 3u)) & 3u;
    if (head > n) head = n;
    const uint32_t mid = (n - head) >> 2, tail = (n - head) & 3u;
    for (uint32_t i = lane; i < head; i += CF_WAVE) dst[i] = (uint8_t)tx_base_at(w, m, i);
    for (uint32_t j = lane; 4 * j < mid; j += CF_WAVE) {
        const uint32_t b = head + 16 * j, k = b >> 5, s = b & 31u;
        uint64_t c = w[k] >> (2u * s);
        uint32_t mm = m[k] >> s;
        if (s > 16u && 32u * (k + 1) < n) { c |= w[k + 1] << (64u - 2u * s); mm |= m[k + 1] << (32u - s); }   // (the 16 bases lie in two words)
#pragma unroll
        for (uint32_t d = 0; d < 4; d++)
            if (4 * j + d < mid) {
                const uint32_t v = tx_letters4((uint32_t)(c >> (8u * d)) & 0xffu, (mm >> (4u * d)) & 0xfu);
                __builtin_memcpy(__builtin_assume_aligned(dst + b + 4 * d, 4), &v, 4);
            }
    }
    for (uint32_t i = head + 4 * mid + lane; i < head + 4 * mid + tail; i += CF_WAVE) dst[i] = (uint8_t)tx_base_at(w, m, i);
}
// the long column c of query Q at dst
CF_DEV void fmt_wave_long(const DTextFmt &f, const FmtQuery &Q, uint32_t c, uint8_t *dst, uint32_t at, uint32_t lane) {
    const bool both = c == kColSeq || c == kColQual, second = c == kColSeq2 || c == kColQual2;
    if (second && !f.paired) return;
    for (uint32_t part = second ? 1u : 0u; part < (both && f.paired ? 2u : second ? 2u : 1u); part++) {
        const uint32_t r = Q.ra + part, n = part ? Q.len2 : Q.len1;
        if (part && both) { if (lane == 0) dst[0] = '_'; dst++; at++; }
        if (tx_col_qual(c)) fmt_wave_bytes(dst, at, f.qualOff ? f.text : nullptr, f.qualOff ? f.qualOff[r] : 0u, n, lane);
        else fmt_wave_seq(dst, at, f.bases + f.woff[r], f.nmask + f.woff[r], n, lane);
        dst += n; at += n;
    }
}
template <typename P>
CF_DEV void fmt_rows_write(const DTextFmt &f, const P &p, uint32_t q, uint8_t *lds) {
#ifndef CF_HOST_EMU
    if (!lds) lds = fmt_wave_lds();
#endif
    const bool live = q < f.nQueries;
    uint32_t oneTaxon = 0xffffffffu;                                     // the taxon this query is a perfect single assignment of
    const uint32_t lane = cf_lane(), q0 = q - lane;
    const uint32_t qe = q0 + CF_WAVE < f.nQueries ? q0 + CF_WAVE : f.nQueries;
    const uint64_t segBegin = q0 < f.nQueries ? f.outOff[q0] : 0, segEnd = q0 < f.nQueries ? f.outOff[qe] : 0;
    const uint32_t phase = (uint32_t)(segBegin & 3u);
    const bool viaLds = lds != nullptr && segEnd > segBegin && segEnd - segBegin + phase <= kFmtLds && segEnd <= f.outCap;
    bool anyLong = false;                                                // (the default program: false, known to the compiler)
    for (uint32_t k = 0; k < p.nCols(); k++) anyLong = anyLong || tx_col_long(p.col(k));
    bool printed = false;
    if (live) {
        const FmtQuery Q = fmt_query(f, q);
        const bool uncl = Q.n == 0;
        const uint32_t ms = f.maxScore[q];
        const uint64_t o = f.outOff[q];
        printed = o + f.size[q] <= f.outCap;
        if (printed) {
            uint8_t *w = viaLds ? lds + phase + (uint32_t)(o - segBegin) : f.out + o;
            for (uint32_t i = 0; i < (uncl ? 1u : Q.n); i++) {
                const TextRow row = uncl ? TextRow{0, 0, 0, 0} : f.rows[Q.f0 + i];
#pragma unroll P::kUnroll
                for (uint32_t k = 0; k < p.nCols(); k++) { w = fmt_col_put(f, Q, p.col(k), uncl, row, w); *w++ = k + 1 < p.nCols() ? '\t' : '\n'; }
            }
        }
        // SpeciesMetrics::addSpeciesCounts (aln_sink.h:142-172), the part the per-taxon counters do not hold: only perfect hits feed
        // the EM.  The tally does not depend on the columns
        if (uncl) oneTaxon = f.idxZero;
        else if (Q.n == 1) { const TextRow row = f.rows[Q.f0]; if (ms != 0xffffffffu && row.score >= ms && row.tidx < f.nTaxa) oneTaxon = row.tidx; }
        else {
            bool all = ms != 0xffffffffu;
            for (uint32_t i = 0; i < Q.n && all; i++) { const TextRow row = f.rows[Q.f0 + i]; all = row.score >= ms && row.tidx < f.nTaxa; }
            if (all) {
                const uint32_t at = cf_atomic_add(&f.st->tupleWords, Q.n + 1);
                if (at + Q.n + 1 <= f.tuplesCap) { f.tuples[at] = Q.n; for (uint32_t i = 0; i < Q.n; i++) f.tuples[at + 1 + i] = f.rows[Q.f0 + i].tidx; }
            }
        }
    }
    if (anyLong) {
        // the long fields, query by query: the ballot names the lanes whose rows are being printed; what the field needs — where its
        // letters come from, where they go, how many — is the same for every lane (read again from the leading lane's query)
        uint64_t pend = cf_ballot(printed);
        while (pend) {
            const uint32_t ql = q0 + (uint32_t)cf_ctz64(pend);
            pend &= pend - 1;
            const FmtQuery Q = fmt_query(f, ql);
            const bool uncl = Q.n == 0;
            uint64_t o = f.outOff[ql];
            for (uint32_t i = 0; i < (uncl ? 1u : Q.n); i++) {
                const TextRow row = uncl ? TextRow{0, 0, 0, 0} : f.rows[Q.f0 + i];
                for (uint32_t k = 0; k < p.nCols(); k++) {
                    const uint32_t c = p.col(k), n = fmt_col_len(f, Q, c, uncl, row);
                    if (tx_col_long(c) && n) fmt_wave_long(f, Q, c, viaLds ? lds + phase + (uint32_t)(o - segBegin) : f.out + o, (uint32_t)(o & 3u), lane);
                    o += n + 1;
                }
            }
        }
    }
    if (viaLds) {
        // every lane's bytes are in LDS (the operations of a wavefront on its LDS retire in order; the fence keeps the compiler's
        // hands off the order): out they go, dword j of the stretch by lane j mod 64
        cf_compiler_fence();
        const uint32_t total = phase + (uint32_t)(segEnd - segBegin);
        uint8_t *const dst = f.out + (segBegin - phase);                  // a dword boundary of the output
        for (uint32_t j = lane; 4 * j < total; j += CF_WAVE) {
            const uint32_t lo = 4 * j, hi = lo + 4;
            if (lo >= phase && hi <= total) {
                uint32_t v;
                __builtin_memcpy(&v, lds + lo, 4);
                *reinterpret_cast<uint32_t *>(dst + lo) = v;
            } else
                for (uint32_t k = lo < phase ? phase : lo; k < (hi < total ? hi : total); k++) dst[k] = lds[k];
        }
        cf_compiler_fence();
    }
    // one atomic per taxon and wavefront: the lanes that name the same taxon as the lowest waiting lane are counted by it
    bool waiting = oneTaxon != 0xffffffffu;
    for (;;) {
        const uint64_t w = cf_ballot(waiting);
        if (!w) break;
        const uint32_t lead = cf_shfl(oneTaxon, cf_ctz64(w));
        const uint64_t same = cf_ballot(waiting && oneTaxon == lead);
        if (waiting && oneTaxon == lead) {
            if ((uint32_t)cf_ctz64(same) == cf_lane()) cf_atomic_add(&f.single[lead], (unsigned long long)cf_popc64(same));
            waiting = false;
        }
    }
    if (live && q + 1 == f.nQueries) f.st->outBytes = f.outOff[f.nQueries];
}
// the bodies of the kernels: the default columns (k_fmt_size, k_fmt_write) and a list (k_fmt_cols_size, k_fmt_cols_write)
CF_DEV void fmt_size_body(const DTextFmt &f, uint32_t q) { fmt_rows_size(f, FmtDefaultCols{}, q); }
CF_DEV void fmt_write_body(const DTextFmt &f, uint32_t q, uint8_t *lds = nullptr) { fmt_rows_write(f, FmtDefaultCols{}, q, lds); }
CF_DEV void fmt_cols_size_body(const DTextFmt &f, const TextCols &pc, uint32_t q) { fmt_rows_size(f, FmtListCols{pc}, q); }
CF_DEV void fmt_cols_write_body(const DTextFmt &f, const TextCols &pc, uint32_t q, uint8_t *lds = nullptr) { fmt_rows_write(f, FmtListCols{pc}, q, lds); }

// ---- egress: the reads themselves (--un / --al / --un-conc / --al-conc: the reference's wrapper script has centrifuge-class print
// readSeq and readQual, cuts the two columns off again and writes a FASTQ record per ROW; here the records are made from what the
// batch holds anyway).  A sink is one file's text: 0 unclassified (mates: their first reads), 1 the unclassified pairs' second
// reads, 2 and 3 the same for the classified.  A query writes one record per printed row — max(1, rows) copies of
//   @readID \n bases \n + \n qualities \n
// — into the sinks of its class; an unpaired batch feeds sinks 0 and 2 only, and a class nobody asked for is neither sized nor
// written.  Both mates' records carry the row's readID (mate 1's); bases come from the packed words (trimmed, upper case),
// qualities from the block (FASTA: 'I').  split_size_body, one thread per query, leaves the bytes per sink; behind the exclusive
// sums split_write_body writes them — a record at a time by the WHOLE wavefront (fmt_wave_bytes / fmt_wave_seq: aligned dwords),
// what a lane knows of its own query handed round by shuffles.
enum : uint32_t { kSplitUn = 1u, kSplitAl = 2u, kSplitSinks = 4u };
struct DTextSplit {
    const uint8_t *text;
    const uint32_t *idOff, *idLen, *rlen;
    const uint8_t *qinfo;
    const uint64_t *woff, *bases;
    const uint32_t *nmask, *qualOff;         // qualOff nullptr: FASTA
    uint32_t nQueries, paired, sinks;        // sinks: kSplitUn | kSplitAl
    uint32_t *size[kSplitSinks];             // per query (a sink that is off: nullptr)
    const uint64_t *off[kSplitSinks];        // exclusive sums of size
    uint8_t *out[kSplitSinks];               // dword-aligned
    uint64_t cap[kSplitSinks];
    unsigned long long *nRec;                // [kSplitSinks]: records per sink (added to)
};
CF_DEV bool split_sink_on(const DTextSplit &d, uint32_t s) { return ((d.sinks >> (s >> 1)) & 1u) != 0 && (d.paired || !(s & 1u)); }
CF_DEV void split_size_body(const DTextSplit &d, uint32_t q) {
    const bool live = q < d.nQueries;
    uint32_t cls = 0, copies = 0;
    if (live) {
        const uint32_t n = d.qinfo[q] & 0x3fu, ra = d.paired ? 2 * q : q, idn = d.idLen[ra];
        cls = n ? 1u : 0u; copies = n ? n : 1u;
        for (uint32_t s = 0; s < kSplitSinks; s++)
            if (split_sink_on(d, s)) d.size[s][q] = (s >> 1) == cls ? copies * (1u + idn + 1u + d.rlen[ra + (s & 1u)] + 3u + d.rlen[ra + (s & 1u)] + 1u) : 0u;
    }
    // the records per class: over the wavefront first, one atomic per wavefront and sink
    for (uint32_t c = 0; c < 2; c++) {
        if (!split_sink_on(d, 2 * c)) continue;                          // (the same for every thread of the launch)
        unsigned long long v = live && cls == c ? copies : 0u;
        for (int m = CF_WAVE / 2; m > 0; m >>= 1) v += cf_shfl_xor(v, m);
        if (cf_lane() == 0 && v) { cf_atomic_add(&d.nRec[2 * c], v); if (d.paired) cf_atomic_add(&d.nRec[2 * c + 1], v); }
    }
}
// ... by a selection of taxa instead (--split-taxids): the class is the ROW's — `al` when the taxon its taxID column prints is
// selected (mask: a byte per dense taxon and, at nTaxa, taxID 0's, which the one row of a query without rows prints;
// kreport::splitTaxaMask makes it) —, so a query's max(1, n) records may go a of them to the classified sinks and the others to the
// unclassified ones.  Only the sizes change.  split_write_body needs no word of this: per sink it takes a query's copies from
// size[s][q] alone — its loop `c * rec < size` runs size / rec times, rec being the record's bytes it computes from the same idLen
// and rlen[ra + (s & 1)] as here, never 0 —, asks nothing of qinfo or of a class, and visits every sink that is on for every query;
// the records of a query are the same bytes, so "in row order" holds whichever of them a sink gets.
struct DTextSplitSel {
    const TextRow *rows;                     // the batch's narrow rows and where each query's begin (DTextFmt::rows, rowFirst)
    const uint64_t *rowFirst;
    const uint8_t *mask;                     // [nTaxa + 1]
    uint32_t nTaxa;
};
CF_DEV void split_sel_size_body(const DTextSplit &d, const DTextSplitSel &e, uint32_t q) {
    const bool live = q < d.nQueries;
    uint32_t un = 0, al = 0;                                                  // the query's records per class (a lane past the end: none)
    if (live) {
        const uint32_t n = d.qinfo[q] & 0x3fu, ra = d.paired ? 2 * q : q, idn = d.idLen[ra];
        if (n) {
            const uint64_t f0 = e.rowFirst[q];
            for (uint32_t i = 0; i < n; i++) { const uint32_t t = e.rows[f0 + i].tidx; al += e.mask[t < e.nTaxa ? t : 0u] ? 1u : 0u; }   // (fmt_col_len's t)
            un = n - al;
        } else { al = e.mask[e.nTaxa] ? 1u : 0u; un = 1u - al; }
        for (uint32_t s = 0; s < kSplitSinks; s++)
            if (split_sink_on(d, s)) d.size[s][q] = ((s >> 1) ? al : un) * (1u + idn + 1u + d.rlen[ra + (s & 1u)] + 3u + d.rlen[ra + (s & 1u)] + 1u);
    }
    // the records per class, as split_size_body tallies them: every lane of the wavefront is here
    for (uint32_t c = 0; c < 2; c++) {
        if (!split_sink_on(d, 2 * c)) continue;                          // (the same for every thread of the launch)
        unsigned long long v = c ? al : un;
        for (int m = CF_WAVE / 2; m > 0; m >>= 1) v += cf_shfl_xor(v, m);
        if (cf_lane() == 0 && v) { cf_atomic_add(&d.nRec[2 * c], v); if (d.paired) cf_atomic_add(&d.nRec[2 * c + 1], v); }
    }
}
// one record at dst, whose place in the sink is `at` bytes past a dword boundary: every lane of the wavefront, the same arguments
CF_DEV void split_wave_record(const DTextSplit &d, uint8_t *dst, uint32_t at, uint32_t idOff, uint32_t idn, uint32_t r, uint32_t len, uint32_t lane) {
    const uint64_t wo = d.woff[r];
    const uint32_t qo = d.qualOff ? d.qualOff[r] : 0u;
    const uint32_t pSeq = 1u + idn + 1u, pQual = pSeq + len + 3u;
    if (lane == 0) { dst[0] = '@'; dst[pSeq - 1] = '\n'; dst[pQual + len] = '\n'; }
    for (uint32_t i = lane; i < 3; i += CF_WAVE) dst[pSeq + len + i] = i == 1 ? (uint8_t)'+' : (uint8_t)'\n';
    fmt_wave_bytes(dst + 1, at + 1, d.text, idOff, idn, lane);
    fmt_wave_seq(dst + pSeq, at + pSeq, d.bases + wo, d.nmask + wo, len, lane);
    fmt_wave_bytes(dst + pQual, at + pQual, d.qualOff ? d.text : nullptr, qo, len, lane);
}
CF_DEV void split_write_body(const DTextSplit &d, uint32_t q) {
    const bool live = q < d.nQueries;
    const uint32_t lane = cf_lane(), q0 = q - lane;
    const uint32_t ra = d.paired ? 2 * q : q;
    const uint32_t myId = live ? d.idLen[ra] : 0u, myIdOff = live ? d.idOff[ra] : 0u;
    for (uint32_t s = 0; s < kSplitSinks; s++) {
        if (!split_sink_on(d, s)) continue;                              // (the same for every thread of the launch)
        const uint32_t mySize = live ? d.size[s][q] : 0u, myLen = live ? d.rlen[ra + (s & 1u)] : 0u;
        const uint64_t myOff = live ? d.off[s][q] : 0;
        uint64_t pend = cf_ballot(mySize != 0 && myOff + mySize <= d.cap[s]);
        while (pend) {
            const int l = cf_ctz64(pend);
            pend &= pend - 1;
            const uint32_t size = cf_shfl(mySize, l), len = cf_shfl(myLen, l), idn = cf_shfl(myId, l), idOff = cf_shfl(myIdOff, l);
            const uint64_t o = cf_shfl(myOff, l);
            const uint32_t ql = q0 + (uint32_t)l, r = (d.paired ? 2 * ql : ql) + (s & 1u), rec = 1u + idn + 1u + len + 3u + len + 1u;
            for (uint32_t c = 0; c * rec < size; c++) split_wave_record(d, d.out[s] + o + (uint64_t)c * rec, (uint32_t)((o + (uint64_t)c * rec) & 3u), idOff, idn, r, len, lane);
        }
    }
}

}  // namespace cfamd
