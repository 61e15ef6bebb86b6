// pjd_lut_build.h -- construction of the two-level decode tables (layout: pjd_internal.h, PjdDevTset), ONE text for the device
// (pjd_k_build_tables, pjd_k_huffman.hip) and the host (the planner's geometry, pjd_plan.cpp; pjd_plan_luts, pjd_api.hip).
#pragma once
#include "pjd_internal.h"

#define PJD_LUT_BAD  PJD_LUT_ENTRY(16u, 1u, false, PJD_LUT_BADSYM)    // no code: consume 16 bits (as the reference's get_next_symbol)

// The first code of every length (reference generate_codes, jpeg_scanner.cpp:438-448): first[1..16]; first[0] = 0.
// Returns false for an over-subscribed table (not a prefix code).  *end9 / *end16: one past the last code of at most 9 / 16 bits,
// at that length.
static inline __host__ __device__ bool pjd_lut_first_codes(const PjdDevHuffRaw &q, uint32_t *first, uint32_t *end9 = nullptr, uint32_t *end16 = nullptr)
{
    bool ok = true;
    uint32_t code = 0;
    first[0] = 0;
    for (int len = 1; len <= 16; len++) {
        const uint32_t cnt = (uint32_t)q.offsets[len] - q.offsets[len - 1];
        first[len] = code;
        if (code + cnt > (1u << len)) ok = false;
        if (len == PJD_LUT_BITS && end9) *end9 = code + cnt;
        if (len == 16 && end16) *end16 = code + cnt;
        code = (code + cnt) << 1;
    }
    return ok;
}

// Second-level geometry of ONE decode table.  The prefixes [p0, p1) start codes longer than 9 bits (canonical codes keep them in one
// range); the table of prefix P has 2^k(P) entries, 9 + k(P) the longest code under P, and k does not fall as P rises: cp[k - 1] is
// the first prefix of class k = 1..7 (cp[0] == p0; an empty class has cp[k - 1] == cp[k]; a prefix with no code under it lands in
// class 1).  Returns false, with an empty range, for a table that is not a prefix code.
static inline __host__ __device__ bool pjd_lut_geometry(const PjdDevHuffRaw &r, uint16_t *cp /* [PJD_L2_BITS] */, uint16_t &p1_out)
{
    uint32_t first[17], end9 = 0, end16 = 0;
    const bool ok = pjd_lut_first_codes(r, first, &end9, &end16);
    const uint32_t np = 1u << PJD_LUT_BITS;
    uint32_t p0 = end9 < np ? end9 : np, p1 = (end16 + (1u << PJD_L2_BITS) - 1) >> PJD_L2_BITS;
    if (p1 > np) p1 = np;
    if (p1 < p0 || !ok) p1 = p0;
    uint32_t nxt = p1;                                  // first prefix that starts a code of this length or a longer one
    for (int len = 16; len > PJD_LUT_BITS; len--) {
        if (r.offsets[len] != r.offsets[len - 1]) {
            const uint32_t fp = first[len] >> (len - PJD_LUT_BITS);
            if (fp < nxt) nxt = fp;
        }
        if (nxt < p0) nxt = p0;
        cp[len - PJD_LUT_BITS - 1] = (uint16_t)nxt;
    }
    cp[0] = (uint16_t)p0;
    p1_out = (uint16_t)p1;
    return ok;
}

// u16 entries of the table's second-level region, and (ce, optional) the first entry of every class when the region starts at `off`
static inline __host__ __device__ uint32_t pjd_lut_l2_entries(const uint16_t *cp, uint32_t p1, uint32_t off = 0, uint16_t *ce = nullptr)
{
    uint32_t n = off;
    for (uint32_t k = 1; k <= PJD_L2_BITS; k++) {
        if (ce) ce[k - 1] = (uint16_t)n;
        n += ((k < PJD_L2_BITS ? (uint32_t)cp[k] : p1) - cp[k - 1]) << k;
    }
    return n - off;
}

// the 16-bit entry of symbol `sym` with a code of `len` bits
static inline __host__ __device__ uint32_t pjd_lut_symbol_entry(uint32_t len, uint32_t sym, bool is_ac)
{
    uint32_t run = 0, size, bad = 0;
    bool eob = false;
    if (sym == 0xFF) bad = PJD_LUT_BADSYM;                              // the reference reads a returned 0xFF as "no symbol" (jpeg_scanner.cpp:470,490)
    if (is_ac) {
        run = sym >> 4; size = sym & 15u;
        if (sym == 0) eob = true;
        else if (size > 10 && !bad) bad = PJD_LUT_BADLEN;               // jpeg_scanner.cpp:506
    } else {
        size = sym;
        if (sym > 11 && !bad) bad = PJD_LUT_BADLEN;                     // jpeg_scanner.cpp:474
    }
    return PJD_LUT_ENTRY(len + (bad ? 0u : size), eob ? 32u : run + 1, eob, bad ? bad : size);   // EOB: 32 + 64 = 96 slots (pjd_internal.h)
}

// the symbol whose code is the leading bits of `bits` (`nbits` of them are known), among the codes of lo..hi bits; 0 if none is
// determined by them.  Shortest match wins, as the reference's scan.  first: pjd_lut_first_codes of q
static inline __host__ __device__ uint32_t pjd_lut_match(const PjdDevHuffRaw &q, const uint32_t *first, bool ac, uint32_t bits, uint32_t nbits, uint32_t lo, uint32_t hi)
{
    for (uint32_t len = lo; len <= hi && len <= nbits; len++) {
        const uint32_t c = bits >> (nbits - len);
        const uint32_t d = c - first[len], cnt = (uint32_t)q.offsets[len] - q.offsets[len - 1];
        if (c >= first[len] && d < cnt) return pjd_lut_symbol_entry(len, q.symbols[q.offsets[len - 1] + d], ac);
    }
    return 0u;
}

// First-level entry `idx` (32 bits) of table r.  cp, ce, p1: the table's second-level geometry (PjdDevTset).  r2 / first2: the table
// the SECOND symbol of a pair is decoded with (r itself for an AC table, the AC table of the components that use this DC table),
// or null: no pairs.
static inline __host__ __device__ uint32_t pjd_lut_l1_entry(const PjdDevHuffRaw &r, const uint32_t *first, const PjdDevHuffRaw *r2, const uint32_t *first2,
                                                            const uint16_t *cp, const uint16_t *ce, uint32_t p1, uint32_t idx)
{
    const bool is_ac = r.is_ac != 0;
    const uint32_t m = pjd_lut_match(r, first, is_ac, idx, PJD_LUT_BITS, 1, PJD_LUT_BITS);
    if (!m && idx >= cp[0] && idx < p1) {
        // pointer entry: bits 4..0 == 0; bits 9..5 = 32 - k, the right shift that leaves the top k of the seven bits behind the prefix
        // (of the window moved up by the prefix); high half = byte offset, relative to the blob, of the prefix's 2^k-entry table
        uint32_t k = 1;
        while (k < PJD_L2_BITS && idx >= cp[k]) k++;
        return ((32u - k) << 5) | ((2u * (ce[k - 1] + ((idx - cp[k - 1]) << k))) << 16);
    }
    const uint32_t e = m ? m : PJD_LUT_BAD;
    // the pair: this symbol whole inside the 9 bits, a valid run/size (or DC) symbol, and the bits after it determine the next code
    uint32_t pair = 0;
    if (r2 && m && !(m & PJD_LUT_EOB) && PJD_LUT_SIZE(m) < PJD_LUT_BADSYM && PJD_LUT_USED(m) < PJD_LUT_BITS) {
        const uint32_t rest = PJD_LUT_BITS - PJD_LUT_USED(m);
        const uint32_t m2 = pjd_lut_match(*r2, first2, true, idx & ((1u << rest) - 1u), rest, 1, rest);
        if (m2 && PJD_LUT_SIZE(m2) < PJD_LUT_BADSYM && PJD_LUT_USED(m) + PJD_LUT_USED(m2) <= 31u)
            pair = (PJD_LUT_USED(m) + PJD_LUT_USED(m2)) | ((PJD_LUT_ADV(m) + PJD_LUT_ADV(m2)) << 5) | (PJD_LUT_SIZE(m2) << 12);   // size 2: bits 31..28 of the entry
    }
    // no pair: the pair field repeats the symbol's own used / advance (a "pair" that is the symbol alone), so the state-only
    // passes need not ask whether there is one; the write pass tells a real pair by used12 != used
    if (!pair) pair = e & 0xfffu;
    return (e & 0xffffu) | (pair << 16);
}

// Entry j of the table's second-level region (j < pjd_lut_l2_entries): the region is the tables of the prefixes cp[0] .. p1 - 1 one
// after the other; the entry at index i of prefix P's table stands for the 9 + k bits (P << k) | i
static inline __host__ __device__ uint32_t pjd_lut_l2_entry(const PjdDevHuffRaw &r, const uint32_t *first, const uint16_t *cp, const uint16_t *ce, uint32_t j)
{
    uint32_t k = 1;
    while (k < PJD_L2_BITS && ce[0] + j >= ce[k]) k++;
    const uint32_t q = ce[0] + j - ce[k - 1];
    const uint32_t bits = ((cp[k - 1] + (q >> k)) << k) | (q & ((1u << k) - 1u));
    const uint32_t m = pjd_lut_match(r, first, r.is_ac != 0, bits, PJD_LUT_BITS + k, PJD_LUT_BITS + 1, PJD_LUT_BITS + k);
    return m ? m : PJD_LUT_BAD;
}
