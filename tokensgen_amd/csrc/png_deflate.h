// The deflate side of csrc/png.hip as plain inline code that a kernel and a host program both compile: what a run of equal bytes becomes, the
// length-limited Huffman code lengths, the canonical codes, the header of a dynamic block, CRC-32 and Adler-32 arithmetic, and a serial coder of one band that puts the
// pieces together in the order of the definition (include/tokensgen_hip.h; tests/png_ref.py restates it).  No HIP type appears here; tests/csrc/png_deflate_host.cpp
// includes this file under g++ with the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PD_HD __host__ __device__ __forceinline__
#else
#define PD_HD inline
#endif

constexpr int PD_LL_SYMBOLS = 286;              // literals, end of block (256), lengths (257 .. 285)
constexpr int PD_CL_SYMBOLS = 19;
constexpr int PD_MAX_BAND = 65535;              // bytes of a band: one stored block, 16-bit counters
constexpr int PD_MAX_MATCH = 258;
constexpr int PD_EOB = 256;

// ---- a run of L equal bytes: `lits` literals (the first byte, and a remainder of 1 or 2), n258 matches of 258 at distance 1, one more match of `rem` (3 .. 257, or 0)
PD_HD void pd_run_split(int L, int& lits, int& n258, int& rem) {
    const int rest = L - 1;
    n258 = rest / PD_MAX_MATCH;
    const int r = rest - n258 * PD_MAX_MATCH;
    rem = r >= 3 ? r : 0;
    lits = r >= 3 ? 1 : 1 + r;
}

// a match length 3 .. 258 -> its literal/length symbol, the number of extra bits and their value
PD_HD void pd_length_symbol(int n, int& sym, int& eb, int& ev) {
    const int l = n - 3;
    if (l < 8) {
        sym = 257 + l;
        eb = ev = 0;
    } else if (l == 255) {
        sym = 285;
        eb = ev = 0;
    } else {
        int k = 3;
        while ((l >> (k + 1)) != 0) ++k;        // floor(log2 l), 3 .. 7
        eb = k - 2;
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        ev = l & ((1 << eb) - 1);
    }
}

// the run's share of the histogram; `add(symbol, count)`
template <class F>
PD_HD void pd_run_count(int v, int L, F&& add) {
    int lits, n258, rem;
    pd_run_split(L, lits, n258, rem);
    add(v, lits);
    if (n258) add(285, n258);
    if (rem) {
        int sym, eb, ev;
        pd_length_symbol(rem, sym, eb, ev);
        add(sym, 1);
    }
}

// the run's bits under the literal/length lengths `ll` (a match: its code, the extra bits, one bit of the distance code)
PD_HD uint32_t pd_run_bits(int v, int L, const uint8_t* ll) {
    int lits, n258, rem;
    pd_run_split(L, lits, n258, rem);
    uint32_t bits = (uint32_t)lits * ll[v] + (uint32_t)n258 * (ll[285] + 1u);
    if (rem) {
        int sym, eb, ev;
        pd_length_symbol(rem, sym, eb, ev);
        bits += ll[sym] + (uint32_t)eb + 1u;
    }
    return bits;
}

// the run's tokens in order: the literal, the matches of 258, then the remainder as a match or as literals.  sink.put(value, bits), least significant bit first.
template <class Sink>
PD_HD void pd_run_emit(int v, int L, const uint8_t* ll, const uint16_t* code, Sink& sink) {
    int lits, n258, rem;
    pd_run_split(L, lits, n258, rem);
    sink.put(code[v], ll[v]);
    for (int i = 0; i < n258; ++i) sink.put(code[285], ll[285] + 1);           // the distance code's one bit is 0: it rides on top of the length code
    if (rem) {
        int sym, eb, ev;
        pd_length_symbol(rem, sym, eb, ev);
        sink.put((uint32_t)code[sym] | (uint32_t)ev << ll[sym], ll[sym] + eb + 1);
    }
    for (int i = 1; i < lits; ++i) sink.put(code[v], ll[v]);
}

// ---- code lengths -------------------------------------------------------------------------------------------------------------------------------------------------
struct PdTree {                                 // scratch of pd_lengths_sorted: leaves 0 .. m - 1 in sorted order, internal nodes after them
    uint32_t weight[2 * PD_LL_SYMBOLS];
    uint16_t parent[2 * PD_LL_SYMBOLS];
    uint16_t depth[2 * PD_LL_SYMBOLS];
};

// the symbols with a count, ascending by (count, symbol), into order[]; returns how many.  Insertion sort: the host, and the 19 symbols of the code-length alphabet.
PD_HD int pd_sort_symbols(const uint32_t* counts, int n, uint16_t* order) {
    int m = 0;
    for (int s = 0; s < n; ++s) {
        if (counts[s] == 0) continue;
        int i = m++;
        for (; i > 0 && counts[order[i - 1]] > counts[s]; --i) order[i] = order[i - 1];    // equal counts keep the symbol order
        order[i] = (uint16_t)s;
    }
    return m;
}

// lens[0 .. n) from the m sorted symbols: a two-queue Huffman tree (of two equal weights the leaf goes first), depths past max_len cut to it and the excess of the Kraft
// sum repaid by the step of zlib's gen_bitlen, and the sorted symbols take the lengths from the longest to the shortest.  One symbol alone: length 1.
PD_HD void pd_lengths_sorted(const uint32_t* counts, const uint16_t* order, int m, int n, int max_len, uint8_t* lens, PdTree* t) {
    for (int s = 0; s < n; ++s) lens[s] = 0;
    if (m == 0) return;
    if (m == 1) {
        lens[order[0]] = 1;
        return;
    }
    for (int i = 0; i < m; ++i) t->weight[i] = counts[order[i]];
    int leaf = 0, node = m;
    for (int fresh = m; fresh < 2 * m - 1; ++fresh) {
        uint32_t w = 0;
        for (int k = 0; k < 2; ++k) {
            int pick;
            if (leaf < m && (node >= fresh || t->weight[leaf] <= t->weight[node])) pick = leaf++;
            else pick = node++;
            t->parent[pick] = (uint16_t)fresh;
            w += t->weight[pick];
        }
        t->weight[fresh] = w;
    }
    t->depth[2 * m - 2] = 0;
    for (int i = 2 * m - 3; i >= 0; --i) t->depth[i] = (uint16_t)(t->depth[t->parent[i]] + 1);
    int bl[16];
    for (int b = 0; b < 16; ++b) bl[b] = 0;
    for (int i = 0; i < m; ++i) {
        const int d = t->depth[i];
        ++bl[d > max_len ? max_len : d];
    }
    // the Kraft sum in units of 2^-max_len: cutting the deep leaves to max_len took it past 1.  Every step below repays exactly one unit, and the level max_len holds
    // more leaves than units are owed (the cut leaves of a subtree rooted at depth max_len are one more than its excess), so the steps never run out of leaves.
    long kraft = 0;
    for (int b = 1; b <= max_len; ++b) kraft += (long)bl[b] << (max_len - b);
    for (long excess = kraft - (1L << max_len); excess > 0; --excess) {
        int bits = max_len - 1;
        while (bl[bits] == 0) --bits;
        --bl[bits];
        bl[bits + 1] += 2;
        --bl[max_len];
    }
    int i = 0;
    for (int bits = max_len; bits >= 1; --bits)
        for (int k = 0; k < bl[bits]; ++k) lens[order[i++]] = (uint8_t)bits;
}

// RFC 1951 3.2.2, each code reversed: the stream takes a Huffman code from its most significant bit
PD_HD void pd_canonical_codes(const uint8_t* lens, int n, int max_len, uint16_t* code) {
    int bl[17], next[17];
    for (int b = 0; b < 17; ++b) bl[b] = 0;
    for (int s = 0; s < n; ++s) ++bl[lens[s]];
    bl[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int b = 1; b <= max_len; ++b) {
        c = (c + bl[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        uint32_t v = l ? (uint32_t)next[l]++ : 0u, r = 0;
        for (int b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1 - b);
        code[s] = (uint16_t)r;
    }
}

// ---- the header of a dynamic block ----------------------------------------------------------------------------------------------------------------------------------
PD_HD int pd_hlit(const uint8_t* ll) {         // literal/length codes sent: up to the last used symbol, at least 257 (the end of block is always used)
    int h = PD_LL_SYMBOLS;
    while (h > 257 && ll[h - 1] == 0) --h;
    return h;
}

// the code-length sequence (ll[0 .. hlit) and the distance code's single length 1, as ONE sequence) in the code-length alphabet: f(symbol, extra bits, their value).
// r zeros: 18 (up to 138) while r >= 11, then 17 if r >= 3, then single zeros; r equal lengths: the length, 16 (up to 6) while r >= 3 remain, then the length again.
template <class F>
PD_HD void pd_cl_symbols(const uint8_t* ll, int hlit, F&& f) {
    const int n = hlit + 1;
    int i = 0;
    while (i < n) {
        const int v = i < hlit ? ll[i] : 1;
        int r = 1;
        while (i + r < n && (i + r < hlit ? ll[i + r] : 1) == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) {
                const int k = r < 138 ? r : 138;
                f(18, 7, k - 11);
                r -= k;
            }
            if (r >= 3) {
                f(17, 3, r - 3);
                r = 0;
            }
            for (; r > 0; --r) f(0, 0, 0);
        } else {
            f(v, 0, 0);
            --r;
            while (r >= 3) {
                const int k = r < 6 ? r : 6;
                f(16, 2, k - 3);
                r -= k;
            }
            for (; r > 0; --r) f(v, 0, 0);
        }
    }
}

PD_HD int pd_cl_order(int i) {
    const uint8_t order[PD_CL_SYMBOLS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// the code-length code of a block: cl[19] from the histogram of pd_cl_symbols
PD_HD void pd_cl_lengths(const uint8_t* ll, uint8_t* cl, PdTree* t) {
    uint32_t counts[PD_CL_SYMBOLS];
    uint16_t order[PD_CL_SYMBOLS];
    for (int s = 0; s < PD_CL_SYMBOLS; ++s) counts[s] = 0;
    pd_cl_symbols(ll, pd_hlit(ll), [&](int s, int, int) { ++counts[s]; });
    const int m = pd_sort_symbols(counts, PD_CL_SYMBOLS, order);
    pd_lengths_sorted(counts, order, m, PD_CL_SYMBOLS, 7, cl, t);
}

PD_HD int pd_hclen(const uint8_t* cl) {
    int h = PD_CL_SYMBOLS;
    while (h > 4 && cl[pd_cl_order(h - 1)] == 0) --h;
    return h;
}

// BFINAL 0, BTYPE 10, HLIT, HDIST 0, HCLEN, the code-length code's lengths, the coded sequence
PD_HD uint32_t pd_header_bits(const uint8_t* ll, const uint8_t* cl) {
    uint32_t bits = 17 + 3 * (uint32_t)pd_hclen(cl);
    pd_cl_symbols(ll, pd_hlit(ll), [&](int s, int eb, int) { bits += cl[s] + (uint32_t)eb; });
    return bits;
}

template <class Sink>
PD_HD void pd_header_emit(const uint8_t* ll, const uint8_t* cl, Sink& sink) {
    uint16_t cl_code[PD_CL_SYMBOLS];
    pd_canonical_codes(cl, PD_CL_SYMBOLS, 7, cl_code);
    const int hlit = pd_hlit(ll), hclen = pd_hclen(cl);
    sink.put(0, 1);
    sink.put(2, 2);
    sink.put((uint32_t)(hlit - 257), 5);
    sink.put(0, 5);
    sink.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) sink.put(cl[pd_cl_order(i)], 3);
    pd_cl_symbols(ll, hlit, [&](int s, int eb, int ev) { sink.put((uint32_t)cl_code[s] | (uint32_t)ev << cl[s], cl[s] + eb); });
}

// the bytes of the dynamic form from the bits of header and tokens: the end of block, the empty stored block's three bits, the padding, 00 00 FF FF
PD_HD uint32_t pd_dynamic_bytes(uint32_t header_bits, uint32_t token_bits, const uint8_t* ll) { return (header_bits + token_bits + ll[PD_EOB] + 3 + 7) / 8 + 4; }
PD_HD uint32_t pd_stored_bytes(int n) { return 5u + (uint32_t)n; }

// ---- checksums -----------------------------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t PD_CRC_POLY = 0xedb88320u;

PD_HD uint32_t pd_crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ PD_CRC_POLY : i >> 1;
    return i;
}

// CRC-32 of n bytes continued from `crc` (0 at the start), without a table
PD_HD uint32_t pd_crc32(uint32_t crc, const uint8_t* p, long n) {
    crc = ~crc;
    for (long i = 0; i < n; ++i) crc = pd_crc_table_entry((crc ^ p[i]) & 255u) ^ (crc >> 8);
    return ~crc;
}

// a(x) b(x) mod the CRC polynomial, bit-reflected (bit 31 is x^0): zlib's multmodp
PD_HD uint32_t pd_crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ PD_CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 n) mod the polynomial; crc(A || B) = pd_crc_mulmod(pd_crc_shift(|B|), crc(A)) ^ crc(B)
PD_HD uint32_t pd_crc_shift(uint32_t n) {
    uint32_t p = 1u << 31, sq = 1u << 23;       // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1u) p = pd_crc_mulmod(sq, p);
        sq = pd_crc_mulmod(sq, sq);
    }
    return p;
}

constexpr uint32_t PD_ADLER_MOD = 65521u;

// the Adler pair of n <= 65535 bytes from sum = Σ d[i] and weighted = Σ (n - i) d[i]: A = 1 + sum, B = n + weighted (mod 65521)
PD_HD void pd_adler_pair(uint64_t sum, uint64_t weighted, uint32_t n, uint32_t& A, uint32_t& B) {
    A = (uint32_t)((1u + sum) % PD_ADLER_MOD);
    B = (uint32_t)((n + weighted) % PD_ADLER_MOD);
}

// (A1, B1) of a prefix and (A2, B2) of the n2 bytes after it -> the pair of both
PD_HD void pd_adler_combine(uint32_t& A1, uint32_t& B1, uint32_t A2, uint32_t B2, uint32_t n2) {
    const uint64_t a = (uint64_t)A1 + A2 + PD_ADLER_MOD - 1u;
    const uint64_t b = (uint64_t)B1 + B2 + (uint64_t)(n2 % PD_ADLER_MOD) * ((A1 + PD_ADLER_MOD - 1u) % PD_ADLER_MOD);
    A1 = (uint32_t)(a % PD_ADLER_MOD);
    B1 = (uint32_t)(b % PD_ADLER_MOD);
}

// ---- one band, serially: the order of the definition, for the host program (the kernels run the same pieces per lane and per run) -------------------------------------
struct PdByteSink {                             // least significant bit first into out[0 .. cap); bytes past cap are counted, not stored
    uint8_t* out;
    long cap, bytes;
    uint64_t acc;
    int n;
    PD_HD void put(uint32_t value, int bits) {
        acc |= (uint64_t)value << n;
        n += bits;
        while (n >= 8) {
            if (bytes < cap) out[bytes] = (uint8_t)acc;
            ++bytes;
            acc >>= 8;
            n -= 8;
        }
    }
    PD_HD void pad() {
        if (n) put(0, 8 - n);
    }
};

struct PdBandPlan {
    uint8_t ll[PD_LL_SYMBOLS + 2];
    uint8_t cl[PD_CL_SYMBOLS + 1];
    uint32_t header_bits, token_bits, dynamic_bytes, stored;
};

// f(value, length) for every maximal run of d[0 .. n)
template <class F>
PD_HD void pd_for_runs(const uint8_t* d, int n, F&& f) {
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && d[j] == d[i]) ++j;
        f((int)d[i], j - i);
        i = j;
    }
}

PD_HD void pd_band_plan(const uint8_t* d, int n, PdBandPlan* plan, PdTree* t) {
    uint32_t counts[PD_LL_SYMBOLS];
    uint16_t order[PD_LL_SYMBOLS];
    for (int s = 0; s < PD_LL_SYMBOLS; ++s) counts[s] = 0;
    counts[PD_EOB] = 1;
    pd_for_runs(d, n, [&](int v, int L) { pd_run_count(v, L, [&](int s, int c) { counts[s] += (uint32_t)c; }); });
    const int m = pd_sort_symbols(counts, PD_LL_SYMBOLS, order);
    pd_lengths_sorted(counts, order, m, PD_LL_SYMBOLS, 15, plan->ll, t);
    pd_cl_lengths(plan->ll, plan->cl, t);
    plan->header_bits = pd_header_bits(plan->ll, plan->cl);
    uint32_t bits = 0;
    pd_for_runs(d, n, [&](int v, int L) { bits += pd_run_bits(v, L, plan->ll); });
    plan->token_bits = bits;
    plan->dynamic_bytes = pd_dynamic_bytes(plan->header_bits, bits, plan->ll);
    plan->stored = plan->dynamic_bytes >= pd_stored_bytes(n);
}

// the band's deflate bytes into out[0 .. cap); returns their number (the dynamic block and the empty stored block, or one stored block)
PD_HD long pd_band_write(const uint8_t* d, int n, const PdBandPlan* plan, uint8_t* out, long cap) {
    PdByteSink sink = {out, cap, 0, 0, 0};
    if (plan->stored) {
        sink.put(0, 8);
        sink.put((uint32_t)n, 16);
        sink.put((uint32_t)n ^ 0xffffu, 16);
        for (int i = 0; i < n; ++i) sink.put(d[i], 8);
        return sink.bytes;
    }
    uint16_t code[PD_LL_SYMBOLS];
    pd_canonical_codes(plan->ll, PD_LL_SYMBOLS, 15, code);
    pd_header_emit(plan->ll, plan->cl, sink);
    pd_for_runs(d, n, [&](int v, int L) { pd_run_emit(v, L, plan->ll, code, sink); });
    sink.put(code[PD_EOB], plan->ll[PD_EOB]);
    sink.put(0, 3);
    sink.pad();
    sink.put(0xffff0000u, 32);
    return sink.bytes;
}
