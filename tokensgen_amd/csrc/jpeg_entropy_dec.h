// The entropy decoder of csrc/jpeg_decode.hip as plain inline code that a kernel and a host program both compile: the canonical Huffman table of
// Annex C / F.2.2.3 with an 8-bit look-ahead, a bit reader that never reads at or past `end`, one block, and one restart segment.  No HIP type appears here;
// tests/csrc/jpeg_entropy_host.cpp includes this file under g++ with the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

// the bits of status[f]; the same values as TG_JPEG_ST_* of include/tokensgen_hip.h
enum : int {
    JD_ST_INVALID_CODE = 1,      // no Huffman code matches the next 16 bits, or an AC symbol (run 1..14, size 0) that baseline does not have
    JD_ST_COEF_INDEX = 2,        // a run takes the coefficient index past 63
    JD_ST_CATEGORY = 4,          // a DC category above 11 or an AC size above 10
    JD_ST_OUT_OF_BITS = 8,       // the segment ends before its MCUs do
    JD_ST_RST_COUNT = 16,        // the scan does not hold n_seg - 1 restart markers
    JD_ST_RST_NUMBER = 32,       // a restart marker is not FF D0 + (k mod 8)
    JD_ST_RANGE = 64             // a byte range or a table index that does not lie inside its buffer
};

// maxcode[l]: the largest code of length l (-1: none), valoff[l]: index into vals of the first code of length l minus that code, l = 1 .. 16; maxcode[17] ends every
// search.  look[b]: for the 8 next bits b, length << 8 | symbol of the code they start with, 0 where that code is longer than 8 bits.
struct JdHuffTable {
    int32_t maxcode[18];
    int32_t valoff[18];
    uint16_t look[256];
    uint8_t vals[256];
};
constexpr int JD_TABLE_BYTES = 912;
static_assert(sizeof(JdHuffTable) == JD_TABLE_BYTES, "JdHuffTable is a plain 912-byte record");
constexpr int JD_TABLES_PER_SET = 6;            // component c: DC at 2 c, AC at 2 c + 1

// BITS (codes per length 1 .. 16) and HUFFVAL (n symbols) -> table.  0, or 1: the counts do not add up to n (or n > 256), 2: more codes of some length than that length
// has left (an over-subscribed code).  A refused table is left all zero with maxcode -1: it matches nothing.
JD_HD int jd_build_table(const uint8_t* bits, const uint8_t* vals, int n, JdHuffTable* t) {
    for (int i = 0; i < 18; ++i) {
        t->maxcode[i] = -1;
        t->valoff[i] = 0;
    }
    for (int i = 0; i < 256; ++i) {
        t->look[i] = 0;
        t->vals[i] = 0;
    }
    t->maxcode[17] = 0x7fffffff;
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    if (n < 0 || n > 256 || total != n) return 1;
    int code = 0;
    for (int l = 1; l <= 16; ++l) {             // first the check alone: nothing is written for a refused table
        code += bits[l - 1];
        if (code > (1 << l)) return 2;
        code <<= 1;
    }
    code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = bits[l - 1];
        if (cnt) {
            t->valoff[l] = k - code;
            if (l <= 8)
                for (int i = 0; i < cnt; ++i) {
                    const int first = (code + i) << (8 - l);
                    for (int j = 0; j < (1 << (8 - l)); ++j) t->look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
                }
            k += cnt;
            code += cnt;
            t->maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    for (int i = 0; i < n; ++i) t->vals[i] = vals[i];
    return 0;
}

// Bytes [p, end) of one restart segment: entropy data in which FF 00 stands for FF.  An FF followed by anything else (fill before a marker, a marker, the end) ends the
// data.  acc holds the n next bits in its low end.
struct JdBitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint32_t acc;
    int n;
    int err;
};

JD_HD void jd_fill(JdBitReader& br) {
    while (br.n <= 24 && br.p < br.end) {
        const uint32_t b = *br.p++;
        if (b == 0xffu) {
            if (br.p < br.end && *br.p == 0) {
                ++br.p;
            } else {
                br.p = br.end;
                break;
            }
        }
        br.acc = (br.acc << 8) | b;
        br.n += 8;
    }
}

// the next 16 bits, zeros past the end of the data
JD_HD uint32_t jd_peek16(const JdBitReader& br) { return (br.n >= 16 ? br.acc >> (br.n - 16) : br.acc << (16 - br.n)) & 0xffffu; }

// one Huffman symbol, or -1 with br.err set
JD_HD int jd_symbol(JdBitReader& br, const JdHuffTable* t) {
    jd_fill(br);
    const uint32_t w = jd_peek16(br);
    int len, sym;
    const uint32_t e = t->look[w >> 8];
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255u);
    } else {
        len = 9;
        while (len <= 16 && (int32_t)(w >> (16 - len)) > t->maxcode[len]) ++len;
        if (len > 16) {
            br.err |= JD_ST_INVALID_CODE;
            return -1;
        }
        sym = t->vals[((int32_t)(w >> (16 - len)) + t->valoff[len]) & 255];
    }
    if (len > br.n) {
        br.err |= JD_ST_OUT_OF_BITS;
        return -1;
    }
    br.n -= len;
    return sym;
}

// the value of the next s bits (1 <= s <= 16) by the EXTEND rule of F.2.2.1; 0 with br.err set where the data ends first
JD_HD int jd_receive_extend(JdBitReader& br, int s) {
    jd_fill(br);
    if (s > br.n) {
        br.err |= JD_ST_OUT_OF_BITS;
        return 0;
    }
    const int v = (int)((br.acc >> (br.n - s)) & ((1u << s) - 1u));
    br.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

JD_HD void jd_zero_block(int16_t* out) {        // 64 coefficients; out is 16-byte aligned
    uint64_t* q = (uint64_t*)out;
    for (int i = 0; i < 16; ++i) q[i] = 0;
}

// One block: `out` receives all 64 coefficients in zigzag order, zeros first and the non-zero ones after, so no private array is indexed by a run-time value.  pred is
// the component's running DC (int32; stored clamped to int16).  At most 64 symbol steps: every step moves k forward or ends the block.  Returns 0, or the status bits
// with the block all zero.
JD_HD int jd_decode_block(JdBitReader& br, const JdHuffTable* dc, const JdHuffTable* ac, int32_t& pred, int16_t* out) {
    jd_zero_block(out);
    int s = jd_symbol(br, dc);
    if (s >= 0 && s > 11) br.err |= JD_ST_CATEGORY;
    if (br.err) return br.err;
    if (s) pred += jd_receive_extend(br, s);
    if (br.err) return br.err;
    out[0] = (int16_t)(pred < -32768 ? -32768 : pred > 32767 ? 32767 : pred);
    int k = 1;
    while (k < 64) {
        const int rs = jd_symbol(br, ac);
        if (rs < 0) break;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r == 0) break;                  // end of block
            if (r != 15) {
                br.err |= JD_ST_INVALID_CODE;
                break;
            }
            k += 16;
            if (k > 64) br.err |= JD_ST_COEF_INDEX;
            continue;
        }
        if (s > 10) {
            br.err |= JD_ST_CATEGORY;
            break;
        }
        k += r;
        if (k > 63) {
            br.err |= JD_ST_COEF_INDEX;
            break;
        }
        const int v = jd_receive_extend(br, s);
        if (br.err) break;
        out[k++] = (int16_t)v;
    }
    if (br.err) jd_zero_block(out);
    return br.err;
}

// MCUs of one restart segment: n_mcus x bpm blocks into out (bpm 6: Y Y Y Y Cb Cr, bpm 3: Y Cb Cr), DC prediction from 0.  tabs: the frame's six tables.  After the
// first error every later block of the segment is zero.  Returns the status bits.
JD_HD int jd_decode_segment(const uint8_t* begin, const uint8_t* end, const JdHuffTable* tabs, int bpm, long n_mcus, int16_t* out) {
    JdBitReader br;
    br.p = begin;
    br.end = end;
    br.acc = 0;
    br.n = 0;
    br.err = 0;
    int32_t pred0 = 0, pred1 = 0, pred2 = 0;
    for (long m = 0; m < n_mcus; ++m) {
        for (int k = 0; k < bpm; ++k, out += 64) {
            if (br.err) {
                jd_zero_block(out);
                continue;
            }
            const int comp = k < bpm - 2 ? 0 : k - (bpm - 3);
            int32_t pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
            jd_decode_block(br, tabs + 2 * comp, tabs + 2 * comp + 1, pred, out);
            pred0 = comp == 0 ? pred : pred0;
            pred1 = comp == 1 ? pred : pred1;
            pred2 = comp == 2 ? pred : pred2;
        }
    }
    return br.err;
}
