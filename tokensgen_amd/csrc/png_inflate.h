// The inflate side of csrc/png_decode.hip as plain inline code that a kernel and a host program both compile: a bounds-checked bit reader, the
// validation of a block's code lengths and its decoding tables, a serial decoder of one raw deflate range into an output range, the five filter inverses and the
// Adler-32 of what was produced.  The definition is the comment of include/tokensgen_hip.h; tests/png_dec_ref.py restates it.  No HIP type appears here;
// tests/csrc/png_inflate_host.cpp includes this file under g++ with the address and undefined-behaviour sanitizers, and the kernels run the very same functions.
//
// The input is untrusted.  Every read of `data` lies inside the piece's range [begin, end), which the caller has checked against [0, data_bytes); every store lies
// inside [0, cap) of the frame's filtered area and inside the 64 KiB ring; every loop is bounded by the bits consumed or the bytes produced, and a symbol consumes
// at least one bit.  An error is a bit of the returned status and ends the decoding of the piece.
//
// One decoder for one lane and for many: the template parameter C says how many lanes run the function together (C::lanes()), which one this is (C::lane()) and how
// they meet (C::sync(), C::sum()).  All lanes follow the same symbols, so every branch is uniform; the lane id only spreads the bytes of a stored block or a match and
// picks the one lane that stores a literal or builds a table.  PiSerial is the host: one lane, nothing to meet.
#pragma once
#include <stdint.h>

#include "png_deflate.h"

constexpr int PI_BAD_BLOCK = 1;                 // block type 3, or a stored block whose LEN is not ~NLEN
constexpr int PI_BAD_LENGTHS = 2;               // code lengths that are no code (pi_build_*), more than 286 / 30 symbols, a repeat with nothing before it or past the end
constexpr int PI_BAD_SYMBOL = 4;                // a bit pattern that is no code, a length symbol 286 / 287, a distance symbol 30 / 31
constexpr int PI_BAD_DISTANCE = 8;              // a distance that reaches before the first byte of the frame's output
constexpr int PI_TRUNCATED = 16;                // the input ends inside a block
constexpr int PI_BAD_SIZE = 32;                 // the output is not exactly cap bytes, or the stream does not end where its range ends
constexpr int PI_BAD_ADLER = 64;
constexpr int PI_BAD_FILTER = 128;              // a filter type above 4
constexpr int PI_NOT_INDEPENDENT = 256;         // chunk mode: the piece is not a stream of whole blocks of its own; a verdict, not an error
constexpr int PI_BAD_RANGE = 512;               // a byte range or an index outside its buffer

constexpr int PI_STREAM = 0, PI_CHUNK_SIZE = 1, PI_CHUNK_WRITE = 2;            // the modes of pi_inflate
constexpr int PI_RING = 65536;                  // bytes of the output ring: a power of two, at least 32768 + 258
constexpr int PI_FAST_BITS = 10;

struct PiSerial {
    static PD_HD int lane() { return 0; }
    static PD_HD int lanes() { return 1; }
    static PD_HD void sync() {}
    static PD_HD uint64_t sum(uint64_t v) { return v; }
};

// one prefix code: the first-level table over PI_FAST_BITS bits of the stream (symbol << 4 | length; 0: not there), and for the longer codes and the patterns that
// are no code the canonical walk over count[] and symbol[] (the second level)
struct PiCode {
    uint16_t fast[1 << PI_FAST_BITS];
    uint16_t count[16];
    uint16_t symbol[288];
};

struct PiTables {
    PiCode ll, d;                               // d also serves as the code-length code while a dynamic header is read
    uint8_t lens[320];
    int verdict;                                // what the building lane found, for all lanes
};

// ---- the bit reader: `hold` has `n` bits, least significant first; `ip` is the next byte of data, never past `end` -----------------------------------------------
struct PiBits {
    const uint8_t* data;
    long ip, end;
    uint64_t hold;
    int n;
};

PD_HD void pi_refill(PiBits& b) {
    if (b.end - b.ip >= 8) {
        uint64_t w = 0;
        for (int k = 0; k < 8; ++k) w |= (uint64_t)b.data[b.ip + k] << (8 * k);
        b.hold |= b.n < 64 ? w << b.n : 0;
        const int take = (63 - b.n) >> 3;
        b.ip += take;
        b.n += 8 * take;
    } else {
        while (b.n <= 56 && b.ip < b.end) {
            b.hold |= (uint64_t)b.data[b.ip++] << b.n;
            b.n += 8;
        }
    }
    if (b.n < 64) b.hold &= (1ull << b.n) - 1;                                  // the bits past n are zeros
}

PD_HD long pi_bits_left(const PiBits& b) { return b.n + 8 * (b.end - b.ip); }

PD_HD void pi_drop(PiBits& b, int k) {
    b.hold >>= k;
    b.n -= k;
}

// k <= 16 bits; false where the input ends first (nothing is consumed then)
PD_HD bool pi_take(PiBits& b, int k, uint32_t& v) {
    if (b.n < k) pi_refill(b);
    if (b.n < k) return false;
    v = (uint32_t)(b.hold & ((1u << k) - 1));
    pi_drop(b, k);
    return true;
}

// ---- code lengths -> a code ------------------------------------------------------------------------------------------------------------------------------------------
// The counts and the sorted symbols of lens[0 .. n) (n <= 288, every length <= 15).  Returns -1 for an over-subscribed set, else what is left of the code space in
// units of 2^-15 (0: complete).  The caller has zeroed c->fast.
PD_HD int pi_build(const uint8_t* lens, int n, PiCode* c) {
    int offs[16];
    for (int l = 0; l < 16; ++l) c->count[l] = 0;
    for (int s = 0; s < n; ++s) ++c->count[lens[s] & 15];
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - c->count[l];
        if (left < 0) return -1;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + c->count[l];
    for (int s = 0; s < n; ++s)
        if (lens[s] & 15) c->symbol[offs[lens[s] & 15]++] = (uint16_t)s;
    int code = 0, index = 0;
    for (int l = 1; l <= PI_FAST_BITS; ++l) {
        for (int k = 0; k < c->count[l]; ++k, ++code, ++index) {
            uint32_t r = 0;
            for (int bit = 0; bit < l; ++bit) r |= (((uint32_t)code >> bit) & 1u) << (l - 1 - bit);
            for (uint32_t at = r; at < (1u << PI_FAST_BITS); at += 1u << l) c->fast[at] = (uint16_t)(c->symbol[index] << 4 | l);
        }
        code <<= 1;
    }
    return left;
}

template <class C>
PD_HD void pi_clear_fast(PiCode* c) {
    for (int i = C::lane(); i < (1 << PI_FAST_BITS); i += C::lanes()) c->fast[i] = 0;
    C::sync();
}

// what kind of code the lengths must be: the rules of zlib's inflate_table
constexpr int PI_KIND_CL = 0, PI_KIND_LL = 1, PI_KIND_D = 2;

// all lanes: build `c` from t->lens[at .. at + n); returns 0 or PI_BAD_LENGTHS
template <class C>
PD_HD int pi_build_checked(PiTables* t, int at, int n, PiCode* c, int kind) {
    pi_clear_fast<C>(c);
    if (C::lane() == 0) {
        const int left = pi_build(t->lens + at, n, c);
        const int codes = n - c->count[0];
        bool ok = left == 0;
        if (kind == PI_KIND_D) ok = left == 0 || codes == 0 || (codes == 1 && c->count[1] == 1);       // no distance code at all, or a single one of length 1
        if (kind == PI_KIND_LL && ok) ok = (t->lens[at + PD_EOB] & 15) != 0;                             // no end of block
        t->verdict = ok ? 0 : PI_BAD_LENGTHS;
    }
    C::sync();
    const int v = t->verdict;
    C::sync();
    return v;
}

// one symbol of `c`; -1 with a bit in status: a pattern that is no code (PI_BAD_SYMBOL), or the input ends first (PI_TRUNCATED; also where fewer than 15 bits are
// left and they start no code, since the zeros behind them were not in the stream)
PD_HD int pi_symbol(PiBits& b, const PiCode* c, int& status) {
    if (b.n < 15) pi_refill(b);
    int sym = -1, len = 0;
    const uint32_t e = c->fast[b.hold & ((1u << PI_FAST_BITS) - 1)];
    if (e) {
        sym = (int)(e >> 4);
        len = (int)(e & 15u);
    } else {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l <= 15; ++l) {
            code |= (int)((b.hold >> (l - 1)) & 1u);
            const int count = c->count[l];
            if (code - count < first) {
                sym = c->symbol[index + (code - first)];
                len = l;
                break;
            }
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
    }
    if (sym < 0) {
        status |= b.n < 15 ? PI_TRUNCATED : PI_BAD_SYMBOL;
        return -1;
    }
    if (len > b.n) {
        status |= PI_TRUNCATED;
        return -1;
    }
    pi_drop(b, len);
    return sym;
}

// ---- the output of one piece ------------------------------------------------------------------------------------------------------------------------------------------
struct PiOut {
    uint8_t* ring;                              // PI_RING bytes, indexed by pos & (PI_RING - 1); nullptr in PI_CHUNK_SIZE
    uint8_t* dst;                               // the frame's filtered area, cap bytes
    long at, cap;                               // where the piece's output starts in dst; pos counts from there
    long pos;
    uint64_t sum, weighted;                     // this lane's share of Σ d[i] and Σ (i mod 65521) d[i], i the position in the piece
};

PD_HD void pi_emit(PiOut& o, long i, uint32_t v) {
    o.ring[i & (PI_RING - 1)] = (uint8_t)v;
    o.dst[o.at + i] = (uint8_t)v;
    o.sum += v;
    o.weighted += (uint64_t)v * (uint32_t)((uint64_t)i % PD_ADLER_MOD);
}

PD_HD void pi_length_base(int sym, int& base, int& extra) {                     // sym 257 .. 285
    if (sym < 265) {
        base = sym - 254;
        extra = 0;
    } else if (sym == 285) {
        base = 258;
        extra = 0;
    } else {
        extra = (sym - 261) >> 2;
        base = 3 + ((4 + ((sym - 261) & 3)) << extra);
    }
}

PD_HD void pi_distance_base(int sym, int& base, int& extra) {                   // sym 0 .. 29
    if (sym < 4) {
        base = 1 + sym;
        extra = 0;
    } else {
        extra = (sym >> 1) - 1;
        base = 1 + ((2 + (sym & 1)) << extra);
    }
}

// The header of a dynamic block: HLIT, HDIST, HCLEN, the code-length code, the two sets of lengths as ONE sequence (a repeat may cross from one into the other).
template <class C>
PD_HD int pi_dynamic_header(PiBits& b, PiTables* t) {
    uint32_t hlit, hdist, hclen, v;
    if (!pi_take(b, 5, hlit) || !pi_take(b, 5, hdist) || !pi_take(b, 4, hclen)) return PI_TRUNCATED;
    const int nlen = 257 + (int)hlit, ndist = 1 + (int)hdist, ncode = 4 + (int)hclen;
    if (nlen > 286 || ndist > 30) return PI_BAD_LENGTHS;
    if (C::lane() == 0)
        for (int i = 0; i < PD_CL_SYMBOLS; ++i) t->lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!pi_take(b, 3, v)) return PI_TRUNCATED;
        if (C::lane() == 0) t->lens[pd_cl_order(i)] = (uint8_t)v;
    }
    C::sync();
    int status = pi_build_checked<C>(t, 0, PD_CL_SYMBOLS, &t->d, PI_KIND_CL);
    if (status) return status;
    int have = 0, prev = 0;
    while (have < nlen + ndist) {
        const int sym = pi_symbol(b, &t->d, status);
        if (sym < 0) return status;
        int len = 0, rep = 1;
        if (sym < 16) {
            len = sym;
        } else {
            const int eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (!pi_take(b, eb, v)) return PI_TRUNCATED;
            if (sym == 16) {
                if (have == 0) return PI_BAD_LENGTHS;
                len = prev;
                rep = 3 + (int)v;
            } else {
                rep = (sym == 17 ? 3 : 11) + (int)v;
            }
            if (have + rep > nlen + ndist) return PI_BAD_LENGTHS;
        }
        if (C::lane() == 0)
            for (int k = 0; k < rep; ++k) t->lens[have + k] = (uint8_t)len;
        have += rep;
        prev = len;
    }
    C::sync();
    status = pi_build_checked<C>(t, 0, nlen, &t->ll, PI_KIND_LL);
    if (status) return status;
    return pi_build_checked<C>(t, nlen, ndist, &t->d, PI_KIND_D);
}

template <class C>
PD_HD int pi_fixed_tables(PiTables* t) {
    for (int s = C::lane(); s < 320; s += C::lanes()) t->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
    C::sync();
    const int status = pi_build_checked<C>(t, 0, 288, &t->ll, PI_KIND_LL);
    return status | pi_build_checked<C>(t, 288, 32, &t->d, PI_KIND_D);
}

// The tokens of one Huffman block up to its end of block.
template <class C>
PD_HD int pi_huffman_block(PiBits& b, PiTables* t, PiOut& o, int mode) {
    int status = 0;
    for (;;) {
        const int sym = pi_symbol(b, &t->ll, status);
        if (sym < 0) return status;
        if (sym < 256) {
            if (o.at + o.pos >= o.cap) return PI_BAD_SIZE;
            if (mode != PI_CHUNK_SIZE && C::lane() == 0) pi_emit(o, o.pos, (uint32_t)sym);
            ++o.pos;
            continue;
        }
        if (sym == PD_EOB) return 0;
        if (sym > 285) return PI_BAD_SYMBOL;
        int base, extra;
        uint32_t v = 0;
        pi_length_base(sym, base, extra);
        if (extra && !pi_take(b, extra, v)) return PI_TRUNCATED;
        const int len = base + (int)v;
        const int dsym = pi_symbol(b, &t->d, status);
        if (dsym < 0) return status;
        if (dsym > 29) return PI_BAD_SYMBOL;
        pi_distance_base(dsym, base, extra);
        v = 0;
        if (extra && !pi_take(b, extra, v)) return PI_TRUNCATED;
        const long dist = base + (long)v;
        if (dist > o.pos) return mode == PI_STREAM ? PI_BAD_DISTANCE : PI_NOT_INDEPENDENT;
        if (o.at + o.pos + len > o.cap) return PI_BAD_SIZE;
        if (mode != PI_CHUNK_SIZE) {
            C::sync();                          // the bytes the lanes stored for the tokens before this one are in the ring
            const long from = o.pos - dist;
            for (int i = C::lane(); i < len; i += C::lanes()) pi_emit(o, o.pos + i, o.ring[(from + i % dist) & (PI_RING - 1)]);
        }
        o.pos += len;
    }
}

template <class C>
PD_HD int pi_stored_block(PiBits& b, PiOut& o, int mode) {
    uint32_t len, nlen;
    pi_drop(b, b.n & 7);
    if (!pi_take(b, 16, len) || !pi_take(b, 16, nlen)) return PI_TRUNCATED;
    if ((len ^ 0xffffu) != nlen) return PI_BAD_BLOCK;
    b.ip -= b.n >> 3;                           // whole bytes: give them back and copy from the input
    b.hold = 0;
    b.n = 0;
    if (b.end - b.ip < (long)len) return PI_TRUNCATED;
    if (o.at + o.pos + (long)len > o.cap) return PI_BAD_SIZE;
    if (mode != PI_CHUNK_SIZE)
        for (long i = C::lane(); i < (long)len; i += C::lanes()) pi_emit(o, o.pos + i, b.data[b.ip + i]);
    b.ip += len;
    o.pos += len;
    return 0;
}

// One piece: data[begin, end) is raw deflate (no zlib header, no Adler bytes).
//   PI_STREAM       the whole stream of a frame: blocks up to the final one, which must end in the last byte of the range, and exactly cap bytes of output.
//   PI_CHUNK_SIZE   counts the piece's output and stores nothing (ring and dst are not touched; `at` is 0, where the output ends is checked by PI_CHUNK_WRITE).
//   PI_CHUNK_WRITE  the piece's output goes to dst[at ...].
// In the chunk modes the piece must be whole blocks that end exactly at `end`, with a final block in the last piece (`last`) and only there, and no distance may
// reach before the piece's own first byte; anything else, and every error, also sets PI_NOT_INDEPENDENT.
// Returns the status bits; produced: the bytes of output; adler3: A, B of the piece's bytes as pd_adler_combine takes them, and their number.
template <class C>
PD_HD int pi_inflate(const uint8_t* data, long begin, long end, int mode, bool last, PiTables* t, uint8_t* ring, uint8_t* dst, long at, long cap, long* produced,
                     uint32_t* adler3) {
    PiBits b = {data, begin, end, 0, 0};
    PiOut o = {ring, dst, at, cap, 0, 0, 0};
    int status = 0;
    bool final_seen = false;
    if (at < 0 || at > cap) status = PI_BAD_RANGE;
    while (!status) {
        uint32_t head;
        if (!pi_take(b, 3, head)) {
            status = PI_TRUNCATED;
            break;
        }
        const int type = (int)(head >> 1);
        if (type == 0) status = pi_stored_block<C>(b, o, mode);
        else if (type == 3) status = PI_BAD_BLOCK;
        else {
            status = type == 1 ? pi_fixed_tables<C>(t) : pi_dynamic_header<C>(b, t);
            if (!status) status = pi_huffman_block<C>(b, t, o, mode);
        }
        if (status) break;
        const long left = pi_bits_left(b);
        if (head & 1u) {
            final_seen = true;
            if (left >= 8) status = PI_BAD_SIZE;                               // bytes behind the final block
            break;
        }
        if (mode != PI_STREAM && left == 0) break;                              // the piece ends with a block that ends with a byte
    }
    if (mode == PI_STREAM) {
        if (!status && o.pos != cap) status = PI_BAD_SIZE;
    } else {
        if (!status && (final_seen != last || (last && mode == PI_CHUNK_WRITE && at + o.pos != cap))) status = PI_NOT_INDEPENDENT;
        if (status) status |= PI_NOT_INDEPENDENT;
    }
    *produced = o.pos;
    if (mode != PI_CHUNK_SIZE) {
        const uint64_t S = C::sum(o.sum) % PD_ADLER_MOD, T = C::sum(o.weighted) % PD_ADLER_MOD, n = (uint64_t)o.pos % PD_ADLER_MOD;
        adler3[0] = (uint32_t)((1u + S) % PD_ADLER_MOD);
        adler3[1] = (uint32_t)((n + n * S + PD_ADLER_MOD - T) % PD_ADLER_MOD);  // n + Σ (n - i) d[i]
        adler3[2] = (uint32_t)o.pos;
    }
    return status;
}

// the Adler-32 of a frame from its pieces' triples
PD_HD uint32_t pi_adler_of(const uint32_t* adler3, int pieces) {
    uint32_t A = 1, B = 0;
    for (int k = 0; k < pieces; ++k) pd_adler_combine(A, B, adler3[3 * k], adler3[3 * k + 1], adler3[3 * k + 2]);
    return B << 16 | A;
}

// ---- the filter inverses: x the filtered byte, a the byte bpp to the left, b the byte above, c the byte above a (zeros outside the image) ---------------------------
PD_HD int pi_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

PD_HD int pi_unfilter_byte(int type, int x, int a, int b, int c) {
    const int pred = type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : type == 4 ? pi_paeth(a, b, c) : 0;
    return (x + pred) & 255;
}

// A frame serially: filtered [H, 1 + bpp W] -> rgb [H, W, 3] (bpp 3 or 4; the fourth byte of a pixel takes no part in the other three and is dropped).  A filter type
// above 4 is read as 0 and reported.
PD_HD int pi_unfilter_frame(const uint8_t* filtered, int H, int W, int bpp, uint8_t* rgb) {
    const long row = 1 + (long)bpp * W;
    int status = 0;
    for (int y = 0; y < H; ++y) {
        int type = filtered[y * row];
        if (type > 4) {
            status |= PI_BAD_FILTER;
            type = 0;
        }
        for (int x = 0; x < W; ++x)
            for (int ch = 0; ch < 3; ++ch) {
                const long at = ((long)y * W + x) * 3 + ch;
                const int a = x > 0 ? rgb[at - 3] : 0, b = y > 0 ? rgb[at - 3L * W] : 0, c = x > 0 && y > 0 ? rgb[at - 3L * W - 3] : 0;
                rgb[at] = (uint8_t)pi_unfilter_byte(type, filtered[y * row + 1 + (long)x * bpp + ch], a, b, c);
            }
    }
    return status;
}
