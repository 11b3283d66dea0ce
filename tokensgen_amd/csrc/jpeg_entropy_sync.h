// The self-synchronising entropy decoder of csrc/jpeg_decode_sync.hip as plain inline code that a kernel and a host program both compile: a decoder
// state at a symbol boundary, one subsequence of a restart segment decoded from an entry state to an exit state (count mode), and the same with the coefficients
// stored (write mode).  The Huffman step, the EXTEND rule and the status bits are those of jpeg_entropy_dec.h.  No HIP type appears here;
// tests/csrc/jpeg_sync_host.cpp includes this file under g++ with the address and undefined-behaviour sanitizers.
//
// A segment's bytes are cut into subsequences of sub_bytes raw bytes.  Lane i starts at the first bit of subsequence i with the guess (block 0, index 0) and decodes
// symbols while a symbol STARTS inside its subsequence; a symbol with its extra bits belongs to the lane in which it starts.  In rounds, lane i takes lane i - 1's exit
// as its entry and decodes again if that differs from the entry it used (from its own guess where that entry is invalid); lane 0's entry is true, truth moves on by at
// least one lane per round, and at the fixed point every entry is the serial decoder's state.  The caller runs the rounds; this file holds what one lane does.
#pragma once
#include "jpeg_entropy_dec.h"

// how a state was reached
enum : uint32_t {
    JS_VALID = 0,                // a symbol boundary of a decode without error
    JS_END = 1,                  // the data ended where a DC code should start, inside the last byte: the padding bits
    JS_INVALID = 2               // the decode from this lane's entry met a condition that jd_decode_block reports
};

// pos: the canonical bit position, 8 * (raw byte that holds the next bit, from the segment's first byte) + (bit within it, 0 the most significant).  It never rests on
// the 00 of an FF 00 pair and does not depend on how far a reader has prefetched.  at: how << 16 | block within the MCU << 8 | zigzag index; index 0: the next symbol
// is a DC code.  JS_END and JS_INVALID states are all zero below `how`, so two of them compare equal.
struct JsState {
    uint32_t pos;
    uint32_t at;
};
constexpr uint32_t JS_MAX_SEGMENT_BYTES = 1u << 28;     // pos counts bits in 32
constexpr int JS_MAX_SYMBOL_BITS = 16 + 11;             // a code and its extra bits

JD_HD JsState js_state(uint32_t pos, int blk, int k) { return JsState{pos, (uint32_t)blk << 8 | (uint32_t)k}; }
JD_HD JsState js_stopped(uint32_t how) { return JsState{0u, how << 16}; }
JD_HD uint32_t js_how(const JsState& s) { return s.at >> 16; }
JD_HD bool js_same(const JsState& a, const JsState& b) { return a.pos == b.pos && a.at == b.at; }

// the guess of the lane whose subsequence starts at raw byte `start` (> 0): its first bit, skipping the 00 of an FF 00 pair that the boundary splits
JD_HD JsState js_guess(const uint8_t* seg, uint32_t seg_bytes, uint32_t start) {
    if (start > 0 && start < seg_bytes && seg[start] == 0 && seg[start - 1] == 0xffu) ++start;
    return js_state(start * 8u, 0, 0);
}

// What a lane decodes from: the entry it was handed, or its own guess again where that entry is JS_INVALID, so that the lanes behind a wrong chain that met an error
// keep looking for the true chain.  A chain with such a lane on it at the fixed point is not vouched for.
JD_HD JsState js_effective(const JsState& entry, const JsState& guess) { return js_how(entry) == JS_INVALID ? guess : entry; }

// symbol steps of one lane: every symbol takes at least one bit, and one more symbol may start in the subsequence's last bit
JD_HD int js_max_steps(int sub_bytes) { return 8 * sub_bytes + 1; }

// The bit reader: jd_symbol and jd_receive_extend work on `br`, whose own byte range is empty (jd_fill does nothing); js_fill feeds it from seg[p .. end) and keeps,
// for the bytes that `br.acc` holds, whether each came from an FF 00 pair, so that the canonical position follows from p, br.n and those flags alone.
struct JsReader {
    JdBitReader br;
    const uint8_t* seg;
    uint32_t p, end;             // the next raw byte to load, the segment's bytes
    uint32_t pairs;              // bit j: the j-th last loaded byte was an FF with its 00
    int eod;                     // an FF followed by anything but 00: the data ends before it (p stays on it)
};

JD_HD void js_fill(JsReader& r) {
    while (r.br.n <= 24 && !r.eod && r.p < r.end) {     // every read is at an index < end
        const uint32_t b = r.seg[r.p];
        uint32_t pair = 0;
        if (b == 0xffu) {
            if (r.p + 1 < r.end && r.seg[r.p + 1] == 0) {
                pair = 1;
            } else {
                r.eod = 1;
                break;
            }
        }
        r.p += 1 + pair;
        r.pairs = (r.pairs << 1) | pair;
        r.br.acc = (r.br.acc << 8) | b;
        r.br.n += 8;
    }
}

JD_HD uint32_t js_position(const JsReader& r) {
    const int held = (r.br.n + 7) >> 3;                 // bytes that br.acc still holds bits of, at most 4
    const uint32_t byte = r.p - (uint32_t)held - (uint32_t)__builtin_popcount(r.pairs & ((1u << held) - 1u));
    return byte * 8u + (uint32_t)((8 - (r.br.n & 7)) & 7);
}

// One subsequence: from the state `in`, symbols while one starts before raw byte sub_end (<= seg_bytes), at most max_steps of them.  Returns the exit state; *started
// receives the blocks started, that is the DC symbols completed.  WRITE: the coefficients go to coef, the segment's n_blocks blocks of 64, which the caller has zeroed:
// block_base is the number of blocks started before this lane, an entry inside a block continues block block_base - 1; DC values are stored as differences; every
// store's block index is checked against n_blocks.  seg_bytes <= JS_MAX_SEGMENT_BYTES.
template <bool WRITE>
JD_HD JsState js_run(const uint8_t* seg, uint32_t seg_bytes, uint32_t sub_end, int max_steps, const JdHuffTable* tabs, int bpm, JsState in, int32_t* started,
                     int16_t* coef, long block_base, long n_blocks) {
    *started = 0;
    if (js_how(in) != JS_VALID) return in;
    JsReader r;
    r.br.p = r.br.end = seg;
    r.br.acc = 0;
    r.br.n = 0;
    r.br.err = 0;
    r.seg = seg;
    r.p = in.pos >> 3;
    r.end = seg_bytes;
    r.pairs = 0;
    r.eod = 0;
    if (r.p > seg_bytes) return js_stopped(JS_INVALID);
    js_fill(r);
    const int skip = (int)(in.pos & 7u);
    if (skip > r.br.n) return js_stopped(JS_INVALID);   // a position inside a byte that the data does not have
    r.br.n -= skip;
    int blk = (int)((in.at >> 8) & 255u), k = (int)(in.at & 255u);
    if (blk >= bpm || k > 63) return js_stopped(JS_INVALID);
    long cur = block_base - 1;
    int n_started = 0;
    uint32_t pos = in.pos;
    for (int step = 0; step < max_steps; ++step) {
        js_fill(r);
        pos = js_position(r);
        if ((pos >> 3) >= sub_end) break;
        const int comp = blk < bpm - 2 ? 0 : blk - (bpm - 3);
        if (k == 0) {
            const int left = r.br.n;
            int s = jd_symbol(r.br, tabs + 2 * comp);
            if (s < 0) {                                // nothing was consumed
                *started = n_started;
                return js_stopped((r.eod || r.p >= r.end) && left < 8 ? JS_END : JS_INVALID);
            }
            if (s > 11) r.br.err |= JD_ST_CATEGORY;
            int v = 0;
            if (s && !r.br.err) {
                js_fill(r);
                v = jd_receive_extend(r.br, s);
            }
            if (r.br.err) break;
            cur = block_base + n_started;
            ++n_started;
            if (WRITE && cur >= 0 && cur < n_blocks) coef[cur * 64] = (int16_t)v;
            k = 1;
            continue;
        }
        const int rs = jd_symbol(r.br, tabs + 2 * comp + 1);
        if (rs < 0) break;
        const int run = rs >> 4, s = rs & 15;
        bool done = false;
        if (s == 0) {
            if (run == 0) {
                done = true;
            } else if (run == 15) {
                k += 16;
                if (k > 64) r.br.err |= JD_ST_COEF_INDEX;
                done = k == 64;
            } else {
                r.br.err |= JD_ST_INVALID_CODE;
            }
        } else if (s > 10) {
            r.br.err |= JD_ST_CATEGORY;
        } else {
            k += run;
            if (k > 63) {
                r.br.err |= JD_ST_COEF_INDEX;
            } else {
                js_fill(r);
                const int v = jd_receive_extend(r.br, s);
                if (!r.br.err) {
                    if (WRITE && cur >= 0 && cur < n_blocks) coef[cur * 64 + k] = (int16_t)v;
                    done = ++k == 64;
                }
            }
        }
        if (r.br.err) break;
        if (done) {
            k = 0;
            blk = blk + 1 == bpm ? 0 : blk + 1;
        }
    }
    *started = n_started;
    if (r.br.err) return js_stopped(JS_INVALID);
    js_fill(r);
    pos = js_position(r);
    if ((pos >> 3) < sub_end) return js_stopped(JS_INVALID);        // the step bound ran out (an entry before the subsequence): no exit to pass on
    return js_state(pos, blk, k);
}

// What the converged chain of one segment must show: no lane was handed an invalid entry, it ended without an invalid lane, at a block boundary of a whole MCU, having
// started exactly its blocks.
JD_HD bool js_segment_clean(bool invalid_entry, const JsState& last, long started, long n_blocks) {
    return !invalid_entry && js_how(last) != JS_INVALID && (last.at & 0xffffu) == 0 && started == n_blocks;
}

// The running DC of MCUs [m0, m1) of a segment whose blocks hold DC differences: pred holds the three components' sums before m0 (int32) and after the call those
// before m1.  STORE: the running value replaces the difference, clamped to int16 as jd_decode_block stores it.
template <bool STORE>
JD_HD void js_dc_prefix(int16_t* coef, int bpm, long m0, long m1, int32_t& p0, int32_t& p1, int32_t& p2) {
    for (long m = m0; m < m1; ++m)
        for (int b = 0; b < bpm; ++b) {
            int16_t* dc = coef + (m * bpm + b) * 64;
            const int comp = b < bpm - 2 ? 0 : b - (bpm - 3);
            int32_t pred = comp == 0 ? p0 : comp == 1 ? p1 : p2;
            pred += *dc;
            if (STORE) *dc = (int16_t)(pred < -32768 ? -32768 : pred > 32767 ? 32767 : pred);
            p0 = comp == 0 ? pred : p0;
            p1 = comp == 1 ? pred : p1;
            p2 = comp == 2 ? pred : p2;
        }
}
