// Parallel entropy decoding inside a restart segment: the self-synchronising decoder of jpeg_entropy_sync.h, for streams whose restart segments are
// long, above all the files without any restart marker that most encoders write.  The result is the coefficient array of tg_jpeg_decode_coeffs, bit for bit.
//   tg_jpeg_decode_coeffs_sync, first launch: one workgroup of 1024 lanes per (segment, frame), the frame's six Huffman tables in LDS.  The workgroup zeroes its
//                  segment's coefficients, then takes the segment's bytes 1024 subsequences of sub_bytes at a time (a chunk).  Every lane decodes its subsequence from
//                  the guess (block 0, index 0) in count mode and leaves its exit state in LDS; in rounds lane i takes lane i - 1's exit as its entry and decodes
//                  again where that differs from the entry it used (from its guess where that entry is invalid), until a round changes nothing: at most (lanes of
//                  the chunk) - 1 rounds, since lane 0's entry is true and truth moves on by one lane a round.  A prefix sum of the blocks every lane started gives it its first block; the lanes decode once more
//                  and store the coefficients, DC values as differences.  The last lane's exit is the next chunk's entry.  Last, a prefix sum per component over the
//                  segment's blocks turns the differences into the running DC (int32, stored clamped to int16).  Every loop has a bound computed before it starts, every
//                  lane reaches every barrier, every store's block index is checked against the segment's blocks.  Whether the converged chain is the whole segment
//                  (no invalid lane, exactly its blocks, ending between two MCUs) goes to the workspace with the rounds taken.
//   second launch: one workgroup per frame folds the segments' verdicts into clean[f] and rounds[f].
// status is not an argument: lanes that decode from a wrong guess meet errors all the time, and these are not findings.
#include "common.h"
#include "jpeg_common.h"
#include "jpeg_entropy_sync.h"
#include "tokensgen_hip.h"

namespace {

constexpr int SY_LANES = 1024, SY_WAVES = SY_LANES / 64;

long segments_of(const Geometry& g, int restart) { return restart == 0 ? 1 : (g.n_mcu + restart - 1) / restart; }

// exclusive prefix sum of v over the workgroup and the workgroup's total; wave_total [SY_WAVES] in LDS.  Two barriers.
__device__ __forceinline__ int block_exclusive(int v, int* wave_total, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < SY_WAVES; ++w) {
        const int t = wave_total[w];
        before += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();                            // wave_total is rewritten by the next call
    return before + incl - v;
}

__global__ __launch_bounds__(SY_LANES) void jpeg_sync_kernel(const uint8_t* __restrict__ data, long data_bytes, const long long* __restrict__ seg_begin,
                                                             const long long* __restrict__ seg_end, long n_seg, long n_mcu, int bpm, long restart,
                                                             const uint32_t* __restrict__ htabs, int n_sets, const int32_t* __restrict__ htab_index, int sub_bytes,
                                                             int16_t* __restrict__ coef, int32_t* __restrict__ seg_clean, int32_t* __restrict__ seg_rounds) {
    constexpr int SET_WORDS = JD_TABLES_PER_SET * JD_TABLE_BYTES / 4;
    __shared__ __align__(16) uint32_t tab_words[SET_WORDS];
    __shared__ uint32_t exit_pos[SY_LANES], exit_at[SY_LANES];
    __shared__ int wave_total[SY_WAVES];
    const int tid = threadIdx.x;
    const int f = blockIdx.y;
    const long s = blockIdx.x;                  // < n_seg: the grid is n_seg wide
    const int set = htab_index[f];
    const bool set_ok = set >= 0 && set < n_sets;
    if (set_ok)
        for (int i = tid; i < SET_WORDS; i += SY_LANES) tab_words[i] = htabs[(long)set * SET_WORDS + i];
    const JdHuffTable* tabs = (const JdHuffTable*)tab_words;
    const long m0 = s * restart, m1 = m0 + restart < n_mcu ? m0 + restart : n_mcu;          // m0 < n_mcu: n_seg = ceil(n_mcu / restart)
    const long n_blocks = (m1 - m0) * bpm;
    int16_t* out = coef + ((long)f * n_mcu + m0) * bpm * 64;
    const long long b = seg_begin[(long)f * n_seg + s], e = seg_end[(long)f * n_seg + s];
    const bool ok = set_ok && b >= 0 && e >= b && e <= data_bytes && e - b <= (long long)JS_MAX_SEGMENT_BYTES;
    const uint8_t* seg = data + (ok ? b : 0);
    const uint32_t bytes = ok ? (uint32_t)(e - b) : 0u;
    for (long i = tid; i < n_blocks * 8; i += SY_LANES) ((uint4*)out)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();                            // the tables are in LDS, and no value is stored into a block before every block is zero

    const uint32_t chunk_bytes = (uint32_t)SY_LANES * (uint32_t)sub_bytes;                 // <= 2^18
    const uint32_t n_chunks = (bytes + chunk_bytes - 1) / chunk_bytes;                      // bytes <= 2^28
    const int max_steps = js_max_steps(sub_bytes);
    JsState carry = js_state(0, 0, 0);          // the true state at the chunk's first byte; the same in every lane
    long base = 0;                              // blocks started before the chunk
    int most_rounds = 0, invalid_entry = 0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t c0 = c * chunk_bytes, left = bytes - c0;
        const int n_act = left >= chunk_bytes ? SY_LANES : (int)((left + (uint32_t)sub_bytes - 1) / (uint32_t)sub_bytes);     // >= 1
        const bool active = tid < n_act;
        const uint32_t start = c0 + (uint32_t)tid * (uint32_t)sub_bytes;
        const uint32_t sub_end = active ? (start + (uint32_t)sub_bytes < bytes ? start + (uint32_t)sub_bytes : bytes) : 0u;
        const JsState guess = active ? js_guess(seg, bytes, start) : carry;
        JsState entry = tid == 0 ? carry : guess, exit = carry;
        int32_t started = 0;
        if (active) {
            exit = js_run<false>(seg, bytes, sub_end, max_steps, tabs, bpm, js_effective(entry, guess), &started, nullptr, 0, 0);
            exit_pos[tid] = exit.pos;
            exit_at[tid] = exit.at;
        }
        __syncthreads();
        int rounds = 1;
        for (int r = 1; r < n_act; ++r) {       // n_act is the same in every lane, and so is the break below
            JsState next = entry;
            if (active && tid > 0) next = JsState{exit_pos[tid - 1], exit_at[tid - 1]};
            __syncthreads();                    // every exit is read before any is replaced
            int changed = 0;
            if (active && !js_same(next, entry)) {
                entry = next;
                exit = js_run<false>(seg, bytes, sub_end, max_steps, tabs, bpm, js_effective(entry, guess), &started, nullptr, 0, 0);
                exit_pos[tid] = exit.pos;
                exit_at[tid] = exit.at;
                changed = 1;
            }
            if (!__syncthreads_or(changed)) break;
            ++rounds;
        }
        most_rounds = rounds > most_rounds ? rounds : most_rounds;
        const JsState last = JsState{exit_pos[n_act - 1], exit_at[n_act - 1]};
        invalid_entry |= __syncthreads_or(active && js_how(entry) == JS_INVALID);
        int total;
        const int before = block_exclusive(active ? started : 0, wave_total, total);       // its barriers also keep `last` from the next chunk's stores
        if (active) {
            int32_t again;
            js_run<true>(seg, bytes, sub_end, max_steps, tabs, bpm, js_effective(entry, guess), &again, out, base + before, n_blocks);
        }
        carry = last;
        base += total;
    }
    __syncthreads();                            // the differences are in memory before the prefix reads them

    // the running DC: every lane sums the differences of its run of MCUs, a prefix over the lanes, then the lane adds them up again and stores
    const long per_lane = (m1 - m0 + SY_LANES - 1) / SY_LANES;
    long a0 = (long)tid * per_lane, a1 = a0 + per_lane;
    a0 = a0 < m1 - m0 ? a0 : m1 - m0;
    a1 = a1 < m1 - m0 ? a1 : m1 - m0;
    int32_t p0 = 0, p1 = 0, p2 = 0, unused;
    js_dc_prefix<false>(out, bpm, a0, a1, p0, p1, p2);
    p0 = block_exclusive(p0, wave_total, unused);
    p1 = block_exclusive(p1, wave_total, unused);
    p2 = block_exclusive(p2, wave_total, unused);
    js_dc_prefix<true>(out, bpm, a0, a1, p0, p1, p2);
    if (tid == 0) {
        seg_clean[(long)f * n_seg + s] = ok && js_segment_clean(invalid_entry != 0, carry, base, n_blocks) ? 1 : 0;
        seg_rounds[(long)f * n_seg + s] = most_rounds;
    }
}

__global__ __launch_bounds__(256) void jpeg_sync_finish_kernel(const int32_t* __restrict__ seg_clean, const int32_t* __restrict__ seg_rounds, long n_seg,
                                                               int32_t* __restrict__ clean, int32_t* __restrict__ rounds) {
    __shared__ int most;
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) most = 0;
    __syncthreads();
    int all = 1, mine = 0;
    for (long k = tid; k < n_seg; k += 256) {
        all &= seg_clean[(long)f * n_seg + k] == 1;
        const int r = seg_rounds[(long)f * n_seg + k];
        mine = r > mine ? r : mine;
    }
    atomicMax(&most, mine);
    all = __syncthreads_and(all);
    if (tid == 0) {
        clean[f] = all;
        rounds[f] = most;
    }
}

bool sub_bytes_ok(int v) { return v == 16 || v == 32 || v == 64 || v == 128 || v == 256; }

}  // namespace

extern "C" long tg_jpeg_sync_ws_bytes(int F, int H, int W, int subsampling, int restart_interval) {
    Geometry g;
    if (F < 1 || F > 65535 || !geometry(H, W, subsampling, g) || restart_interval < 0 || restart_interval > 65535) return 0;
    return 2L * 4 * F * segments_of(g, restart_interval);
}

extern "C" int tg_jpeg_decode_coeffs_sync(const void* data, long data_bytes, const void* seg_begin, const void* seg_end, int F, int H, int W, int subsampling,
                                          int restart_interval, const void* htabs, int n_sets, const void* htab_index, int sub_bytes, void* ws, long ws_bytes, void* coef,
                                          void* clean, void* rounds, hipStream_t stream) {
    TG_REQUIRE(data && seg_begin && seg_end && htabs && htab_index && ws && coef && clean && rounds, TG_ERR_ARG, "tg_jpeg_decode_coeffs_sync: null pointer");
    TG_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, TG_ERR_ARG, "tg_jpeg_decode_coeffs_sync: restart_interval must be in 0..65535 (got %d)",
               restart_interval);
    TG_REQUIRE(n_sets >= 1, TG_ERR_ARG, "tg_jpeg_decode_coeffs_sync: at least one table set (got %d)", n_sets);
    TG_REQUIRE(sub_bytes_ok(sub_bytes), TG_ERR_ARG, "tg_jpeg_decode_coeffs_sync: sub_bytes must be 16, 32, 64, 128 or 256 (got %d)", sub_bytes);
    Geometry g;
    TG_REQUIRE(data_bytes >= 1 && F >= 1 && F <= 65535 && geometry(H, W, subsampling, g), TG_ERR_SHAPE,
               "tg_jpeg_decode_coeffs_sync: bad shape data_bytes=%ld F=%d (1..65535) H=%d W=%d (1..65535) subsampling=%d (420 or 444)", data_bytes, F, H, W, subsampling);
    const long need = tg_jpeg_sync_ws_bytes(F, H, W, subsampling, restart_interval);
    TG_REQUIRE(ws_bytes >= need, TG_ERR_SHAPE, "tg_jpeg_decode_coeffs_sync: the workspace needs %ld bytes (got %ld)", need, ws_bytes);
    TG_REQUIRE(tg_aligned16(coef) && (((uintptr_t)seg_begin | (uintptr_t)seg_end) & 7) == 0 &&
                   (((uintptr_t)htabs | (uintptr_t)htab_index | (uintptr_t)ws | (uintptr_t)clean | (uintptr_t)rounds) & 3) == 0,
               TG_ERR_ALIGN, "tg_jpeg_decode_coeffs_sync: coef must be 16-byte aligned, the byte ranges 8-byte, tables, indices, workspace, clean and rounds 4-byte");
    const long n_seg = segments_of(g, restart_interval), restart = restart_interval == 0 ? g.n_mcu : restart_interval;
    TG_REQUIRE(n_seg < (1L << 31), TG_ERR_SHAPE, "tg_jpeg_decode_coeffs_sync: too many restart segments (%ld)", n_seg);
    int32_t* seg_clean = (int32_t*)ws;
    int32_t* seg_rounds = seg_clean + (long)F * n_seg;
    hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)n_seg, (unsigned)F), dim3(SY_LANES), 0, stream, (const uint8_t*)data, data_bytes, (const long long*)seg_begin,
                       (const long long*)seg_end, n_seg, g.n_mcu, g.bpm, restart, (const uint32_t*)htabs, n_sets, (const int32_t*)htab_index, sub_bytes, (int16_t*)coef,
                       seg_clean, seg_rounds);
    TG_LAUNCH_CHECK("tg_jpeg_decode_coeffs_sync (segments)");
    hipLaunchKernelGGL(jpeg_sync_finish_kernel, dim3((unsigned)F), dim3(256), 0, stream, (const int32_t*)seg_clean, (const int32_t*)seg_rounds, n_seg, (int32_t*)clean,
                       (int32_t*)rounds);
    TG_LAUNCH_CHECK("tg_jpeg_decode_coeffs_sync");
    return TG_OK;
}
