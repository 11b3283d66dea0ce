// Baseline JPEG decoding, the inverse of csrc/jpeg.hip: restart-segment ranges, quantised coefficients, RGB bytes.  Integer arithmetic only; the
// definition is the comment of include/tokensgen_hip.h, restated by tests/jpeg_dec_ref.py.
//   tg_jpeg_find_segments: one workgroup per frame walks the frame's entropy data 2048 bytes at a time, eight bytes per thread.  FF D0 .. D7 cannot occur inside entropy
//                  data (an FF there is followed by 00), so every such pair is a marker.  A wave prefix sum by shuffles and four wave totals in LDS give every marker
//                  its place in order: no atomics, no host wait.  Marker k ends segment k and segment k + 1 starts two bytes later.  Entries that the stream has no
//                  marker for become the empty range at the end of the scan, so the output never depends on old memory.  The kernel stores status[f]: it runs first.
//   tg_jpeg_decode_coeffs: one lane per restart segment (grid.y is the frame), the frame's six Huffman tables in LDS (5472 bytes).  The lane runs jd_decode_segment of
//                  jpeg_entropy_dec.h: every block is zeroed in memory and its non-zero coefficients are stored after, so there is no private array and no scratch.
//                  Errors are OR-ed into status[f].
//   tg_jpeg_idct_rgb:      first launch: eight threads per block as in the encoder, a workgroup takes 32 consecutive blocks (4096 bytes of coefficients, one 16-byte load
//                  per thread into LDS); thread (block, v) dequantises row v and does the first product, thread (block, x) the second; the samples go through LDS
//                  to the planes of the workspace as one 8-byte store per block row.  Second launch: four pixels of one row per thread; at 4:2:0 the triangle filter
//                  reads the real chroma plane of ceil(H / 2) x ceil(W / 2) samples with its edges repeated; three dword stores where the row is dword-aligned, bytes
//                  otherwise, every store checked against the end of the output.
#include "common.h"
#include "jpeg_common.h"
#include "jpeg_entropy_dec.h"
#include "tokensgen_hip.h"

static_assert(JD_ST_INVALID_CODE == TG_JPEG_ST_INVALID_CODE && JD_ST_COEF_INDEX == TG_JPEG_ST_COEF_INDEX && JD_ST_CATEGORY == TG_JPEG_ST_CATEGORY &&
                  JD_ST_OUT_OF_BITS == TG_JPEG_ST_OUT_OF_BITS && JD_ST_RST_COUNT == TG_JPEG_ST_RST_COUNT && JD_ST_RST_NUMBER == TG_JPEG_ST_RST_NUMBER &&
                  JD_ST_RANGE == TG_JPEG_ST_RANGE,
              "the status bits of the header are those of jpeg_entropy_dec.h");

namespace {

// restart_interval 0: no markers, one segment
long segments_of(const Geometry& g, int restart) { return restart == 0 ? 1 : (g.n_mcu + restart - 1) / restart; }

constexpr int FS_THREADS = 256, FS_PER_THREAD = 8;

__global__ __launch_bounds__(FS_THREADS) void jpeg_find_segments_kernel(const uint8_t* __restrict__ data, long data_bytes, const long long* __restrict__ scan_begin,
                                                                        const long long* __restrict__ scan_end, long n_seg, long long* __restrict__ seg_begin,
                                                                        long long* __restrict__ seg_end, int32_t* __restrict__ status) {
    __shared__ int wave_total[FS_THREADS / 64];
    __shared__ int bad;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long b = scan_begin[f], e = scan_end[f];
    int st = 0;
    if (b < 0 || e < b || e > data_bytes) {     // a range outside the buffer: treated as empty
        st |= JD_ST_RANGE;
        b = e = 0;
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    long long* sb = seg_begin + (long)f * n_seg;
    long long* se = seg_end + (long)f * n_seg;
    long found = 0;                             // markers before this chunk; the same in every thread
    int wrong = 0;
    for (long long base = b; base < e; base += FS_THREADS * FS_PER_THREAD) {
        const long long p0 = base + (long long)tid * FS_PER_THREAD;
        uint32_t mask = 0;                      // bit j: a marker starts at p0 + j
        uint32_t prev = p0 < e ? data[p0] : 0;
#pragma unroll
        for (int j = 0; j < FS_PER_THREAD; ++j) {
            const long long q = p0 + j + 1;
            const uint32_t next = q < e ? data[q] : 0;      // q < e <= data_bytes
            if (prev == 0xffu && (next & 0xf8u) == 0xd0u) mask |= 1u << j;
            prev = next;
        }
        const int cnt = __popc(mask);
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < FS_THREADS / 64; ++w) {
            before += w < wave ? wave_total[w] : 0;
            chunk += wave_total[w];
        }
        long k = found + before + (incl - cnt);
#pragma unroll
        for (int j = 0; j < FS_PER_THREAD; ++j)
            if (mask & (1u << j)) {
                if (k < n_seg - 1) {
                    se[k] = p0 + j;
                    sb[k + 1] = p0 + j + 2;
                    if ((data[p0 + j + 1] & 7u) != (uint32_t)(k & 7)) wrong = 1;
                }
                ++k;
            }
        found += chunk;
        __syncthreads();                        // wave_total is rewritten by the next chunk
    }
    if (wrong) bad = 1;                         // every writer stores the same value
    const long have = found < n_seg - 1 ? found : n_seg - 1;
    for (long k = have + tid; k < n_seg - 1; k += FS_THREADS) {
        se[k] = e;
        sb[k + 1] = e;
    }
    __syncthreads();
    if (tid == 0) {
        sb[0] = b;
        se[n_seg - 1] = e;
        if (found != n_seg - 1) st |= JD_ST_RST_COUNT;
        if (bad) st |= JD_ST_RST_NUMBER;
        status[f] = st;
    }
}

__global__ __launch_bounds__(64) void jpeg_decode_coeffs_kernel(const uint8_t* __restrict__ data, long data_bytes, const long long* __restrict__ seg_begin,
                                                                const long long* __restrict__ seg_end, long n_seg, long n_mcu, int bpm, long restart,
                                                                const uint32_t* __restrict__ htabs, int n_sets, const int32_t* __restrict__ htab_index,
                                                                int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    constexpr int SET_WORDS = JD_TABLES_PER_SET * JD_TABLE_BYTES / 4;
    __shared__ __align__(16) uint32_t tab_words[SET_WORDS];
    const int f = blockIdx.y;
    const int set = htab_index[f];
    const bool set_ok = set >= 0 && set < n_sets;
    if (set_ok)
        for (int i = threadIdx.x; i < SET_WORDS; i += 64) tab_words[i] = htabs[(long)set * SET_WORDS + i];
    __syncthreads();
    const long s = (long)blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seg) return;
    const long m0 = s * restart, m1 = m0 + restart < n_mcu ? m0 + restart : n_mcu;         // m0 < n_mcu: n_seg = ceil(n_mcu / restart)
    int16_t* out = coef + ((long)f * n_mcu + m0) * bpm * 64;
    long long b = seg_begin[(long)f * n_seg + s], e = seg_end[(long)f * n_seg + s];
    int st = 0;
    if (!set_ok || b < 0 || e < b || e > data_bytes) {
        st = JD_ST_RANGE;
        for (long i = 0; i < (m1 - m0) * bpm; ++i) jd_zero_block(out + 64 * i);
    } else {
        st = jd_decode_segment(data + b, data + e, (const JdHuffTable*)tab_words, bpm, m1 - m0, out);
    }
    if (st) atomicOr(status + f, st);
}

// the planes of the workspace: Y [F][rows mcu][cols mcu], then Cb and Cr [F][rows 8][cols 8]
struct Planes { long y_w, y_h, c_w, c_h, cb, cr; };
Planes planes_of(const Geometry& g, int F) {
    Planes p;
    p.y_w = (long)g.cols * g.mcu;
    p.y_h = (long)g.rows * g.mcu;
    p.c_w = (long)g.cols * 8;
    p.c_h = (long)g.rows * 8;
    p.cb = F * p.y_w * p.y_h;
    p.cr = p.cb + F * p.c_w * p.c_h;
    return p;
}

template <bool S420>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, long n_blocks, long n_mcu, int mcu_cols, const uint16_t* __restrict__ qtabs,
                                                        int n_qsets, const int32_t* __restrict__ qtab_index, Planes pl, uint8_t* __restrict__ ws) {
    constexpr int BPM = S420 ? 6 : 3;
    __shared__ __align__(16) int16_t zz[32][64];
    __shared__ int32_t tb[32][72];
    __shared__ __align__(8) uint8_t px[32][64];
    const int tid = threadIdx.x, b = tid >> 3, i8 = tid & 7;
    const long first = (long)blockIdx.x * 32, gb = first + b;
    if (first * 8 + tid < n_blocks * 8) ((uint4*)&zz[0][0])[tid] = ((const uint4*)(coef + first * 64))[tid];
    __syncthreads();
    const bool live = gb < n_blocks;
    long f = 0, m = 0;
    int k = 0, comp = 0;
    if (live) {
        const long gm = gb / BPM;
        k = (int)(gb - gm * BPM);
        f = gm / n_mcu;
        m = gm - f * n_mcu;
        comp = S420 ? (k < 4 ? 0 : k - 3) : k;
        int set = qtab_index[f];
        set = set < 0 ? 0 : set >= n_qsets ? n_qsets - 1 : set;
        const uint16_t* q = qtabs + ((long)set * 3 + comp) * 64 + i8 * 8;
        int d[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int v = (int)zz[b][UNZIG.at[i8 * 8 + u]] * (int)q[u];
            d[u] = v < -2048 ? -2048 : v > 2047 ? 2047 : v;
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int s = 512;
#pragma unroll
            for (int u = 0; u < 8; ++u) s += DCT_A[u][x] * d[u];
            tb[b][i8 * 9 + x] = s >> 10;
        }
    }
    __syncthreads();
    if (live) {
        int t[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) t[v] = tb[b][v * 9 + i8];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            int s = 32768;
#pragma unroll
            for (int v = 0; v < 8; ++v) s += DCT_A[v][y] * t[v];
            const int p = (s >> 16) + 128;
            px[b][y * 8 + i8] = (uint8_t)(p < 0 ? 0 : p > 255 ? 255 : p);
        }
    }
    __syncthreads();
    if (live) {
        const long my = m / mcu_cols, mx = m - my * mcu_cols;
        uint8_t* dst;
        if (comp == 0) {
            const long y0 = S420 ? my * 16 + (k >> 1) * 8 : my * 8, x0 = S420 ? mx * 16 + (k & 1) * 8 : mx * 8;
            dst = ws + (f * pl.y_h + y0 + i8) * pl.y_w + x0;
        } else {
            dst = ws + (comp == 1 ? pl.cb : pl.cr) + (f * pl.c_h + my * 8 + i8) * pl.c_w + mx * 8;
        }
        *(uint2*)dst = *(const uint2*)&px[b][i8 * 8];                            // every plane width and x0 is a multiple of 8, ws is 16-byte aligned
    }
}

template <bool S420>
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const uint8_t* __restrict__ ws, Planes pl, long total, int H, int W, int quads, uint8_t* __restrict__ rgb,
                                                       long rgb_bytes) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int qx = (int)(id % quads);
    const long fy = id / quads;
    const int y = (int)(fy % H);
    const long f = fy / H;
    const int x0 = qx * 4;
    const uint8_t* yrow = ws + (f * pl.y_h + y) * pl.y_w + x0;                    // x0 + 3 < y_w: the plane is padded to whole MCUs
    int cb[4], cr[4];
    if constexpr (S420) {
        const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
        const int near = y >> 1;
        int far = (y & 1) ? near + 1 : near - 1;
        far = far < 0 ? 0 : far > ch - 1 ? ch - 1 : far;
        const uint8_t* bn = ws + pl.cb + (f * pl.c_h + near) * pl.c_w;
        const uint8_t* bf = ws + pl.cb + (f * pl.c_h + far) * pl.c_w;
        const uint8_t* rn = ws + pl.cr + (f * pl.c_h + near) * pl.c_w;
        const uint8_t* rf = ws + pl.cr + (f * pl.c_h + far) * pl.c_w;
        const int i0 = x0 >> 1;
        int sb[4], sr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int i = i0 - 1 + j;
            i = i < 0 ? 0 : i > cw - 1 ? cw - 1 : i;
            sb[j] = 3 * bn[i] + bf[i];
            sr[j] = 3 * rn[i] + rf[i];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cb[2 * j] = (3 * sb[j + 1] + sb[j] + 8) >> 4;
            cb[2 * j + 1] = (3 * sb[j + 1] + sb[j + 2] + 7) >> 4;
            cr[2 * j] = (3 * sr[j + 1] + sr[j] + 8) >> 4;
            cr[2 * j + 1] = (3 * sr[j + 1] + sr[j + 2] + 7) >> 4;
        }
    } else {
        const uint8_t* bn = ws + pl.cb + (f * pl.c_h + y) * pl.c_w + x0;
        const uint8_t* rn = ws + pl.cr + (f * pl.c_h + y) * pl.c_w + x0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cb[j] = bn[j];
            cr[j] = rn[j];
        }
    }
    uint8_t o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int Y = yrow[j], b = cb[j] - 128, r = cr[j] - 128;
        const int R = Y + ((91881 * r + 32768) >> 16), G = Y + ((-22554 * b - 46802 * r + 32768) >> 16), B = Y + ((116130 * b + 32768) >> 16);
        o[3 * j] = (uint8_t)(R < 0 ? 0 : R > 255 ? 255 : R);
        o[3 * j + 1] = (uint8_t)(G < 0 ? 0 : G > 255 ? 255 : G);
        o[3 * j + 2] = (uint8_t)(B < 0 ? 0 : B > 255 ? 255 : B);
    }
    const long off = ((f * H + y) * (long)W + x0) * 3;
    uint8_t* dst = rgb + off;
    if (x0 + 4 <= W && ((uintptr_t)dst & 3) == 0 && off + 12 <= rgb_bytes) {
#pragma unroll
        for (int w = 0; w < 3; ++w)
            ((uint32_t*)dst)[w] = (uint32_t)o[4 * w] | (uint32_t)o[4 * w + 1] << 8 | (uint32_t)o[4 * w + 2] << 16 | (uint32_t)o[4 * w + 3] << 24;
    } else {
        const int n = (W - x0 < 4 ? W - x0 : 4) * 3;
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < n && off + i < rgb_bytes) dst[i] = o[i];
    }
}

}  // namespace

extern "C" long tg_jpeg_huff_table_bytes(void) { return JD_TABLE_BYTES; }

extern "C" int tg_jpeg_huff_table(const void* bits, const void* vals, int n_vals, void* table) {
    TG_REQUIRE(bits && vals && table, TG_ERR_ARG, "tg_jpeg_huff_table: null pointer");
    TG_REQUIRE(((uintptr_t)table & 3) == 0, TG_ERR_ALIGN, "tg_jpeg_huff_table: table must be 4-byte aligned");
    const int r = jd_build_table((const uint8_t*)bits, (const uint8_t*)vals, n_vals, (JdHuffTable*)table);
    TG_REQUIRE(r != 1, TG_ERR_ARG, "tg_jpeg_huff_table: the code counts do not add up to the %d symbols (at most 256)", n_vals);
    TG_REQUIRE(r == 0, TG_ERR_ARG, "tg_jpeg_huff_table: an over-subscribed code (more codes of one length than that length has left)");
    return TG_OK;
}

extern "C" long tg_jpeg_decode_segments(int H, int W, int subsampling, int restart_interval) {
    Geometry g;
    if (!geometry(H, W, subsampling, g) || restart_interval < 0 || restart_interval > 65535) return 0;
    return segments_of(g, restart_interval);
}

extern "C" int tg_jpeg_find_segments(const void* data, long data_bytes, const void* scan_begin, const void* scan_end, int F, long n_seg, void* seg_begin, void* seg_end,
                                     void* status, hipStream_t stream) {
    TG_REQUIRE(data && scan_begin && scan_end && seg_begin && seg_end && status, TG_ERR_ARG, "tg_jpeg_find_segments: null pointer");
    TG_REQUIRE(data_bytes >= 1 && F >= 1 && F <= 65535 && n_seg >= 1 && n_seg <= (1L << 32), TG_ERR_SHAPE,
               "tg_jpeg_find_segments: bad shape data_bytes=%ld F=%d (1..65535) n_seg=%ld", data_bytes, F, n_seg);
    TG_REQUIRE((((uintptr_t)scan_begin | (uintptr_t)scan_end | (uintptr_t)seg_begin | (uintptr_t)seg_end) & 7) == 0 && ((uintptr_t)status & 3) == 0, TG_ERR_ALIGN,
               "tg_jpeg_find_segments: the byte ranges must be 8-byte aligned, status 4-byte");
    hipLaunchKernelGGL(jpeg_find_segments_kernel, dim3((unsigned)F), dim3(FS_THREADS), 0, stream, (const uint8_t*)data, data_bytes, (const long long*)scan_begin,
                       (const long long*)scan_end, n_seg, (long long*)seg_begin, (long long*)seg_end, (int32_t*)status);
    TG_LAUNCH_CHECK("tg_jpeg_find_segments");
    return TG_OK;
}

extern "C" int tg_jpeg_decode_coeffs(const void* data, long data_bytes, const void* seg_begin, const void* seg_end, int F, int H, int W, int subsampling,
                                     int restart_interval, const void* htabs, int n_sets, const void* htab_index, void* coef, void* status, hipStream_t stream) {
    TG_REQUIRE(data && seg_begin && seg_end && htabs && htab_index && coef && status, TG_ERR_ARG, "tg_jpeg_decode_coeffs: null pointer");
    TG_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, TG_ERR_ARG, "tg_jpeg_decode_coeffs: restart_interval must be in 0..65535 (got %d)", restart_interval);
    TG_REQUIRE(n_sets >= 1, TG_ERR_ARG, "tg_jpeg_decode_coeffs: at least one table set (got %d)", n_sets);
    Geometry g;
    TG_REQUIRE(data_bytes >= 1 && F >= 1 && F <= 65535 && geometry(H, W, subsampling, g), TG_ERR_SHAPE,
               "tg_jpeg_decode_coeffs: bad shape data_bytes=%ld F=%d (1..65535) H=%d W=%d (1..65535) subsampling=%d (420 or 444)", data_bytes, F, H, W, subsampling);
    TG_REQUIRE(tg_aligned16(coef) && (((uintptr_t)seg_begin | (uintptr_t)seg_end) & 7) == 0 && (((uintptr_t)htabs | (uintptr_t)htab_index | (uintptr_t)status) & 3) == 0,
               TG_ERR_ALIGN, "tg_jpeg_decode_coeffs: coef must be 16-byte aligned, the byte ranges 8-byte, tables, indices and status 4-byte");
    const long n_seg = segments_of(g, restart_interval), restart = restart_interval == 0 ? g.n_mcu : restart_interval;
    hipLaunchKernelGGL(jpeg_decode_coeffs_kernel, dim3((unsigned)((n_seg + 63) / 64), (unsigned)F), dim3(64), 0, stream, (const uint8_t*)data, data_bytes,
                       (const long long*)seg_begin, (const long long*)seg_end, n_seg, g.n_mcu, g.bpm, restart, (const uint32_t*)htabs, n_sets, (const int32_t*)htab_index,
                       (int16_t*)coef, (int32_t*)status);
    TG_LAUNCH_CHECK("tg_jpeg_decode_coeffs");
    return TG_OK;
}

extern "C" long tg_jpeg_idct_ws_bytes(int F, int H, int W, int subsampling) {
    Geometry g;
    if (F < 1 || !geometry(H, W, subsampling, g)) return 0;
    const Planes p = planes_of(g, F);
    return p.cr + F * p.c_w * p.c_h;
}

extern "C" int tg_jpeg_idct_rgb(const void* coef, int F, int H, int W, int subsampling, const void* qtabs, int n_qsets, const void* qtab_index, void* ws, long ws_bytes,
                                void* rgb, long rgb_bytes, hipStream_t stream) {
    TG_REQUIRE(coef && qtabs && qtab_index && ws && rgb, TG_ERR_ARG, "tg_jpeg_idct_rgb: null pointer");
    TG_REQUIRE(n_qsets >= 1, TG_ERR_ARG, "tg_jpeg_idct_rgb: at least one table set (got %d)", n_qsets);
    Geometry g;
    TG_REQUIRE(F >= 1 && geometry(H, W, subsampling, g), TG_ERR_SHAPE, "tg_jpeg_idct_rgb: bad shape F=%d H=%d W=%d (1..65535) subsampling=%d (420 or 444)", F, H, W,
               subsampling);
    TG_REQUIRE(ws_bytes >= tg_jpeg_idct_ws_bytes(F, H, W, subsampling), TG_ERR_SHAPE, "tg_jpeg_idct_rgb: the workspace needs %ld bytes (got %ld)",
               tg_jpeg_idct_ws_bytes(F, H, W, subsampling), ws_bytes);
    TG_REQUIRE(rgb_bytes >= 1, TG_ERR_SHAPE, "tg_jpeg_idct_rgb: rgb_bytes must be positive (got %ld)", rgb_bytes);
    TG_REQUIRE(tg_aligned16(coef) && tg_aligned16(ws) && (((uintptr_t)qtab_index) & 3) == 0 && ((uintptr_t)qtabs & 1) == 0, TG_ERR_ALIGN,
               "tg_jpeg_idct_rgb: coef and the workspace must be 16-byte aligned, qtab_index 4-byte, qtabs 2-byte");
    const long n_blocks = (long)F * g.n_mcu * g.bpm, grid1 = (n_blocks + 31) / 32;
    const int quads = (W + 3) / 4;
    const long total = (long)F * H * quads, grid2 = (total + 255) / 256;
    TG_REQUIRE(grid1 < (1L << 31) && grid2 < (1L << 31), TG_ERR_SHAPE, "tg_jpeg_idct_rgb: too many blocks");
    const Planes pl = planes_of(g, F);
    if (subsampling == 420) {
        hipLaunchKernelGGL(jpeg_idct_kernel<true>, dim3((unsigned)grid1), dim3(256), 0, stream, (const int16_t*)coef, n_blocks, g.n_mcu, g.cols, (const uint16_t*)qtabs,
                           n_qsets, (const int32_t*)qtab_index, pl, (uint8_t*)ws);
        TG_LAUNCH_CHECK("tg_jpeg_idct_rgb (planes)");
        hipLaunchKernelGGL(jpeg_rgb_kernel<true>, dim3((unsigned)grid2), dim3(256), 0, stream, (const uint8_t*)ws, pl, total, H, W, quads, (uint8_t*)rgb, rgb_bytes);
    } else {
        hipLaunchKernelGGL(jpeg_idct_kernel<false>, dim3((unsigned)grid1), dim3(256), 0, stream, (const int16_t*)coef, n_blocks, g.n_mcu, g.cols, (const uint16_t*)qtabs,
                           n_qsets, (const int32_t*)qtab_index, pl, (uint8_t*)ws);
        TG_LAUNCH_CHECK("tg_jpeg_idct_rgb (planes)");
        hipLaunchKernelGGL(jpeg_rgb_kernel<false>, dim3((unsigned)grid2), dim3(256), 0, stream, (const uint8_t*)ws, pl, total, H, W, quads, (uint8_t*)rgb, rgb_bytes);
    }
    TG_LAUNCH_CHECK("tg_jpeg_idct_rgb");
    return TG_OK;
}
