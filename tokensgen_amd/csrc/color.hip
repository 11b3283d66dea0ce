// Colour of the byte output: per-frame histograms, lookup tables that match a video's colour to an anchor, their application, and CIE L*a*b* sums.
//   tg_color_hist_u8:    per frame and channel the 256 counts of contiguous uint8 [F][H][W][3].  A frame is 3 H W bytes, in general no multiple of 16, so every frame
//                  has its own head (the bytes up to the first 16-byte boundary), body (aligned 16-byte loads) and tail; the channel of a byte is its index in the
//                  frame mod 3.  A workgroup owns a strip of 1 536 vectors (24 576 bytes) of one frame; a wave takes 192 vectors per round, a lane vectors l, l + 64
//                  and l + 128 of it: three loads in flight, and because 16 * 64 = 1 (mod 3) and 16 * 768 = 0 (mod 3) byte j of a lane's slot s has one channel in
//                  every round.  Each of the nine (slot, j mod 3) byte streams of a lane keeps a (bin, count) run and touches LDS only when the bin changes: noise
//                  pays one LDS add per byte as without it, a flat frame (the black bars of pad_to_fit) nine adds per lane and strip, so it is the cheap case, not
//                  the 64-way same-address one.  Every wave has its own [3][256] counts in LDS; the four are added and go to the output by integer atomics
//                  (order-independent: the result is exact), bins that are zero are skipped.  The output is zeroed by a launch of the call's own.
//   tg_color_match_lut:  one workgroup per frame and channel, thread v owns bin v: the causal window sum over the call's and the carried histograms in int64, the
//                  anchor's bin, then either the exact integer moments and the mean / std transfer in float64 (every operation rounded by itself), or the
//                  cumulative sums by a scan in LDS and a binary search for min{u : cr[u] ns >= cs[v] nr} in 64-bit integers.
//   tg_color_apply_lut:  out byte = table[channel][in byte].  The frame's 768-byte table sits in LDS, one channel every 296 bytes: 296 / 4 = 74 = 10 (mod 32), so the
//                  same value in the three channels (a grey pixel: the lanes of one ds_read_u8 hold all three channels) lies 10 and 20 banks apart instead of on one
//                  bank in three different dwords; values within a dword share an address and broadcast.  A workgroup owns 1 024 vectors of one frame, a lane four of
//                  them, loaded before the first gather.  Head, body and tail are cut by the OUTPUT address, so every body store is an aligned 16 bytes; the loads
//                  are aligned too whenever input and output are congruent mod 16 (always in place), otherwise they are 16 bytes of any alignment.
//   tg_lab_metrics:      OpenCV's documented floating-point RGB2Lab per pixel in float64, no fused multiply-add, for one or two inputs in the strided addressing of
//                  tg_image_metrics.  A workgroup owns 32 rows x 64 pixels, a thread eight pixels of one column; uint8 inputs read the sRGB curve from a 256-entry
//                  table the workgroup builds in LDS.  The sums are added over a thread's pixels in row order, over the lanes by butterfly, over the four waves in
//                  order, and a second launch adds a frame's tiles in tile order: no atomics, a frame's numbers depend on its own pixels alone.
#include <math.h>

#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int CH_STRIP = 1536;                  // histogram: 16-byte vectors per workgroup, two rounds of 4 waves x 192
constexpr int CA_STRIP = 1024;                  // apply: 16-byte vectors per workgroup, four per thread
constexpr int CA_PITCH = 296;                   // apply: bytes between the channels' tables in LDS
constexpr int CM_MAX_WINDOW = 64;

__global__ __launch_bounds__(256) void color_zero_kernel(int32_t* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// a frame's bytes [0, n) as head [0, head), vectors [head, head + 16 nvec) and tail, by the address `a` of byte 0
__device__ __forceinline__ void split16(uintptr_t a, long n, long& head, long& nvec) {
    head = (long)((0 - a) & 15);
    if (head > n) head = n;
    nvec = (n - head) >> 4;
}

// one byte of a run: the bin changes -> the finished run goes to LDS
__device__ __forceinline__ void hist_step(uint32_t* hw, uint32_t k, uint32_t& key, uint32_t& cnt) {
    if (k != key) {
        if (cnt) atomicAdd(&hw[key], cnt);      // key < 768
        key = k;
        cnt = 0;
    }
    ++cnt;
}

__global__ __launch_bounds__(256) void color_hist_kernel(const uint8_t* __restrict__ src, long frame_bytes, int strips, int32_t* __restrict__ out) {
    __shared__ uint32_t h[4][768];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long f = blockIdx.x / strips;
    const int strip = blockIdx.x - (int)(f * strips);
    for (int i = tid; i < 4 * 768; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    const uint8_t* p = src + f * frame_bytes;
    long head, nvec;
    split16((uintptr_t)p, frame_bytes, head, nvec);
    uint32_t* hw = h[wave];
    if (strip == 0 && wave == 0 && lane < 32) {                                 // the at most 15 + 15 bytes around the vectors: lanes 0 .. 15 the head, 16 .. 31 the tail
        const long i = lane < 16 ? lane : head + nvec * 16 + (lane - 16);
        if (lane < 16 ? i < head : i < frame_bytes) atomicAdd(&hw[(int)(i % 3) * 256 + p[i]], 1u);
    }
    const long v0 = (long)strip * CH_STRIP, v1 = nvec < v0 + CH_STRIP ? nvec : v0 + CH_STRIP;
    const uint4* pv = (const uint4*)(p + head);                                 // 16-byte aligned by the choice of head
    const long first = v0 + wave * 192 + lane;
    uint32_t off[3][3], key[3][3], cnt[3][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int phase = (int)((head + first + s) % 3);                        // channel of byte 0 of vector first + 64 s (+ 768 r): 16 = 64 = 1, 768 = 0 (mod 3)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            off[s][r] = (uint32_t)((phase + r) % 3) * 256u;
            key[s][r] = 0;
            cnt[s][r] = 0;
        }
    }
    for (long v = first; v < v1; v += 768) {
        uint4 x[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) x[s] = v + 64 * s < v1 ? pv[v + 64 * s] : make_uint4(0, 0, 0, 0);      // vector index < nvec: inside the frame
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (v + 64 * s < v1) {
                const uint32_t w[4] = {x[s].x, x[s].y, x[s].z, x[s].w};
#pragma unroll
                for (int j = 0; j < 16; ++j) hist_step(hw, off[s][j % 3] + ((w[j >> 2] >> (8 * (j & 3))) & 255u), key[s][j % 3], cnt[s][j % 3]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (cnt[s][r]) atomicAdd(&hw[key[s][r]], cnt[s][r]);
    __syncthreads();
    for (int i = tid; i < 768; i += 256) {
        const uint32_t s = h[0][i] + h[1][i] + h[2][i] + h[3][i];
        if (s) atomicAdd(&out[f * 768 + i], (int32_t)s);
    }
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Moments { double mean, std; };

// mean and standard deviation from the exact integer moments, each operation rounded by itself in this order
__device__ __forceinline__ Moments moments_of(long long n, long long s1, long long s2) {
#pragma clang fp contract(off)
    Moments m;
    m.mean = (double)s1 / (double)n;
    const double ex2 = (double)s2 / (double)n;
    const double d = ex2 - m.mean * m.mean;
    m.std = sqrt(fmax(d, 0.0));
    return m;
}

__device__ __forceinline__ double meanstd_map(int v, Moments src, Moments ref, double strength, double inv_gain, double max_gain) {
#pragma clang fp contract(off)
    double g = src.std > 0.0 ? ref.std / src.std : 1.0;
    g = fmin(fmax(g, inv_gain), max_gain);
    const double g2 = 1.0 + strength * (g - 1.0);
    const double m2 = src.mean + strength * (ref.mean - src.mean);
    return rint(((double)v - src.mean) * g2 + m2);
}

__device__ __forceinline__ double histogram_map(int v, int m, double strength) {
#pragma clang fp contract(off)
    return rint((double)v + strength * (double)(m - v));
}

// mode 0 meanstd, 1 histogram.  Thread v owns bin v of frame f, channel c.
__global__ __launch_bounds__(256) void color_match_lut_kernel(const int32_t* __restrict__ hist, const int32_t* __restrict__ history, int n_hist,
                                                              const long long* __restrict__ anchor, int mode, double strength, int window, double inv_gain,
                                                              double max_gain, uint8_t* __restrict__ lut, int* __restrict__ status) {
    __shared__ long long scan[2][2][256];       // [source | anchor][ping | pong][bin]
    __shared__ long long red[6][4];
    const int v = threadIdx.x, f = blockIdx.x / 3, c = blockIdx.x - 3 * f;
    long long s = 0;
    bool bad = false;
    for (int k = f - window + 1; k <= f; ++k) {                                 // frame k of the call, or frame n_hist + k of the carried ones; before those: the video's start
        int x = 0;
        if (k >= 0) x = hist[((long)k * 3 + c) * 256 + v];
        else if (n_hist + k >= 0) x = history[((long)(n_hist + k) * 3 + c) * 256 + v];
        bad = bad || x < 0;
        s += x;
    }
    const long long r = anchor[c * 256 + v];
    bad = bad || r < 0;
    int m = v;                                                                  // histogram mode: the matched bin
    long long ns, nr, q[6] = {s, (long long)v * s, (long long)v * v * s, r, (long long)v * r, (long long)v * v * r};
    if (mode == 1) {
        scan[0][0][v] = s;
        scan[1][0][v] = r;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < 256; d <<= 1) {                                     // inclusive scan, eight rounds
            const long long a = scan[0][cur][v] + (v >= d ? scan[0][cur][v - d] : 0), b = scan[1][cur][v] + (v >= d ? scan[1][cur][v - d] : 0);
            scan[0][cur ^ 1][v] = a;
            scan[1][cur ^ 1][v] = b;
            cur ^= 1;
            __syncthreads();
        }
        ns = scan[0][cur][255];
        nr = scan[1][cur][255];
        bad = bad || ns <= 0 || nr <= 0 || ns >= (1LL << 31) || nr >= (1LL << 31);
        if (!__syncthreads_or(bad)) {
            const long long want = scan[0][cur][v] * nr;                        // < 2^62
            int lo = 0, hi = 255;                                               // cr[255] ns = nr ns >= want: the answer exists
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (scan[1][cur][mid] * ns >= want) hi = mid;
                else lo = mid + 1;
            }
            m = lo;
            bad = false;
        } else {
            bad = true;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) q[i] = wave_sum_i64(q[i]);
        if ((v & 63) == 0)
#pragma unroll
            for (int i = 0; i < 6; ++i) red[i][v >> 6] = q[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 6; ++i) q[i] = red[i][0] + red[i][1] + red[i][2] + red[i][3];
        ns = q[0];
        nr = q[3];
        bad = __syncthreads_or(bad || ns <= 0 || nr <= 0 || ns >= (1LL << 31) || nr >= (1LL << 31));
    }
    double o = (double)v;                                                       // a refused histogram leaves the identity table
    if (!bad) o = mode == 1 ? histogram_map(v, m, strength) : meanstd_map(v, moments_of(ns, q[1], q[2]), moments_of(nr, q[4], q[5]), strength, inv_gain, max_gain);
    lut[(long)blockIdx.x * 256 + v] = (uint8_t)(int)fmin(fmax(o, 0.0), 255.0);
    if (bad && v == 0) atomicAdd(status, 1);
}

__global__ __launch_bounds__(256) void color_apply_kernel(const uint8_t* src, const uint8_t* __restrict__ lut, uint8_t* dst, long frame_bytes, int strips) {
    __shared__ uint32_t tab32[3 * CA_PITCH / 4];
    const int tid = threadIdx.x;
    const long f = blockIdx.x / strips;
    const int strip = blockIdx.x - (int)(f * strips);
    if (tid < 192) tab32[(tid >> 6) * (CA_PITCH / 4) + (tid & 63)] = ((const uint32_t*)(lut + f * 768))[tid];       // lut is 4-byte aligned, 768 a multiple of 4
    __syncthreads();
    const uint8_t* tab = (const uint8_t*)tab32;
    const uint8_t* p = src + f * frame_bytes;
    uint8_t* q = dst + f * frame_bytes;
    long head, nvec;
    split16((uintptr_t)q, frame_bytes, head, nvec);
    if (strip == 0 && tid < 32) {                                               // head and tail bytes, as in the histogram
        const long i = tid < 16 ? tid : head + nvec * 16 + (tid - 16);
        if (tid < 16 ? i < head : i < frame_bytes) q[i] = tab[(int)(i % 3) * CA_PITCH + p[i]];
    }
    const long v0 = (long)strip * CA_STRIP, v1 = nvec < v0 + CA_STRIP ? nvec : v0 + CA_STRIP;
    const bool in_aligned = (((uintptr_t)p + head) & 15) == 0;                  // uniform over the frame
    uint4 x[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const long v = v0 + it * 256 + tid;
        x[it] = make_uint4(0, 0, 0, 0);
        if (v < v1) {                                                           // bytes head + 16 v .. + 15 < frame_bytes
            if (in_aligned) x[it] = *(const uint4*)(p + head + 16 * v);
            else __builtin_memcpy(&x[it], p + head + 16 * v, 16);
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const long v = v0 + it * 256 + tid;
        if (v < v1) {
            const int phase = (int)((head + v) % 3);                            // channel of byte 0 of the vector: 16 = 1 (mod 3)
            const int o[3] = {phase * CA_PITCH, ((phase + 1) % 3) * CA_PITCH, ((phase + 2) % 3) * CA_PITCH};
            const uint32_t w[4] = {x[it].x, x[it].y, x[it].z, x[it].w};
            uint32_t y[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) y[j >> 2] |= (uint32_t)tab[o[j % 3] + ((w[j >> 2] >> (8 * (j & 3))) & 255u)] << (8 * (j & 3));
            *(uint4*)(q + head + 16 * v) = make_uint4(y[0], y[1], y[2], y[3]);
        }
    }
}

constexpr int LAB_TH = 32, LAB_TW = 64;         // a tile: 32 rows x 64 pixels, eight pixels of one column per thread

struct LabSrc { const void* p; long so, si, sc, sr, sp; };       // element strides: outer image index, inner image index, channel, row, pixel
struct Lab { double L, a, b, C; };

// sRGB -> linear, c in [0, 1]
__device__ __forceinline__ double srgb_linear(double c) {
#pragma clang fp contract(off)
    return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
}

template <int DT>                               // 0 uint8, 1 fp32, 2 bf16: the linear value of one channel
__device__ __forceinline__ double lab_load(const void* p, long off, const double* tab) {
    if constexpr (DT == 0) {
        return tab[((const uint8_t*)p)[off]];
    } else {
        const double v = DT == 1 ? (double)((const float*)p)[off] : (double)bf16_to_f32(((const bf16_t*)p)[off]);
        return srgb_linear(fmin(fmax(v, 0.0), 1.0));                            // a NaN counts as 0
    }
}

__device__ __forceinline__ double lab_f(double t) {
#pragma clang fp contract(off)
    return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0;
}

// OpenCV's documented floating-point RGB2Lab from linear R, G, B, every operation rounded by itself
__device__ __forceinline__ Lab lab_of(double r, double g, double b) {
#pragma clang fp contract(off)
    const double X = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.950456;
    const double Y = 0.212671 * r + 0.715160 * g + 0.072169 * b;
    const double Z = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.088754;
    const double fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    Lab o;
    o.L = Y > 0.008856 ? 116.0 * cbrt(Y) - 16.0 : 903.3 * Y;
    o.a = 500.0 * (fx - fy);
    o.b = 200.0 * (fy - fz);
    o.C = sqrt(o.a * o.a + o.b * o.b);
    return o;
}

__device__ __forceinline__ double delta_e76(const Lab& p, const Lab& q) {
#pragma clang fp contract(off)
    const double dL = p.L - q.L, da = p.a - q.a, db = p.b - q.b;
    return sqrt(dL * dL + da * da + db * db);
}

template <int DT>
__device__ __forceinline__ Lab lab_pixel(const LabSrc& s, long off, const double* tab) {
    return lab_of(lab_load<DT>(s.p, off, tab), lab_load<DT>(s.p, off + s.sc, tab), lab_load<DT>(s.p, off + 2 * s.sc, tab));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int DT, bool TWO>
__global__ __launch_bounds__(256) void lab_metrics_kernel(LabSrc A, LabSrc B, int n_inner, int h, int w, int tiles_x, int tiles_y, double* __restrict__ ws) {
    constexpr int NS = TWO ? 9 : 4;
    __shared__ double tab[256];
    __shared__ double red[NS][4];
    const int tid = threadIdx.x;
    if constexpr (DT == 0) {
        tab[tid] = srgb_linear((double)tid / 255.0);
        __syncthreads();
    }
    long blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x);
    blk /= tiles_x;
    const int ty = (int)(blk % tiles_y);
    const long image = blk / tiles_y, io = image / n_inner, ii = image - io * n_inner;
    const int x = tx * LAB_TW + (tid & 63), y0 = ty * LAB_TH + (tid >> 6);
    const long base_a = io * A.so + ii * A.si + (long)x * A.sp, base_b = TWO ? io * B.so + ii * B.si + (long)x * B.sp : 0;
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
    if (x < w) {
#pragma unroll 2
        for (int k = 0; k < LAB_TH / 4; ++k) {
            const int y = y0 + 4 * k;
            if (y < h) {                                                        // 0 <= y < h, 0 <= x < w
                const Lab p = lab_pixel<DT>(A, base_a + (long)y * A.sr, tab);
                acc[0] += p.L;
                acc[1] += p.a;
                acc[2] += p.b;
                acc[3] += p.C;
                if constexpr (TWO) {
                    const Lab q = lab_pixel<DT>(B, base_b + (long)y * B.sr, tab);
                    acc[4] += q.L;
                    acc[5] += q.a;
                    acc[6] += q.b;
                    acc[7] += q.C;
                    acc[8] += delta_e76(p, q);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = wave_sum_f64(acc[q]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < NS; ++q) red[q][tid >> 6] = acc[q];
    __syncthreads();
    if (tid < NS) ws[((image * tiles_y + ty) * tiles_x + tx) * NS + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// one wave per frame: lane l adds tiles l, l + 64, ... in that order, then the lanes by butterfly
__global__ __launch_bounds__(64) void lab_metrics_finalize_kernel(const double* __restrict__ ws, long tiles, int ns, double* __restrict__ out) {
    const long image = blockIdx.x;
    const double* p = ws + image * tiles * ns;
    for (int q = 0; q < ns; ++q) {
        double s = 0.0;
        for (long t = threadIdx.x; t < tiles; t += 64) s += p[t * ns + q];
        s = wave_sum_f64(s);
        if (threadIdx.x == 0) out[image * ns + q] = s;
    }
}

template <int DT>
void launch_lab(bool two, unsigned grid, hipStream_t stream, const LabSrc& A, const LabSrc& B, int n_inner, int h, int w, int tiles_x, int tiles_y, double* ws) {
    if (two) hipLaunchKernelGGL((lab_metrics_kernel<DT, true>), dim3(grid), dim3(256), 0, stream, A, B, n_inner, h, w, tiles_x, tiles_y, ws);
    else hipLaunchKernelGGL((lab_metrics_kernel<DT, false>), dim3(grid), dim3(256), 0, stream, A, B, n_inner, h, w, tiles_x, tiles_y, ws);
}

long strips_of(long frame_bytes, int strip) {
    const long n = ((frame_bytes >> 4) + strip - 1) / strip;
    return n > 1 ? n : 1;
}

}  // namespace

extern "C" long tg_color_strip_bytes(int which) { return which == 0 ? 16L * CH_STRIP : which == 1 ? 16L * CA_STRIP : 0; }

extern "C" int tg_color_hist_u8(const void* src, int F, int H, int W, void* hist, hipStream_t stream) {
    TG_REQUIRE(src && hist, TG_ERR_ARG, "tg_color_hist_u8: null pointer");
    TG_REQUIRE(F >= 1 && H >= 1 && W >= 1 && (long)H * W < (1L << 31), TG_ERR_SHAPE, "tg_color_hist_u8: bad shape F=%d H=%d W=%d (a frame must stay below 2^31 pixels)", F, H, W);
    TG_REQUIRE(((uintptr_t)hist & 3) == 0, TG_ERR_ALIGN, "tg_color_hist_u8: hist must be 4-byte aligned");
    const long frame_bytes = 3L * H * W, strips = strips_of(frame_bytes, CH_STRIP), n = 768L * F;
    TG_REQUIRE(strips * F < (1L << 31), TG_ERR_SHAPE, "tg_color_hist_u8: too many strips");
    hipLaunchKernelGGL(color_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (int32_t*)hist, n);
    TG_LAUNCH_CHECK("tg_color_hist_u8 (zero)");
    hipLaunchKernelGGL(color_hist_kernel, dim3((unsigned)(strips * F)), dim3(256), 0, stream, (const uint8_t*)src, frame_bytes, (int)strips, (int32_t*)hist);
    TG_LAUNCH_CHECK("tg_color_hist_u8");
    return TG_OK;
}

extern "C" int tg_color_match_lut(const void* hist, int F, const void* history, int n_history, const void* anchor, int mode, double strength, int window,
                                  double max_gain, void* lut, int* status, hipStream_t stream) {
    TG_REQUIRE(hist && anchor && lut && status, TG_ERR_ARG, "tg_color_match_lut: null pointer");
    TG_REQUIRE(mode == 0 || mode == 1, TG_ERR_ARG, "tg_color_match_lut: mode must be 0 (meanstd) or 1 (histogram), got %d", mode);
    TG_REQUIRE(strength >= 0.0 && strength <= 1.0 && max_gain >= 1.0 && max_gain < HUGE_VAL, TG_ERR_ARG,
               "tg_color_match_lut: strength must be in [0, 1] and max_gain finite and >= 1 (got %g, %g)", strength, max_gain);
    TG_REQUIRE(window >= 1 && window <= CM_MAX_WINDOW, TG_ERR_ARG, "tg_color_match_lut: window must be in 1..%d (got %d)", CM_MAX_WINDOW, window);
    TG_REQUIRE(F >= 1 && F < (1 << 29), TG_ERR_SHAPE, "tg_color_match_lut: bad frame count %d", F);
    TG_REQUIRE(n_history >= 0 && n_history < window && (n_history == 0 || history), TG_ERR_SHAPE,
               "tg_color_match_lut: 0 .. window - 1 carried histograms, with their pointer (got %d, window %d)", n_history, window);
    TG_REQUIRE((((uintptr_t)hist | (uintptr_t)history | (uintptr_t)status) & 3) == 0 && ((uintptr_t)anchor & 7) == 0, TG_ERR_ALIGN,
               "tg_color_match_lut: hist, history and status must be 4-byte aligned, anchor 8-byte");
    hipLaunchKernelGGL(color_match_lut_kernel, dim3(3u * (unsigned)F), dim3(256), 0, stream, (const int32_t*)hist, (const int32_t*)history, n_history,
                       (const long long*)anchor, mode, strength, window, 1.0 / max_gain, max_gain, (uint8_t*)lut, status);
    TG_LAUNCH_CHECK("tg_color_match_lut");
    return TG_OK;
}

extern "C" int tg_color_apply_lut(const void* src, const void* lut, int F, int H, int W, void* dst, hipStream_t stream) {
    TG_REQUIRE(src && lut && dst, TG_ERR_ARG, "tg_color_apply_lut: null pointer");
    TG_REQUIRE(F >= 1 && H >= 1 && W >= 1 && (long)H * W < (1L << 31), TG_ERR_SHAPE, "tg_color_apply_lut: bad shape F=%d H=%d W=%d (a frame must stay below 2^31 pixels)", F, H, W);
    TG_REQUIRE(((uintptr_t)lut & 3) == 0, TG_ERR_ALIGN, "tg_color_apply_lut: lut must be 4-byte aligned");
    const long frame_bytes = 3L * H * W, strips = strips_of(frame_bytes, CA_STRIP);
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, total = (uintptr_t)(frame_bytes * F);
    TG_REQUIRE(a == b || a + total <= b || b + total <= a, TG_ERR_ARG, "tg_color_apply_lut: src and dst must be the same buffer or not overlap");
    TG_REQUIRE(strips * F < (1L << 31), TG_ERR_SHAPE, "tg_color_apply_lut: too many strips");
    hipLaunchKernelGGL(color_apply_kernel, dim3((unsigned)(strips * F)), dim3(256), 0, stream, (const uint8_t*)src, (const uint8_t*)lut, (uint8_t*)dst, frame_bytes,
                       (int)strips);
    TG_LAUNCH_CHECK("tg_color_apply_lut");
    return TG_OK;
}

extern "C" long tg_lab_metrics_tile(int axis) { return axis == 0 ? LAB_TH : axis == 1 ? LAB_TW : 0; }

extern "C" long tg_lab_metrics_ws_doubles(long frames, int h, int w, int two) {
    if (frames < 1 || h < 1 || w < 1) return 0;
    return frames * ((h + LAB_TH - 1) / LAB_TH) * ((w + LAB_TW - 1) / LAB_TW) * (two ? 9 : 4);
}

extern "C" int tg_lab_metrics(const void* a, long a_so, long a_si, long a_sc, long a_sr, long a_sp, const void* b, long b_so, long b_si, long b_sc, long b_sr, long b_sp,
                              int dtype, int n_outer, int n_inner, int h, int w, double* ws, double* out, hipStream_t stream) {
    TG_REQUIRE(a && ws && out, TG_ERR_ARG, "tg_lab_metrics: null pointer");
    TG_REQUIRE(dtype >= 0 && dtype <= 2, TG_ERR_ARG, "tg_lab_metrics: dtype in 0..2 (got %d)", dtype);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && h >= 1 && w >= 1, TG_ERR_SHAPE, "tg_lab_metrics: bad shape n_outer=%d n_inner=%d h=%d w=%d", n_outer, n_inner, h, w);
    TG_REQUIRE(a_so >= 0 && a_si >= 0 && a_sc >= 0 && a_sr >= 0 && a_sp >= 0 && b_so >= 0 && b_si >= 0 && b_sc >= 0 && b_sr >= 0 && b_sp >= 0, TG_ERR_SHAPE,
               "tg_lab_metrics: negative stride");
    const unsigned elem = dtype == 0 ? 0u : dtype == 1 ? 3u : 1u;
    TG_REQUIRE((((uintptr_t)a | (uintptr_t)b) & elem) == 0 && (((uintptr_t)ws | (uintptr_t)out) & 7) == 0, TG_ERR_ALIGN,
               "tg_lab_metrics: the inputs must be aligned to their element, ws and out to 8 bytes");
    const long frames = (long)n_outer * n_inner, tiles_x = (w + LAB_TW - 1) / LAB_TW, tiles_y = (h + LAB_TH - 1) / LAB_TH;
    TG_REQUIRE(frames * tiles_x * tiles_y < (1L << 31), TG_ERR_SHAPE, "tg_lab_metrics: too many tiles");
    const LabSrc A{a, a_so, a_si, a_sc, a_sr, a_sp}, B{b, b_so, b_si, b_sc, b_sr, b_sp};
    const unsigned grid = (unsigned)(frames * tiles_x * tiles_y);
    switch (dtype) {
        case 0: launch_lab<0>(b != nullptr, grid, stream, A, B, n_inner, h, w, (int)tiles_x, (int)tiles_y, ws); break;
        case 1: launch_lab<1>(b != nullptr, grid, stream, A, B, n_inner, h, w, (int)tiles_x, (int)tiles_y, ws); break;
        default: launch_lab<2>(b != nullptr, grid, stream, A, B, n_inner, h, w, (int)tiles_x, (int)tiles_y, ws); break;
    }
    TG_LAUNCH_CHECK("tg_lab_metrics");
    hipLaunchKernelGGL(lab_metrics_finalize_kernel, dim3((unsigned)frames), dim3(64), 0, stream, ws, tiles_x * tiles_y, b ? 9 : 4, out);
    TG_LAUNCH_CHECK("tg_lab_metrics (sum of the tiles)");
    return TG_OK;
}
