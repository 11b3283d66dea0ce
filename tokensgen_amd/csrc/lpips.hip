// LPIPS (VGG16, version 0.1) on channels-last bf16: what the trunk needs besides tg_conv3d_cl (host side: tokensgen_amd/lpips.py; the definition: DESIGN.md §8d).
//   tg_lpips_conv_in:     pixel ends + scaling layer + conv1_1 (3 -> 64, 3 x 3, zero padding 1) + bias + ReLU in one pass, bf16 [F][h][w][64] out.  Pixels are addressed by
//                         element strides like tg_image_metrics (outer image index, inner image index, channel, row, pixel): interleaved uint8 [.., H, W, 3], planar
//                         (n, 3, h, w), a [B, 3, T, H, W] view and a cropped rectangle are one code path and cost no copy.  A workgroup owns 16 x 16 output pixels of one
//                         image: it stages the 3 x 18 x 18 halo patch in LDS as fp32, each value formed in float64 — uint8: 2 f - 1 with f = v / 255 rounded to fp32 (so bytes and
//                         the fp32 frames `.float() / 255` with `normalize` give the same bits); floats: v, or 2 v - 1 with `normalize` — then (x - shift) / scale — and rounded once; a tap outside the image is 0 AFTER the scaling layer (the reference pads the scaled
//                         tensor, so the shift cannot be folded into the bias).  The 64 x 27 weights lie transposed in LDS ([27][64]: a wave reads the same 16 bytes —
//                         a broadcast).  A thread holds its pixel's 27 taps in registers and walks the 64 channels eight at a time: acc = bias, then 27 fused
//                         multiply-adds in the order (channel, row, column) = the weight's own order, ReLU, round to bf16, one 16-byte store.  1 728 fp32 FMAs per pixel.
//   tg_relu_cl:           ReLU in place, 16 bytes per thread.  Exact: a negative value becomes +0, everything else (-0.0 and NaN included) stays as it is — torch.relu.
//   tg_relu_maxpool2_cl:  y[f][i][j] = max over the 2 x 2 block of relu(x), floor mode (an odd last row / column is dropped).  Exact: the four values are compared as
//                         floats in the order (0,0) (0,1) (1,0) (1,1) and a later one wins only if it is greater (or NaN) — F.max_pool2d's own scan.
//   tg_lpips_head:        one tap of the LPIPS distance for all frames: per pixel the two channel norms, then sum_c w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2.
//                         A group of G = C / 8 lanes (a power of two, 8 .. 64) owns a pixel: a lane holds 8 channels of both features in registers (one 16-byte load
//                         each), squares and the lane's 8 terms are added in fp32, the group sums and everything after them in float64.  A workgroup owns 512 pixels of
//                         one frame; its sum (groups in pixel order, lanes by butterfly, the four waves in order) goes to a workspace and a second launch adds a frame's
//                         tiles in tile order: no atomics, a frame's value does not depend on the other frames.  Both features go through the same instructions, so
//                         fa == fb gives exactly 0 and swapping them gives the same bits; an all-zero vector gives 0 / 1e-10 = 0.
#include <math.h>

#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int LP_T = 16;                       // output pixels per tile side
constexpr int LP_P = LP_T + 2;                 // staged patch side
constexpr int LP_CO = 64;                      // conv1_1 output channels
constexpr int LP_K = 27;                       // 3 channels x 3 x 3 taps
constexpr int LP_HEAD_PIX = 512;               // pixels per workgroup of the head
__device__ __forceinline__ double lp_shift(int c) { return c == 0 ? -0.030 : c == 1 ? -0.088 : -0.188; }      // the scaling layer's constants
__device__ __forceinline__ double lp_scale(int c) { return c == 0 ? 0.458 : c == 1 ? 0.448 : 0.450; }

struct LpSrc { const void* p; long so, si, sc, sr, sp; };      // element strides: outer image index, inner image index, channel, row, pixel

template <int DT>                              // 0 uint8, 1 fp32, 2 bf16: the value in [-1, 1], float64
__device__ __forceinline__ double lp_load(const void* p, long off, bool normalize) {
    if constexpr (DT == 0) return 2.0 * (double)((float)((const uint8_t*)p)[off] / 255.0f) - 1.0;      // v / 255 as fp32 (IEEE division): the number `.float() / 255` holds
    else {
        double v;
        if constexpr (DT == 1) v = (double)((const float*)p)[off];
        else v = (double)bf16_to_f32(((const bf16_t*)p)[off]);
        return normalize ? 2.0 * v - 1.0 : v;
    }
}

template <int DT>
__global__ __launch_bounds__(256) void lpips_conv_in_kernel(LpSrc X, int n_inner, int h, int w, int tiles_x, int tiles_y, int normalize, const float* __restrict__ weight,
                                                            const float* __restrict__ bias, bf16_t* __restrict__ y) {
    __shared__ float patch[3][LP_P][LP_P];                      // 3 888 B
    __shared__ __attribute__((aligned(16))) float sw[LP_K][LP_CO];   // 6 912 B
    __shared__ __attribute__((aligned(16))) float sb[LP_CO];
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y, image = blk / tiles_y;
    const long io = image / n_inner, ii = image - io * n_inner;
    const int y0 = ty * LP_T, x0 = tx * LP_T;
    const long base = io * X.so + ii * X.si;

    for (int idx = tid; idx < LP_CO * LP_K; idx += 256) {       // weight [64][27] -> sw[27][64]
        const int co = idx / LP_K, k = idx - co * LP_K;
        sw[k][co] = weight[idx];
    }
    if (tid < LP_CO) sb[tid] = bias[tid];
    for (int idx = tid; idx < 3 * LP_P * LP_P; idx += 256) {
        const int c = idx / (LP_P * LP_P), rem = idx - c * (LP_P * LP_P), r = rem / LP_P, q = rem - r * LP_P;
        const int py = y0 + r - 1, px = x0 + q - 1;
        float v = 0.f;                                          // outside the image: zero in scaled space
        if (py >= 0 && py < h && px >= 0 && px < w) {
            const double d = lp_load<DT>(X.p, base + c * X.sc + (long)py * X.sr + (long)px * X.sp, normalize != 0);
            v = (float)((d - lp_shift(c)) / lp_scale(c));
        }
        patch[c][r][q] = v;
    }
    __syncthreads();

    const int ly = tid >> 4, lx = tid & 15;
    const int oy = y0 + ly, ox = x0 + lx;
    if (oy >= h || ox >= w) return;                             // no barrier below
    float xv[LP_K];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) xv[c * 9 + r * 3 + q] = patch[c][ly + r][lx + q];
    bf16_t* dst = y + (((long)image * h + oy) * w + ox) * LP_CO;
#pragma unroll 1
    for (int c0 = 0; c0 < LP_CO; c0 += 8) {
        float acc[8];
        const f32x4 b0 = *(const f32x4*)&sb[c0], b1 = *(const f32x4*)&sb[c0 + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = b0[j];
            acc[4 + j] = b1[j];
        }
#pragma unroll
        for (int k = 0; k < LP_K; ++k) {
            const f32x4 w0 = *(const f32x4*)&sw[k][c0], w1 = *(const f32x4*)&sw[k][c0 + 4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j] = fmaf(w0[j], xv[k], acc[j]);
                acc[4 + j] = fmaf(w1[j], xv[k], acc[4 + j]);
            }
        }
        uint4 o;
        o.x = pack_bf16x2(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f));
        o.y = pack_bf16x2(fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
        o.z = pack_bf16x2(fmaxf(acc[4], 0.f), fmaxf(acc[5], 0.f));
        o.w = pack_bf16x2(fmaxf(acc[6], 0.f), fmaxf(acc[7], 0.f));
        *(uint4*)(dst + c0) = o;
    }
}

// ReLU on raw bf16 bits: negative and not -0.0 -> +0
__device__ __forceinline__ uint32_t relu_bits(uint32_t b) { return ((b & 0x8000u) && (b & 0x7fffu) && (b & 0x7fffu) <= 0x7f80u) ? 0u : b; }
__device__ __forceinline__ uint32_t relu_pair(uint32_t v) { return relu_bits(v & 0xffffu) | (relu_bits(v >> 16) << 16); }
__device__ __forceinline__ uint4 relu_x8(uint4 v) { return uint4{relu_pair(v.x), relu_pair(v.y), relu_pair(v.z), relu_pair(v.w)}; }

__global__ __launch_bounds__(256) void relu_cl_kernel(uint4* __restrict__ x, long n16) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) x[i] = relu_x8(x[i]);
}

// F.max_pool2d's scan on one channel: the later value wins if it is greater or NaN
__device__ __forceinline__ uint32_t max_bits(uint32_t m, uint32_t v) {
    const float fm = bf16_to_f32((bf16_t)m), fv = bf16_to_f32((bf16_t)v);
    return (fv > fm || fv != fv) ? v : m;
}
__device__ __forceinline__ uint32_t max_pair(uint32_t m, uint32_t v) { return max_bits(m & 0xffffu, v & 0xffffu) | (max_bits(m >> 16, v >> 16) << 16); }
__device__ __forceinline__ uint4 max_x8(uint4 m, uint4 v) { return uint4{max_pair(m.x, v.x), max_pair(m.y, v.y), max_pair(m.z, v.z), max_pair(m.w, v.w)}; }

__global__ __launch_bounds__(256) void relu_maxpool2_kernel(const uint4* __restrict__ x, int H, int W, int C8, int Ho, int Wo, long n16, uint4* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const int c = (int)(i % C8);
    long v = i / C8;
    const int ox = (int)(v % Wo);
    v /= Wo;
    const int oy = (int)(v % Ho);
    const long f = v / Ho;
    const uint4* p = x + ((f * H + 2 * oy) * W + 2 * ox) * C8 + c;          // rows 2 oy, 2 oy + 1 < H and columns 2 ox, 2 ox + 1 < W: Ho = H / 2, Wo = W / 2
    uint4 m = relu_x8(p[0]);
    m = max_x8(m, relu_x8(p[C8]));
    m = max_x8(m, relu_x8(p[(long)W * C8]));
    m = max_x8(m, relu_x8(p[(long)W * C8 + C8]));
    y[i] = m;
}

__device__ __forceinline__ double group_sum_f64(double v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void head_unpack(uint4 v, bool relu, float (&f)[8]) {
    if (relu) v = relu_x8(v);
    f[0] = bf16lo_to_f32(v.x); f[1] = bf16hi_to_f32(v.x);
    f[2] = bf16lo_to_f32(v.y); f[3] = bf16hi_to_f32(v.y);
    f[4] = bf16lo_to_f32(v.z); f[5] = bf16hi_to_f32(v.z);
    f[6] = bf16lo_to_f32(v.w); f[7] = bf16hi_to_f32(v.w);
}

// one feature vector's lane share -> its 8 unit-normalised values (fp32), the norm from the group's float64 sum of the lanes' fp32 sums of squares
__device__ __forceinline__ void head_normalise(float (&f)[8], int G) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += f[j] * f[j];
    const float inv = 1.f / ((float)sqrt(group_sum_f64((double)s, G)) + 1e-10f);       // one division per vector: the 8 values take a multiplication each
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] * inv;
}

__global__ __launch_bounds__(256) void lpips_head_kernel(const uint4* __restrict__ fa, const uint4* __restrict__ fb, const float* __restrict__ w, long HW, int C, int G,
                                                         int relu, long tiles, double* __restrict__ ws) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int groups = 256 / G, g = tid / G, l = tid - g * G;
    const int C8 = C >> 3;
    float wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = w[l * 8 + j];                         // l < G = C / 8
    const long p_end = min(HW, (tile + 1) * LP_HEAD_PIX);
    double acc = 0.0;
    // every lane of a group walks the same pixels, so the shuffles inside see whole groups; G divides 64, so a group lies in one wave
    for (long p = tile * LP_HEAD_PIX + g; p < p_end; p += groups) {
        const long off = (frame * HW + p) * C8 + l;
        float a[8], b[8];
        head_unpack(fa[off], relu != 0, a);
        head_unpack(fb[off], relu != 0, b);
        head_normalise(a, G);
        head_normalise(b, G);
        float s = 0.f;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = a[j] - b[j];
                s += wv[j] * (d * d);
            }
        }
        acc += group_sum_f64((double)s, G);
    }
    if (l != 0) acc = 0.0;                                                     // every lane of a group holds the group's sum: count it once
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) ws[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per frame: lane l adds tiles l, l + 64, ... in that order, then the lanes by butterfly
__global__ __launch_bounds__(64) void lpips_head_finalize_kernel(const double* __restrict__ ws, long tiles, double* __restrict__ out) {
    const double* p = ws + (long)blockIdx.x * tiles;
    double s = 0.0;
    for (long t = threadIdx.x; t < tiles; t += 64) s += p[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

long head_tiles(long HW) { return (HW + LP_HEAD_PIX - 1) / LP_HEAD_PIX; }

}  // namespace

extern "C" int tg_lpips_conv_in(const void* x, long so, long si, long sc, long sr, long sp, int dtype, int normalize, int n_outer, int n_inner, int h, int w,
                                const float* weight, const float* bias, void* y, hipStream_t stream) {
    TG_REQUIRE(x && weight && bias && y, TG_ERR_ARG, "tg_lpips_conv_in: null pointer");
    TG_REQUIRE(dtype >= 0 && dtype <= 2 && (normalize == 0 || normalize == 1) && (dtype != 0 || normalize == 0), TG_ERR_ARG,
               "tg_lpips_conv_in: dtype in 0..2 and normalize in 0..1, 0 with uint8 (got %d, %d)", dtype, normalize);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && h >= 1 && w >= 1, TG_ERR_SHAPE, "tg_lpips_conv_in: bad shape n_outer=%d n_inner=%d h=%d w=%d", n_outer, n_inner, h, w);
    TG_REQUIRE(so >= 0 && si >= 0 && sc >= 0 && sr >= 0 && sp >= 0, TG_ERR_SHAPE, "tg_lpips_conv_in: negative stride");
    const unsigned elem = dtype == 0 ? 0u : dtype == 1 ? 3u : 1u;
    TG_REQUIRE(((uintptr_t)x & elem) == 0 && (((uintptr_t)weight | (uintptr_t)bias) & 3) == 0 && tg_aligned16(y), TG_ERR_ALIGN,
               "tg_lpips_conv_in: the input must be aligned to its element, weight and bias to 4 bytes, y to 16");
    const long tiles_x = (w + LP_T - 1) / LP_T, tiles_y = (h + LP_T - 1) / LP_T;
    const long grid = (long)n_outer * n_inner * tiles_x * tiles_y;
    TG_REQUIRE(grid < (1L << 31), TG_ERR_SHAPE, "tg_lpips_conv_in: too many tiles");
    const LpSrc X{x, so, si, sc, sr, sp};
#define TG_LPIPS_IN(DT) \
    hipLaunchKernelGGL(lpips_conv_in_kernel<DT>, dim3((unsigned)grid), dim3(256), 0, stream, X, n_inner, h, w, (int)tiles_x, (int)tiles_y, normalize, weight, bias, (bf16_t*)y)
    switch (dtype) {
        case 0: TG_LPIPS_IN(0); break;
        case 1: TG_LPIPS_IN(1); break;
        default: TG_LPIPS_IN(2); break;
    }
#undef TG_LPIPS_IN
    TG_LAUNCH_CHECK("tg_lpips_conv_in");
    return TG_OK;
}

extern "C" int tg_relu_cl(void* x, long n, hipStream_t stream) {
    TG_REQUIRE(x, TG_ERR_ARG, "tg_relu_cl: null pointer");
    TG_REQUIRE(n >= 8 && n % 8 == 0 && n / 8 < (1L << 39), TG_ERR_SHAPE, "tg_relu_cl: the element count must be a positive multiple of 8 (got %ld)", n);
    TG_REQUIRE(tg_aligned16(x), TG_ERR_ALIGN, "tg_relu_cl: x must be aligned to 16 bytes");
    const long n16 = n / 8;
    hipLaunchKernelGGL(relu_cl_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, stream, (uint4*)x, n16);
    TG_LAUNCH_CHECK("tg_relu_cl");
    return TG_OK;
}

extern "C" int tg_relu_maxpool2_cl(const void* x, int F, int H, int W, int C, void* y, hipStream_t stream) {
    TG_REQUIRE(x && y, TG_ERR_ARG, "tg_relu_maxpool2_cl: null pointer");
    TG_REQUIRE(F >= 1 && H >= 2 && W >= 2 && C >= 8 && C % 8 == 0, TG_ERR_SHAPE, "tg_relu_maxpool2_cl: need F >= 1, H, W >= 2 and C a positive multiple of 8 (F=%d H=%d W=%d C=%d)",
               F, H, W, C);
    TG_REQUIRE(tg_aligned16(x) && tg_aligned16(y), TG_ERR_ALIGN, "tg_relu_maxpool2_cl: x and y must be aligned to 16 bytes");
    const int Ho = H / 2, Wo = W / 2;
    const long n16 = (long)F * Ho * Wo * (C / 8);
    TG_REQUIRE(n16 < (1L << 39), TG_ERR_SHAPE, "tg_relu_maxpool2_cl: too many elements");
    hipLaunchKernelGGL(relu_maxpool2_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, stream, (const uint4*)x, H, W, C / 8, Ho, Wo, n16, (uint4*)y);
    TG_LAUNCH_CHECK("tg_relu_maxpool2_cl");
    return TG_OK;
}

extern "C" long tg_lpips_head_ws_doubles(int F, int H, int W) {
    if (F < 1 || H < 1 || W < 1) return 0;
    return (long)F * head_tiles((long)H * W);
}

extern "C" int tg_lpips_head(const void* fa, const void* fb, const float* w, int F, int H, int W, int C, int relu_on_load, double* ws, double* out, hipStream_t stream) {
    TG_REQUIRE(fa && fb && w && ws && out, TG_ERR_ARG, "tg_lpips_head: null pointer");
    TG_REQUIRE(relu_on_load == 0 || relu_on_load == 1, TG_ERR_ARG, "tg_lpips_head: relu_on_load in 0..1 (got %d)", relu_on_load);
    TG_REQUIRE(F >= 1 && H >= 1 && W >= 1 && (C == 64 || C == 128 || C == 256 || C == 512), TG_ERR_SHAPE,
               "tg_lpips_head: need F, H, W >= 1 and C in {64, 128, 256, 512} (F=%d H=%d W=%d C=%d)", F, H, W, C);
    TG_REQUIRE(tg_aligned16(fa) && tg_aligned16(fb) && ((uintptr_t)w & 3) == 0 && (((uintptr_t)ws | (uintptr_t)out) & 7) == 0, TG_ERR_ALIGN,
               "tg_lpips_head: fa and fb must be aligned to 16 bytes, w to 4, ws and out to 8");
    const long HW = (long)H * W, tiles = head_tiles(HW);
    TG_REQUIRE(F * tiles < (1L << 31), TG_ERR_SHAPE, "tg_lpips_head: too many tiles");
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)(F * tiles)), dim3(256), 0, stream, (const uint4*)fa, (const uint4*)fb, w, HW, C, C / 8, relu_on_load, tiles, ws);
    TG_LAUNCH_CHECK("tg_lpips_head");
    hipLaunchKernelGGL(lpips_head_finalize_kernel, dim3((unsigned)F), dim3(64), 0, stream, (const double*)ws, tiles, out);
    TG_LAUNCH_CHECK("tg_lpips_head (sum of the tiles)");
    return TG_OK;
}
