// The ViT image encoders' own kernels (transformers ViTModel and CLIPVisionModelWithProjection; host side: tokensgen_amd/vit.py) and the frame-consistency
// metric on their features (tokensgen_amd/metrics.py: video_consistency).  Every projection of an encoder, the patch convolution included, is tg_gemm_bf16
// with TG_EPI_BIAS; the attention is tg_t5_attention (head dimension 64, q pre-scaled by 1/8 at load, a zero bias table); the residual is tg_residual_add.
// What is here is the rest:
//   tg_vit_patch_rows        frames [F][3][H][W] -> the rows of the patch convolution seen as a GEMM, the preprocessing `(x + 1) / 2 -> (. - mean) / std` folded
//                            into one multiply-add per pixel.  One thread writes 8 columns (16 bytes); for p % 8 == 0 it reads them with one 16-byte load.
//   tg_vit_assemble          class token + patch embeddings + position embeddings -> the token sequence.  8 elements per thread.
//   tg_layernorm             nn.LayerNorm over the last dimension.  One wave per row, the row held in registers (D <= 4096), mean first, then the centred sum of
//                            squares, both in fp32 in a fixed order (a lane's elements in column order, then the lanes by butterfly).
//   tg_vit_act               exact GELU (erf) or quick GELU between the two GEMMs of the MLP.  8 elements per thread, the tail guarded.
//   tg_feature_consistency   max(0, cos) of every frame's feature with the previous frame's and with the first frame's, all sums in float64.  One wave per frame, a
//                            lane's elements in column order, then the lanes by butterfly: bitwise reproducible, and a frame's value depends on its three rows alone.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

__device__ __forceinline__ void vit_unpack8(const uint4& p, float* f) {
    f[0] = bf16lo_to_f32(p.x); f[1] = bf16hi_to_f32(p.x);
    f[2] = bf16lo_to_f32(p.y); f[3] = bf16hi_to_f32(p.y);
    f[4] = bf16lo_to_f32(p.z); f[5] = bf16hi_to_f32(p.z);
    f[6] = bf16lo_to_f32(p.w); f[7] = bf16hi_to_f32(p.w);
}

__device__ __forceinline__ uint4 vit_pack8(const float* o) {
    return uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
}

struct VitAffine { float a[3], b[3]; };

// ---- tg_vit_patch_rows: thread i writes columns 8 (i % Kp8) .. + 7 of row i / Kp8
template <bool VEC>
__global__ __launch_bounds__(256) void vit_patch_rows_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, long n8, int H, int W, int p, int Kp8, VitAffine af) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const long row = i / Kp8;
    const int k0 = (int)(i - row * Kp8) * 8, K = 3 * p * p;
    const int gw = W / p, gh = H / p;
    const int px = (int)(row % gw), py = (int)((row / gw) % gh);
    const long f = row / ((long)gw * gh);
    const bf16_t* img = x + f * 3L * H * W;
    float o[8];
    if (VEC) {                                                                // p % 8 == 0: the 8 columns are 8 consecutive pixels of one patch row, 16-byte aligned
        if (k0 < K) {                                                         // K % 8 == 0 here: the 8 columns are inside K or all pad
            const int c = k0 / (p * p), r = k0 - c * p * p, dy = r / p, dx = r - dy * p;
            float v[8];
            vit_unpack8(*(const uint4*)(img + ((long)c * H + py * p + dy) * W + px * p + dx), v);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = fmaf(v[k], af.a[c], af.b[c]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int kk = k0 + k;
            o[k] = 0.f;
            if (kk < K) {
                const int c = kk / (p * p), r = kk - c * p * p, dy = r / p, dx = r - dy * p;
                o[k] = fmaf(bf16_to_f32(img[((long)c * H + py * p + dy) * W + px * p + dx]), af.a[c], af.b[c]);
            }
        }
    }
    *(uint4*)(out + i * 8) = vit_pack8(o);
}

// ---- tg_vit_assemble: thread i writes elements 8 i .. 8 i + 7 of tok [F][S][D]
__global__ __launch_bounds__(256) void vit_assemble_kernel(const bf16_t* __restrict__ patch, const bf16_t* __restrict__ cls, const bf16_t* __restrict__ pos,
                                                           bf16_t* __restrict__ tok, long n8, int P, int D8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int c = (int)(i % D8) * 8;
    const long t = i / D8;                                                    // token index f * S + s
    const int S = P + 1, s = (int)(t % S);
    const long f = t / S;
    const bf16_t* src = s == 0 ? cls + c : patch + (f * P + (s - 1)) * (long)D8 * 8 + c;
    float a[8], b[8], o[8];
    vit_unpack8(*(const uint4*)src, a);
    vit_unpack8(*(const uint4*)(pos + (long)s * D8 * 8 + c), b);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = a[k] + b[k];
    *(uint4*)(tok + i * 8) = vit_pack8(o);
}

// ---- tg_layernorm: one wave per row, four rows per workgroup; the row stays in registers between the three passes
constexpr int LN_MAX_D = 4096;
constexpr int LN_CHUNKS = LN_MAX_D / 512;                                    // a wave covers 512 columns per step: 8 per lane

__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ w, const bf16_t* __restrict__ b,
                                                        bf16_t* __restrict__ y, long ldy, long rows, int D, float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                  // whole waves leave: no barrier below
    const int lane = threadIdx.x & 63;
    const bf16_t* xr = x + row * ldx;
    bf16_t* yr = y + row * ldy;
    float v[LN_CHUNKS][8];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < LN_CHUNKS; ++j) {
        const int c = j * 512 + lane * 8;                                     // D % 64 == 0 and c % 8 == 0: c < D means c + 8 <= D
        if (c < D) {
            vit_unpack8(*(const uint4*)(xr + c), v[j]);
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += v[j][k];
        }
    }
    const float mean = wave_sum(sum) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < LN_CHUNKS; ++j) {
        if (j * 512 + lane * 8 < D) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[j][k] -= mean;
                ss = fmaf(v[j][k], v[j][k], ss);
            }
        }
    }
    const float r = 1.f / sqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
    for (int j = 0; j < LN_CHUNKS; ++j) {
        const int c = j * 512 + lane * 8;
        if (c < D) {
            float g[8], h[8], o[8];
            vit_unpack8(*(const uint4*)(w + c), g);
            vit_unpack8(*(const uint4*)(b + c), h);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = fmaf(v[j][k] * r, g[k], h[k]);
            *(uint4*)(yr + c) = vit_pack8(o);
        }
    }
}

// ---- tg_vit_act
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * erfcf(-0.70710678118654752f * x); }      // 1 + erf(t) == erfc(-t), without the cancellation at -1
__device__ __forceinline__ float gelu_quick(float x) { return x / (1.f + expf(-1.702f * x)); }                  // exp -> inf: x / inf = -0

template <int MODE>
__global__ __launch_bounds__(256) void vit_act_kernel(const bf16_t* x, bf16_t* y, long n8) {   // y may be x
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;                                                      // the tail of the last workgroup
    float a[8], o[8];
    vit_unpack8(*(const uint4*)(x + i * 8), a);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = MODE == 0 ? gelu_erf(a[k]) : gelu_quick(a[k]);
    *(uint4*)(y + i * 8) = vit_pack8(o);
}

// ---- tg_feature_consistency: one wave per output frame
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void feature_consistency_kernel(const float* __restrict__ feat, long ld, int D, const float* __restrict__ first_row,
                                                                 const float* __restrict__ prev_row, int carried, double* __restrict__ prev_out,
                                                                 double* __restrict__ first_out) {
    const int o = blockIdx.x, lane = threadIdx.x;
    const int i = carried ? o : o + 1;                                        // the frame of this output: every frame with a carried pair, else every frame but the first
    const float* fi = feat + (long)i * ld;
    const float* fp = i == 0 ? prev_row : feat + (long)(i - 1) * ld;          // i == 0 only with a carried pair
    const float* ff = carried ? first_row : feat;
    double nii = 0., npp = 0., nff = 0., dip = 0., dif = 0.;
    for (int c = lane; c < D; c += 64) {
        const double a = (double)fi[c], p = (double)fp[c], f = (double)ff[c];
        nii = fma(a, a, nii); npp = fma(p, p, npp); nff = fma(f, f, nff);
        dip = fma(a, p, dip); dif = fma(a, f, dif);
    }
    nii = wave_sum_f64(nii); npp = wave_sum_f64(npp); nff = wave_sum_f64(nff);
    dip = wave_sum_f64(dip); dif = wave_sum_f64(dif);
    if (lane == 0) {
        // F.cosine_similarity: x . y / (max(|x|, eps) * max(|y|, eps)), eps = 1e-8: a zero row gives 0, not NaN
        const double eps = 1e-8, ni = fmax(sqrt(nii), eps);
        prev_out[o] = fmax(dip / (ni * fmax(sqrt(npp), eps)), 0.);
        first_out[o] = fmax(dif / (ni * fmax(sqrt(nff), eps)), 0.);
    }
}

}  // namespace

extern "C" int tg_vit_patch_rows(const void* x, int F, int H, int W, int p, const float* a, const float* b, void* out, int Kp, hipStream_t stream) {
    TG_REQUIRE(x && a && b && out, TG_ERR_ARG, "tg_vit_patch_rows: null pointer");
    TG_REQUIRE(F > 0 && H > 0 && W > 0 && p > 0 && p <= 256 && H % p == 0 && W % p == 0 && H <= 16384 && W <= 16384, TG_ERR_SHAPE,
               "tg_vit_patch_rows: need F >= 1 and H %% p == 0, W %% p == 0 with 1 <= p <= 256 (F=%d H=%d W=%d p=%d)", F, H, W, p);
    TG_REQUIRE(Kp == (3 * p * p + 63) / 64 * 64, TG_ERR_SHAPE, "tg_vit_patch_rows: Kp must be 3 p^2 rounded up to a multiple of 64 (p=%d: %d, got %d)", p,
               (3 * p * p + 63) / 64 * 64, Kp);
    TG_REQUIRE(tg_aligned16(x) && tg_aligned16(out), TG_ERR_ALIGN, "tg_vit_patch_rows: x and out must be 16-byte aligned");
    const long rows = (long)F * (H / p) * (W / p), n8 = rows * (Kp / 8);
    TG_REQUIRE(n8 < (1L << 39), TG_ERR_SHAPE, "tg_vit_patch_rows: too many elements");
    VitAffine af;
    for (int c = 0; c < 3; ++c) { af.a[c] = a[c]; af.b[c] = b[c]; }
    const dim3 grid((unsigned)((n8 + 255) / 256));
    if (p % 8 == 0)
        hipLaunchKernelGGL(vit_patch_rows_kernel<true>, grid, dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)out, n8, H, W, p, Kp / 8, af);
    else
        hipLaunchKernelGGL(vit_patch_rows_kernel<false>, grid, dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)out, n8, H, W, p, Kp / 8, af);
    TG_LAUNCH_CHECK("tg_vit_patch_rows");
    return TG_OK;
}

extern "C" int tg_vit_assemble(const void* patch, const void* cls, const void* pos, void* tok, int F, int P, int D, hipStream_t stream) {
    TG_REQUIRE(patch && cls && pos && tok, TG_ERR_ARG, "tg_vit_assemble: null pointer");
    TG_REQUIRE(F > 0 && P > 0 && D > 0 && D % 64 == 0, TG_ERR_SHAPE, "tg_vit_assemble: need F >= 1, P >= 1 and D %% 64 == 0 (F=%d P=%d D=%d)", F, P, D);
    TG_REQUIRE(tg_aligned16(patch) && tg_aligned16(cls) && tg_aligned16(pos) && tg_aligned16(tok), TG_ERR_ALIGN,
               "tg_vit_assemble: patch, cls, pos and tok must be 16-byte aligned");
    const long n8 = (long)F * (P + 1) * (D / 8);
    TG_REQUIRE(n8 < (1L << 39), TG_ERR_SHAPE, "tg_vit_assemble: too many elements");
    hipLaunchKernelGGL(vit_assemble_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)patch, (const bf16_t*)cls, (const bf16_t*)pos,
                       (bf16_t*)tok, n8, P, D / 8);
    TG_LAUNCH_CHECK("tg_vit_assemble");
    return TG_OK;
}

extern "C" int tg_layernorm(const void* x, long ldx, const void* w, const void* b, void* y, long ldy, long rows, int D, float eps, hipStream_t stream) {
    TG_REQUIRE(x && w && b && y, TG_ERR_ARG, "tg_layernorm: null pointer");
    TG_REQUIRE(rows > 0 && D > 0 && D % 64 == 0 && D <= LN_MAX_D && ldx >= D && ldy >= D && rows <= (1L << 31), TG_ERR_SHAPE,
               "tg_layernorm: need rows >= 1, D %% 64 == 0, D <= %d (the row stays in registers) and leading dimensions >= D (rows=%ld D=%d ldx=%ld ldy=%ld)", LN_MAX_D,
               rows, D, ldx, ldy);
    TG_REQUIRE(eps >= 0.f, TG_ERR_ARG, "tg_layernorm: eps must not be negative");
    TG_REQUIRE(tg_aligned16(x) && tg_aligned16(w) && tg_aligned16(b) && tg_aligned16(y) && ldx % 8 == 0 && ldy % 8 == 0, TG_ERR_ALIGN,
               "tg_layernorm: x, w, b and y must be 16-byte aligned, the leading dimensions multiples of 8");
    hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)x, ldx, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y,
                       ldy, rows, D, eps);
    TG_LAUNCH_CHECK("tg_layernorm");
    return TG_OK;
}

extern "C" int tg_vit_act(const void* x, void* y, long n, int mode, hipStream_t stream) {
    TG_REQUIRE(x && y, TG_ERR_ARG, "tg_vit_act: null pointer");
    TG_REQUIRE(mode == 0 || mode == 1, TG_ERR_ARG, "tg_vit_act: mode must be 0 (exact GELU) or 1 (quick GELU), got %d", mode);
    TG_REQUIRE(n > 0 && n % 8 == 0 && n / 8 < (1L << 39), TG_ERR_SHAPE, "tg_vit_act: n must be a positive multiple of 8 (got %ld)", n);
    TG_REQUIRE(tg_aligned16(x) && tg_aligned16(y), TG_ERR_ALIGN, "tg_vit_act: x and y must be 16-byte aligned");
    const dim3 grid((unsigned)((n / 8 + 255) / 256));
    if (mode == 0)
        hipLaunchKernelGGL(vit_act_kernel<0>, grid, dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, n / 8);
    else
        hipLaunchKernelGGL(vit_act_kernel<1>, grid, dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, n / 8);
    TG_LAUNCH_CHECK("tg_vit_act");
    return TG_OK;
}

extern "C" int tg_feature_consistency(const float* feat, long ld, int F, int D, const float* first_row, const float* prev_row, double* prev_out, double* first_out,
                                      hipStream_t stream) {
    TG_REQUIRE(feat && prev_out && first_out, TG_ERR_ARG, "tg_feature_consistency: null pointer");
    TG_REQUIRE((first_row == nullptr) == (prev_row == nullptr), TG_ERR_ARG, "tg_feature_consistency: the carried first and previous rows come together or not at all");
    const int carried = first_row != nullptr;
    TG_REQUIRE(F >= (carried ? 1 : 2) && D > 0 && ld >= D, TG_ERR_SHAPE,
               "tg_feature_consistency: need D >= 1, ld >= D and a frame with a predecessor: F >= 2, or F >= 1 with carried rows (F=%d D=%d ld=%ld)", F, D, ld);
    TG_REQUIRE((((uintptr_t)feat) & 3) == 0 && (((uintptr_t)first_row) & 3) == 0 && (((uintptr_t)prev_row) & 3) == 0 && (((uintptr_t)prev_out) & 7) == 0 &&
                   (((uintptr_t)first_out) & 7) == 0, TG_ERR_ALIGN, "tg_feature_consistency: features must be 4-byte aligned, the outputs 8-byte aligned");
    hipLaunchKernelGGL(feature_consistency_kernel, dim3((unsigned)(carried ? F : F - 1)), dim3(64), 0, stream, feat, ld, D, first_row, prev_row, carried, prev_out,
                       first_out);
    TG_LAUNCH_CHECK("tg_feature_consistency");
    return TG_OK;
}
