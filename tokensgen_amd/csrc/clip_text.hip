// The CLIP text tower's own kernels (transformers CLIPTextModelWithProjection; host side: tokensgen_amd/clip_text.py) and the text-video alignment on its
// features (tokensgen_amd/metrics.py: video_text_alignment).  Every projection of the tower is tg_gemm_bf16 with TG_EPI_BIAS; the LayerNorms are tg_layernorm, the
// activation tg_vit_act, the residual tg_residual_add (csrc/vit.hip, csrc/t5.hip); the causal self-attention is tg_t5_attention with q pre-scaled by 1/8 at load
// and a bias-by-distance table that is 0 for j - i <= 0 and -inf for j - i > 0.  What is here is the rest:
//   tg_text_embed        token embedding gather + learned position embedding -> the token sequence.  One thread writes 8 columns (16 bytes) of one row; an id
//                        outside [0, V) never becomes an address: its row is written as zeros and the caller's status word counts it.
//   tg_text_alignment    cos(image feature f, text feature k) for every frame and every text, all sums in float64.  One wave per frame, a lane's elements in
//                        column order, then the lanes by butterfly: bitwise reproducible, and an output depends on its two rows alone.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

__device__ __forceinline__ void ct_unpack8(const uint4& p, float* f) {
    f[0] = bf16lo_to_f32(p.x); f[1] = bf16hi_to_f32(p.x);
    f[2] = bf16lo_to_f32(p.y); f[3] = bf16hi_to_f32(p.y);
    f[4] = bf16lo_to_f32(p.z); f[5] = bf16hi_to_f32(p.z);
    f[6] = bf16lo_to_f32(p.w); f[7] = bf16hi_to_f32(p.w);
}

// ---- tg_text_embed: thread i writes columns 8 (i % D8) .. + 7 of row i / D8
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, long n8, int S, const bf16_t* __restrict__ tok, int V,
                                                         const bf16_t* __restrict__ pos, bf16_t* __restrict__ out, long ldo, int D8, int* __restrict__ status) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;                                                      // the tail of the last workgroup
    const long row = i / D8;
    const int c = (int)(i - row * D8) * 8;
    const int id = ids[row];
    uint4 o = uint4{0u, 0u, 0u, 0u};
    if (id >= 0 && id < V) {                                                  // the only use of id as an index
        float a[8], b[8];
        ct_unpack8(*(const uint4*)(tok + (long)id * D8 * 8 + c), a);
        ct_unpack8(*(const uint4*)(pos + (row % S) * D8 * 8 + c), b);         // row % S < S: inside pos [S][D]
        o = uint4{pack_bf16x2(a[0] + b[0], a[1] + b[1]), pack_bf16x2(a[2] + b[2], a[3] + b[3]), pack_bf16x2(a[4] + b[4], a[5] + b[5]),
                  pack_bf16x2(a[6] + b[6], a[7] + b[7])};
    } else if (c == 0) {
        atomicAdd(status, 1);                                                 // once per refused row
    }
    *(uint4*)(out + row * ldo + c) = o;
}

// ---- tg_text_alignment: one wave per frame, the texts in turn
__device__ __forceinline__ double ct_wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void text_alignment_kernel(const float* __restrict__ img, long ld_img, const float* __restrict__ txt, long ld_txt, int K, int D,
                                                            double* __restrict__ cos_out) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const float* x = img + (long)f * ld_img;
    double nxx = 0.;
    for (int c = lane; c < D; c += 64) {
        const double a = (double)x[c];
        nxx = fma(a, a, nxx);
    }
    const double eps = 1e-8, nx = fmax(sqrt(ct_wave_sum_f64(nxx)), eps);
    for (int k = 0; k < K; ++k) {
        const float* y = txt + (long)k * ld_txt;
        double nyy = 0., dxy = 0.;
        for (int c = lane; c < D; c += 64) {
            const double a = (double)x[c], b = (double)y[c];
            nyy = fma(b, b, nyy);
            dxy = fma(a, b, dxy);
        }
        nyy = ct_wave_sum_f64(nyy);
        dxy = ct_wave_sum_f64(dxy);
        // F.cosine_similarity: x . y / (max(|x|, eps) * max(|y|, eps)): a zero row gives 0, not NaN
        if (lane == 0) cos_out[(long)f * K + k] = dxy / (nx * fmax(sqrt(nyy), eps));
    }
}

}  // namespace

extern "C" int tg_text_embed(const int* ids, long rows, int S, const void* tok_emb, int V, const void* pos_emb, void* out, long ldo, int D, int* status,
                             hipStream_t stream) {
    TG_REQUIRE(ids && tok_emb && pos_emb && out && status, TG_ERR_ARG, "tg_text_embed: null pointer");
    TG_REQUIRE(rows > 0 && S > 0 && V > 0 && D > 0 && D % 8 == 0 && ldo >= D && rows <= (1L << 31), TG_ERR_SHAPE,
               "tg_text_embed: need rows >= 1, S >= 1, V >= 1, D %% 8 == 0 and ldo >= D (rows=%ld S=%d V=%d D=%d ldo=%ld)", rows, S, V, D, ldo);
    TG_REQUIRE(tg_aligned16(tok_emb) && tg_aligned16(pos_emb) && tg_aligned16(out) && ldo % 8 == 0 && (((uintptr_t)ids) & 3) == 0 && (((uintptr_t)status) & 3) == 0,
               TG_ERR_ALIGN, "tg_text_embed: tok_emb, pos_emb and out must be 16-byte aligned with ldo a multiple of 8, ids and status 4-byte aligned");
    const long n8 = rows * (long)(D / 8);
    TG_REQUIRE(n8 < (1L << 39), TG_ERR_SHAPE, "tg_text_embed: too many elements");
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, ids, n8, S, (const bf16_t*)tok_emb, V, (const bf16_t*)pos_emb,
                       (bf16_t*)out, ldo, D / 8, status);
    TG_LAUNCH_CHECK("tg_text_embed");
    return TG_OK;
}

extern "C" int tg_text_alignment(const float* img, long ld_img, int F, const float* txt, long ld_txt, int K, int D, double* cos_out, hipStream_t stream) {
    TG_REQUIRE(img && txt && cos_out, TG_ERR_ARG, "tg_text_alignment: null pointer");
    TG_REQUIRE(F >= 1 && K >= 1 && D >= 1 && ld_img >= D && ld_txt >= D, TG_ERR_SHAPE,
               "tg_text_alignment: need F >= 1, K >= 1, D >= 1 and leading dimensions >= D (F=%d K=%d D=%d ld_img=%ld ld_txt=%ld)", F, K, D, ld_img, ld_txt);
    TG_REQUIRE((((uintptr_t)img) & 3) == 0 && (((uintptr_t)txt) & 3) == 0 && (((uintptr_t)cos_out) & 7) == 0, TG_ERR_ALIGN,
               "tg_text_alignment: features must be 4-byte aligned, the output 8-byte aligned");
    hipLaunchKernelGGL(text_alignment_kernel, dim3((unsigned)F), dim3(64), 0, stream, img, ld_img, txt, ld_txt, K, D, cos_out);
    TG_LAUNCH_CHECK("tg_text_alignment");
    return TG_OK;
}
