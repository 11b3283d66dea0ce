// The T5 encoder's own kernels (transformers T5EncoderModel, the CogVideoX-5b text_encoder configuration; host side: tokensgen_amd/t5.py).  Every projection of
// the encoder is tg_gemm_bf16; what is here is the rest of a T5 block:
//   tg_rmsnorm       T5LayerNorm: y = w * bf16(x * rsqrt(mean(x^2) + eps)), no mean subtraction and no bias.  One wave per row, the sum of squares in fp32 in a
//                    fixed order (a lane's elements in column order, then the lanes by butterfly), the row read a second time for the output.
//   tg_t5_attention  T5Attention.forward of one encoder block without a mask: softmax_fp32(q k^T + bias[h][j - i]) v per head, NO 1/sqrt(d) scale.  A workgroup of
//                    four waves owns 64 query rows of one (batch, head); a wave owns 16 of them.  The head's K [keys][64] and V, transposed to [64][keys], stay in LDS for
//                    the whole workgroup together with the head's row of the bias-by-distance table (S = 512: 72 + 65 + 4 KiB of the 160), so nothing is rescaled on
//                    line: a wave walks the resident keys three times — row maximum, row sum of exp(s - max), then P V — and recomputes the 16 x 16 score tiles
//                    (two MFMAs each) instead of keeping them.  Scores are computed TRANSPOSED, S^T = K Q^T (v_mfma_f32_16x16x32_bf16, A = 16 keys x 32 dims from LDS,
//                    B = the wave's Q fragment from registers): the result has the query on the lane (lane & 15) and four consecutive keys in the four registers,
//                    which is the A operand of the second product O = P V up to the order of the 32 keys of a k-step; V^T is read in that same order (two 8-byte
//                    reads per fragment), so P goes from accumulator to operand with no lane movement.  The bias is added in fp32 to the fp32 score; P is divided by
//                    the row sum in fp32 and rounded to bf16 (the library's `.type_as(scores)`).  Keys >= S of the last tile are EXCLUDED (they take no part in the
//                    maximum or the sum and enter P V as an exact 0 against zero-filled V), not scored as zeros.
//   tg_gated_gelu    T5DenseGatedActDense between its two GEMMs: out = bf16(gelu_tanh(h[:, :F]) * h[:, F:]) on the output of ONE GEMM over wi_0 | wi_1.
//   tg_residual_add  out = bf16(x + y), the residual of T5LayerSelfAttention / T5LayerFF (dropout is the identity at inference).
#include "common.h"
#include "tokensgen_hip.h"

namespace {

__device__ __forceinline__ void t5_unpack8(const uint4& p, float* f) {
    f[0] = bf16lo_to_f32(p.x); f[1] = bf16hi_to_f32(p.x);
    f[2] = bf16lo_to_f32(p.y); f[3] = bf16hi_to_f32(p.y);
    f[4] = bf16lo_to_f32(p.z); f[5] = bf16hi_to_f32(p.z);
    f[6] = bf16lo_to_f32(p.w); f[7] = bf16hi_to_f32(p.w);
}

// ---- tg_rmsnorm: one wave per row, four rows per workgroup, 16-byte accesses
__global__ __launch_bounds__(256) void rmsnorm_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ w, bf16_t* __restrict__ y, long ldy, long rows,
                                                      int D, float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                  // whole waves leave: no barrier below
    const int lane = threadIdx.x & 63;
    const bf16_t* xr = x + row * ldx;
    bf16_t* yr = y + row * ldy;
    float ss = 0.f;
    for (int c = lane * 8; c < D; c += 512) {                                 // D % 64 == 0: c + 8 <= D
        float v[8];
        t5_unpack8(*(const uint4*)(xr + c), v);
#pragma unroll
        for (int k = 0; k < 8; ++k) ss = fmaf(v[k], v[k], ss);
    }
    ss = wave_sum(ss);
    const float r = 1.f / sqrtf(ss / (float)D + eps);
    for (int c = lane * 8; c < D; c += 512) {
        float v[8], g[8], o[8];
        t5_unpack8(*(const uint4*)(xr + c), v);
        t5_unpack8(*(const uint4*)(w + c), g);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = g[k] * round_bf16(v[k] * r);
        *(uint4*)(yr + c) = uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
    }
}

// ---- tg_gated_gelu / tg_residual_add: 8 elements per thread
__global__ __launch_bounds__(256) void gated_gelu_kernel(const bf16_t* __restrict__ h, long ldh, bf16_t* __restrict__ out, long ldo, long rows, int F8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * F8) return;
    const long r = i / F8;
    const int c = (int)(i - r * F8) * 8;
    float a[8], b[8], o[8];
    t5_unpack8(*(const uint4*)(h + r * ldh + c), a);
    t5_unpack8(*(const uint4*)(h + r * ldh + (long)F8 * 8 + c), b);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = gelu_tanh(a[k]) * b[k];                // (common.h: the function of tg_act mode 2 and of the GEMM's GELU epilogue)
    *(uint4*)(out + r * ldo + c) = uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
}

__global__ __launch_bounds__(256) void residual_add_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y, bf16_t* __restrict__ out, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float a[8], b[8], o[8];
    t5_unpack8(*(const uint4*)(x + i * 8), a);
    t5_unpack8(*(const uint4*)(y + i * 8), b);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = a[k] + b[k];
    *(uint4*)(out + i * 8) = uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
}

// ---- tg_t5_attention
constexpr int T5_MAX_S = 512;
constexpr int T5_KP = 72;                         // K row pitch in LDS (bf16): 144 B, a multiple of 16 for the 16-byte fragment reads, not of 128 (banks)
constexpr int T5_QTILE = 64;                      // query rows per workgroup: 16 per wave

__host__ __device__ constexpr int t5_keys_padded(int S) { return (S + 31) & ~31; }                  // a k-step of the second product is 32 keys
__host__ __device__ constexpr int t5_vpitch(int S) { return t5_keys_padded(S) + 8; }               // V^T row pitch (bf16): a multiple of 4 for the 8-byte reads
__host__ __device__ constexpr long t5_lds_bytes(int S) {
    return (long)t5_keys_padded(S) * T5_KP * 2 + 64L * t5_vpitch(S) * 2 + (((2L * S - 1) * 4 + 15) & ~15L);
}
static_assert(t5_lds_bytes(T5_MAX_S) <= 160 * 1024, "K, V^T and the bias row of one head must fit in the CU's LDS");

// the score tile of 16 keys (kb16) x the wave's 16 queries, transposed: acc[r] = sum_d K[kb16 * 16 + 4 g + r][d] * Q[query of lane & 15][d]
__device__ __forceinline__ f32x4 t5_score_tile(const bf16_t* __restrict__ Ks, int kb16, int l15, int g, const bf16x8 (&qf)[2]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(Ks + (kb16 * 16 + l15) * T5_KP + ks * 32 + g * 8);      // row < keys_padded, column <= 32 + 24 + 7
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
    }
    return acc;
}

__global__ __launch_bounds__(256) void t5_attention_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ld, long sb,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ out, int S, int H) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t5_smem[];
    const int Sp = t5_keys_padded(S), VP = t5_vpitch(S);
    bf16_t* Ks = (bf16_t*)t5_smem;                                            // [Sp][T5_KP]
    bf16_t* Vt = Ks + (long)Sp * T5_KP;                                       // [64][VP]; byte offset Sp * 144: a multiple of 16
    float* bs = (float*)(Vt + 64L * VP);                                      // [2 S - 1]; byte offset + 128 VP: a multiple of 16
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const long base = (long)b * sb + (long)h * 64;

    for (int idx = tid; idx < Sp * 8; idx += 256) {                           // 16 bytes = 8 head dims of one key
        const int row = idx >> 3, c8 = idx & 7;
        uint4 kv = uint4{0u, 0u, 0u, 0u}, vv = uint4{0u, 0u, 0u, 0u};         // keys S .. Sp - 1: zeros (finite operands; they are excluded below)
        if (row < S) {
            kv = *(const uint4*)(k + base + (long)row * ld + c8 * 8);
            vv = *(const uint4*)(v + base + (long)row * ld + c8 * 8);
        }
        *(uint4*)(Ks + row * T5_KP + c8 * 8) = kv;
        const uint32_t vw[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            Vt[(c8 * 8 + 2 * j) * VP + row] = (bf16_t)(vw[j] & 0xffffu);      // dim < 64, row < Sp < VP
            Vt[(c8 * 8 + 2 * j + 1) * VP + row] = (bf16_t)(vw[j] >> 16);
        }
    }
    for (int i = tid; i < 2 * S - 1; i += 256) bs[i] = bias[(long)h * (2 * S - 1) + i];
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * T5_QTILE + wave * 16;
    if (q0 >= S) return;                                                      // no barrier below
    const int qi = q0 + l15;
    bf16x8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (qi < S) qf[ks] = *(const bf16x8*)(q + base + (long)qi * ld + ks * 32 + g * 8);
    }
    // bias_by_distance index of (query qi, key j) is j - qi + S - 1; a lane of a query row past S (never stored) reads as the last row, inside the table
    const float* brow = bs + (S - 1 - min(qi, S - 1));
    const int nkb16 = Sp >> 4;

    float m = -INFINITY;
    for (int kb = 0; kb < nkb16; ++kb) {
        const f32x4 acc = t5_score_tile(Ks, kb, l15, g, qf);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = kb * 16 + 4 * g + r;
            if (key < S) m = fmaxf(m, acc[r] + brow[key]);
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));                                      // finite: key 0 exists in every group's view after the exchange

    float sum = 0.f;
    for (int kb = 0; kb < nkb16; ++kb) {
        const f32x4 acc = t5_score_tile(Ks, kb, l15, g, qf);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = kb * 16 + 4 * g + r;
            if (key < S) sum += expf(acc[r] + brow[key] - m);
        }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);                                           // >= 1: the row maximum contributes exp(0)

    f32x4 o[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb32 = 0; kb32 < (Sp >> 5); ++kb32) {
        float p[8];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 acc = t5_score_tile(Ks, kb32 * 2 + t, l15, g, qf);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kb32 * 32 + t * 16 + 4 * g + r;
                p[t * 4 + r] = key < S ? expf(acc[r] + brow[key] - m) / sum : 0.f;
            }
        }
        // element j of the fragment of lane group g is key kb32 * 32 + (j < 4 ? 4 g + j : 16 + 4 g + j - 4): the same order on both operands
        union { uint32_t u[4]; bf16x8 v; } pf;
#pragma unroll
        for (int j = 0; j < 4; ++j) pf.u[j] = pack_bf16x2(p[2 * j], p[2 * j + 1]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const bf16_t* vr = Vt + (nb * 16 + l15) * VP + kb32 * 32 + 4 * g;  // + 16 + 3 <= Sp - 1
            union { uint2 u[2]; bf16x8 v; } vf;
            vf.u[0] = *(const uint2*)vr;
            vf.u[1] = *(const uint2*)(vr + 16);
            o[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf.v, vf.v, o[nb], 0, 0, 0);
        }
    }

    // o[nb][r]: query q0 + 4 g + r, head dim nb * 16 + (lane & 15)
    const long HD = (long)H * 64;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qo = q0 + 4 * g + r;
        if (qo < S) {
            bf16_t* orow = out + ((long)b * S + qo) * HD + (long)h * 64 + l15;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) orow[nb * 16] = f32_to_bf16(o[nb][r]);
        }
    }
}

}  // namespace

extern "C" int tg_rmsnorm(const void* x, long ldx, const void* w, void* y, long ldy, long rows, int D, float eps, hipStream_t stream) {
    TG_REQUIRE(x && w && y, TG_ERR_ARG, "tg_rmsnorm: null pointer");
    TG_REQUIRE(rows > 0 && D > 0 && D % 64 == 0 && ldx >= D && ldy >= D && rows <= (1L << 31), TG_ERR_SHAPE,
               "tg_rmsnorm: need rows >= 1, D %% 64 == 0 and leading dimensions >= D (rows=%ld D=%d ldx=%ld ldy=%ld)", rows, D, ldx, ldy);
    TG_REQUIRE(eps >= 0.f, TG_ERR_ARG, "tg_rmsnorm: eps must not be negative");
    TG_REQUIRE(tg_aligned16(x) && tg_aligned16(w) && tg_aligned16(y) && ldx % 8 == 0 && ldy % 8 == 0, TG_ERR_ALIGN,
               "tg_rmsnorm: x, w and y must be 16-byte aligned, the leading dimensions multiples of 8");
    hipLaunchKernelGGL(rmsnorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)x, ldx, (const bf16_t*)w, (bf16_t*)y, ldy, rows, D, eps);
    TG_LAUNCH_CHECK("tg_rmsnorm");
    return TG_OK;
}

extern "C" int tg_gated_gelu(const void* h, long ldh, void* out, long ldo, long rows, int F, hipStream_t stream) {
    TG_REQUIRE(h && out, TG_ERR_ARG, "tg_gated_gelu: null pointer");
    TG_REQUIRE(rows > 0 && F > 0 && F % 8 == 0 && ldh >= 2L * F && ldo >= F && rows * (long)(F / 8) < (1L << 39), TG_ERR_SHAPE,
               "tg_gated_gelu: need rows >= 1, F %% 8 == 0, ldh >= 2 F and ldo >= F (rows=%ld F=%d ldh=%ld ldo=%ld)", rows, F, ldh, ldo);
    TG_REQUIRE(tg_aligned16(h) && tg_aligned16(out) && ldh % 8 == 0 && ldo % 8 == 0, TG_ERR_ALIGN,
               "tg_gated_gelu: h and out must be 16-byte aligned, the leading dimensions multiples of 8");
    const long n8 = rows * (long)(F / 8);
    hipLaunchKernelGGL(gated_gelu_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)h, ldh, (bf16_t*)out, ldo, rows, F / 8);
    TG_LAUNCH_CHECK("tg_gated_gelu");
    return TG_OK;
}

extern "C" int tg_residual_add(const void* x, const void* y, void* out, long n, hipStream_t stream) {
    TG_REQUIRE(x && y && out, TG_ERR_ARG, "tg_residual_add: null pointer");
    TG_REQUIRE(n > 0 && n % 8 == 0 && n / 8 < (1L << 39), TG_ERR_SHAPE, "tg_residual_add: n must be a positive multiple of 8 (got %ld)", n);
    TG_REQUIRE(tg_aligned16(x) && tg_aligned16(y) && tg_aligned16(out), TG_ERR_ALIGN, "tg_residual_add: x, y and out must be 16-byte aligned");
    hipLaunchKernelGGL(residual_add_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)y, (bf16_t*)out, n / 8);
    TG_LAUNCH_CHECK("tg_residual_add");
    return TG_OK;
}

extern "C" int tg_t5_attention(const void* q, const void* k, const void* v, long ld, long stride_b, const float* bias_by_distance, void* out, int B, int S, int H,
                               hipStream_t stream) {
    TG_REQUIRE(q && k && v && bias_by_distance && out, TG_ERR_ARG, "tg_t5_attention: null pointer");
    TG_REQUIRE(S >= 1 && S <= T5_MAX_S, TG_ERR_SHAPE, "tg_t5_attention: 1 <= S <= %d (one head's K and V stay in LDS), got %d", T5_MAX_S, S);
    TG_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && ld >= 64L * H && stride_b >= 0, TG_ERR_SHAPE,
               "tg_t5_attention: need 1 <= B, H <= 65535, ld >= 64 H and a non-negative batch stride (B=%d H=%d ld=%ld stride_b=%ld)", B, H, ld, stride_b);
    TG_REQUIRE(tg_aligned16(q) && tg_aligned16(k) && tg_aligned16(v) && ld % 8 == 0 && stride_b % 8 == 0 && (((uintptr_t)bias_by_distance) & 3) == 0 &&
                   (((uintptr_t)out) & 1) == 0, TG_ERR_ALIGN,
               "tg_t5_attention: q, k, v must be 16-byte aligned with ld and stride_b multiples of 8, bias_by_distance 4-byte aligned");
    TG_DYN_LDS(t5_attention_kernel, (int)t5_lds_bytes(T5_MAX_S));
    hipLaunchKernelGGL(t5_attention_kernel, dim3((unsigned)((S + T5_QTILE - 1) / T5_QTILE), (unsigned)H, (unsigned)B), dim3(256), (size_t)t5_lds_bytes(S), stream,
                       (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, stride_b, bias_by_distance, (bf16_t*)out, S, H);
    TG_LAUNCH_CHECK("tg_t5_attention");
    return TG_OK;
}
