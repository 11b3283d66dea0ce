// Backward kernels of the training step around the attention operator (reference loop train_cogvideo_to2v.py:1721-2021,
// trainable parameters = names containing "vip_", :1456-1481): per-head LayerNorm + RoPE backward (attention_processor.py:2031-2056),
// and the two HBM-bound helpers that let the existing MFMA GEMM (tg_gemm_bf16: C = A W^T) compute weight and input gradients —
// a 2-D transpose (dW = dY^T X needs both operands K-contiguous along the token axis) and deterministic column sums (bias gradients).
#include "common.h"
#include "tokensgen_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// y = rope(bf16(LN64(x) g + b)) * out_scale      (forward: norm.hip qk_norm_rope_slice)
// Backward for one (token, head) row of 64, 8 lanes x 8 elements like the forward:
//   dl = rope^T(dy * out_scale)        (pair (a, b), angle c/s:  da = dy_a c + dy_b s,  db = dy_b c - dy_a s)
//   dg += dl * x_hat   db += dl        (summed over tokens / heads / batch: per-block partial sums, fixed order)
//   dxh = dl * g       dx = rstd (dxh - mean(dxh) - x_hat mean(dxh * x_hat))
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int ROWS_PER_BLOCK = 32;          // (token, head) rows per pass of a 256-thread block
constexpr int PASSES = 16;                  // passes per block: 512 rows per block

__global__ __launch_bounds__(256) void qk_norm_rope_bwd_kernel(const bf16_t* __restrict__ x, long ld, long sb, const float* __restrict__ dy, long dld,
                                                               long dsb, bf16_t* __restrict__ dx, long xld, long xsb, int tokens, int heads, int batch,
                                                               const bf16_t* __restrict__ w, float eps, int start0, int len0,
                                                               const float* __restrict__ cos0, const float* __restrict__ sin0, int start1, int len1,
                                                               const float* __restrict__ cos1, const float* __restrict__ sin1, float out_scale,
                                                               float* __restrict__ partial) {
    __shared__ float red[ROWS_PER_BLOCK][2][64];
    const int tid = threadIdx.x, part = tid & 7, rl = tid >> 3;
    const long total = (long)batch * tokens * heads;
    float g[8], dgs[8], dbs[8];
    {
        const uint4 wv = *(const uint4*)(w + part * 8);
        const uint32_t wu[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { g[2 * i] = bf16lo_to_f32(wu[i]); g[2 * i + 1] = bf16hi_to_f32(wu[i]); }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) dgs[i] = dbs[i] = 0.f;
    for (int ps = 0; ps < PASSES; ++ps) {
        const long rowid = ((long)blockIdx.x * PASSES + ps) * ROWS_PER_BLOCK + rl;
        const bool live = rowid < total;
        const long rid = live ? rowid : total - 1;
        const int h = (int)(rid % heads);
        const long bt = rid / heads;
        const int t = (int)(bt % tokens), b = (int)(bt / tokens);
        const float* cs = nullptr;
        const float* sn = nullptr;
        if (t >= start0 && t < start0 + len0) { cs = cos0 + (long)(t - start0) * 64 + part * 8; sn = sin0 + (long)(t - start0) * 64 + part * 8; }
        else if (t >= start1 && t < start1 + len1) { cs = cos1 + (long)(t - start1) * 64 + part * 8; sn = sin1 + (long)(t - start1) * 64 + part * 8; }
        const uint4 raw = *(const uint4*)(x + (long)b * sb + (long)t * ld + h * 64 + part * 8);
        const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
        float v[8], s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = bf16lo_to_f32(u[i]); v[2 * i + 1] = bf16hi_to_f32(u[i]); s += v[2 * i] + v[2 * i + 1]; }
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
        const float mean = s * (1.f / 64.f);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { v[i] -= mean; q += v[i] * v[i]; }
        q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
        const float rstd = rsqrtf(q * (1.f / 64.f) + eps);
        const float* dp = dy + (long)b * dsb + (long)t * dld + h * 64 + part * 8;
        const float4 d0 = *(const float4*)dp, d1 = *(const float4*)(dp + 4);
        float dl[8] = {d0.x * out_scale, d0.y * out_scale, d0.z * out_scale, d0.w * out_scale,
                       d1.x * out_scale, d1.y * out_scale, d1.z * out_scale, d1.w * out_scale};
        if (cs) {
            const float4 c0 = *(const float4*)cs, c1 = *(const float4*)(cs + 4), s0 = *(const float4*)sn, s1 = *(const float4*)(sn + 4);
            const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {      // forward: y_a = a c_a - b s_a,  y_b = b c_b + a s_b
                const float ya = dl[2 * i], yb = dl[2 * i + 1];
                dl[2 * i] = ya * c[2 * i] + yb * sv[2 * i + 1];
                dl[2 * i + 1] = yb * c[2 * i + 1] - ya * sv[2 * i];
            }
        }
        float m1 = 0.f, m2 = 0.f, dxh[8], xh[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            xh[i] = v[i] * rstd;
            if (live) { dgs[i] += dl[i] * xh[i]; dbs[i] += dl[i]; }
            dxh[i] = dl[i] * g[i];
            m1 += dxh[i];
            m2 += dxh[i] * xh[i];
        }
        m1 += __shfl_xor(m1, 1, 64); m1 += __shfl_xor(m1, 2, 64); m1 += __shfl_xor(m1, 4, 64);
        m2 += __shfl_xor(m2, 1, 64); m2 += __shfl_xor(m2, 2, 64); m2 += __shfl_xor(m2, 4, 64);
        m1 *= (1.f / 64.f); m2 *= (1.f / 64.f);
        if (live) {
            float o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = rstd * (dxh[i] - m1 - xh[i] * m2);
            uint4 ov;
            ov.x = pack_bf16x2(o[0], o[1]); ov.y = pack_bf16x2(o[2], o[3]); ov.z = pack_bf16x2(o[4], o[5]); ov.w = pack_bf16x2(o[6], o[7]);
            *(uint4*)(dx + (long)b * xsb + (long)t * xld + h * 64 + part * 8) = ov;
        }
    }
    // block partial of dg / db per channel: row lanes summed in a fixed order
#pragma unroll
    for (int i = 0; i < 8; ++i) { red[rl][0][part * 8 + i] = dgs[i]; red[rl][1][part * 8 + i] = dbs[i]; }
    __syncthreads();
    if (tid < 128) {
        const int st = tid >> 6, c = tid & 63;
        float a = 0.f;
        for (int r = 0; r < ROWS_PER_BLOCK; ++r) a += red[r][st][c];
        partial[(long)blockIdx.x * 128 + tid] = a;
    }
}

// dst[c][r] = src[r][c] for r < rows, 0 for rows <= r < rows_pad (the token axis is zero-padded to the GEMM's K granule)
__global__ __launch_bounds__(256) void transpose_2d_kernel(const bf16_t* __restrict__ src, long ld, int rows, int cols, bf16_t* __restrict__ dst,
                                                           long ldd, int rows_pad) {
    __shared__ bf16_t tile[64][66];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        tile[r][c] = (r0 + r < rows && c0 + c < cols) ? src[(long)(r0 + r) * ld + c0 + c] : (bf16_t)0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (c0 + c < cols && r0 + r < rows_pad) dst[(long)(c0 + c) * ldd + r0 + r] = tile[r][c];
    }
}

// 16-byte form of transpose_2d_kernel (cols, row strides and rows_pad multiples of 8, 16-byte aligned bases): 128-byte runs on both the global read and the
// global write side; the tile's row stride of 66 elements keeps the 4-byte LDS stores and the strided 2-byte LDS loads off each other's banks.
__global__ __launch_bounds__(256) void transpose_2d_vec_kernel(const bf16_t* __restrict__ src, long ld, int rows, int cols, bf16_t* __restrict__ dst,
                                                               long ldd, int rows_pad) {
    __shared__ __attribute__((aligned(4))) bf16_t tile[64 * 66];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = threadIdx.x + k * 256, r = i >> 3, cc = (i & 7) * 8;
        uint4 v = uint4{0, 0, 0, 0};
        if (r0 + r < rows && c0 + cc < cols) v = *(const uint4*)(src + (long)(r0 + r) * ld + c0 + cc);
        uint32_t* d = (uint32_t*)(tile + r * 66 + cc);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = threadIdx.x + k * 256, c = i >> 3, rr = (i & 7) * 8;
        if (c0 + c >= cols || r0 + rr >= rows_pad) continue;
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (uint32_t)tile[(rr + 2 * e) * 66 + c] | ((uint32_t)tile[(rr + 2 * e + 1) * 66 + c] << 16);
        *(uint4*)(dst + (long)(c0 + c) * ldd + r0 + rr) = uint4{w[0], w[1], w[2], w[3]};
    }
}

// partial[blk][c] = sum over the block's rows of src[r][c]  (fp32; summed over blk on the host side in a fixed order)
// Rows per block: 256 for the big matrices; fewer for short ones so that the launch still has ~2000 workgroups (a [480 x 3072] product tensor of
// the vip rows was 24 workgroups walking 256 rows each: 75 us per call, 16 calls per layer).  A function of the shape only: the summation order
// stays fixed, and tg_colsum_partial_floats() uses the same value.
static inline int cs_rows(int rows, int cols) {
    const long cb = (cols + 255) / 256;
    long r = ((long)rows * cb + 2047) / 2048;
    r = r < 8 ? 8 : (r > 256 ? 256 : r);
    return (int)r;
}
__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ src, long ld, int rows, int cols, float* __restrict__ partial, int CS_ROWS) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= cols) return;
    const int r0 = blockIdx.x * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    float a = 0.f;
    for (int r = r0; r < r1; ++r) a += bf16_to_f32(src[(long)r * ld + c]);
    partial[(long)blockIdx.x * cols + c] = a;
}

// 8 columns per thread (16-byte loads; cols and ld multiples of 8): same per-column summation order as colsum_kernel, a quarter of the load instructions
__global__ __launch_bounds__(256) void colsum_vec_kernel(const bf16_t* __restrict__ src, long ld, int rows, int cols, float* __restrict__ partial, int CS_ROWS) {
    const int c = (blockIdx.y * 256 + threadIdx.x) * 8;
    if (c >= cols) return;
    const int r0 = blockIdx.x * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; ++r) {
        const uint4 v = *(const uint4*)(src + (long)r * ld + c);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[2 * i] += bf16lo_to_f32(u[i]); a[2 * i + 1] += bf16hi_to_f32(u[i]); }
    }
    float* dst = partial + (long)blockIdx.x * cols + c;
    *(float4*)dst = float4{a[0], a[1], a[2], a[3]};
    *(float4*)(dst + 4) = float4{a[4], a[5], a[6], a[7]};
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward of tg_adaln_modulate:  y = ln * (1 + scale[g]) + shift[g],  ln = bf16(x_hat * gamma + beta),  x_hat = (x - mean) * rstd
// (normalization.py:441-460, 477-488).  One wave per token row.  Per element it also emits the three products whose column sums (over all
// rows, or over the rows of one group) are the parameter gradients:  t_dln = dy (1 + scale)  [-> d beta],  t_dlnx = t_dln * x_hat  [-> d gamma],
// t_dyln = dy * ln  [-> d scale[g]]  (d shift[g] = column sums of dy itself).  fp32 [rows][dim]; summed by tg_colsum_f32 in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adaln_bwd_scalar_kernel(const bf16_t* __restrict__ x, long ldx, long sxb, const bf16_t* __restrict__ dy, long ldd, long sdb,
                                                        bf16_t* __restrict__ dx, long ldo, long sob, const bf16_t* __restrict__ w,
                                                        const bf16_t* __restrict__ bvec, float eps, int tokens, int dim, int batch, int modulate,
                                                        tg_group_table g, float* __restrict__ t_dln, float* __restrict__ t_dlnx,
                                                        float* __restrict__ t_dyln, const bf16_t* __restrict__ add, long lda, long sab) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)tokens * batch) return;
    const int b = (int)(row / tokens), t = (int)(row % tokens);
    const bf16_t* xr = x + (long)b * sxb + (long)t * ldx;
    const bf16_t* dr = dy + (long)b * sdb + (long)t * ldd;
    bf16_t* outr = dx + (long)b * sob + (long)t * ldo;
    float s = 0.f;
    for (int c = lane; c < dim; c += 64) s += bf16_to_f32(xr[c]);
    const float mean = wave_sum(s) / dim;
    float q = 0.f;
    for (int c = lane; c < dim; c += 64) { const float d = bf16_to_f32(xr[c]) - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / dim + eps);
    const bf16_t* scale = nullptr;
    if (modulate) {
        const int gi = g.tok_group[t];
        scale = (const bf16_t*)g.mod + (long)b * g.mod_batch_stride + (long)g.row[gi] * g.mod_ld + g.scale_col[gi];
    }
    float m1 = 0.f, m2 = 0.f;
    for (int c = lane; c < dim; c += 64) {
        const float xh = (bf16_to_f32(xr[c]) - mean) * rstd;
        const float gam = w ? bf16_to_f32(w[c]) : 1.f, bet = bvec ? bf16_to_f32(bvec[c]) : 0.f;
        const float ln = round_bf16(xh * gam + bet);
        const float d = bf16_to_f32(dr[c]);
        const float dln = d * (1.f + (scale ? bf16_to_f32(scale[c]) : 0.f));
        if (t_dln) {                                       // the products are wanted only where the norm's parameters train (the vip rows)
            const long o = row * dim + c;
            t_dln[o] = dln; t_dlnx[o] = dln * xh; t_dyln[o] = d * ln;
        }
        const float dxh = dln * gam;
        m1 += dxh; m2 += dxh * xh;
    }
    m1 = wave_sum(m1) / dim; m2 = wave_sum(m2) / dim;
    const bf16_t* ar = add ? add + (long)b * sab + (long)t * lda : nullptr;
    for (int c = lane; c < dim; c += 64) {
        const float xh = (bf16_to_f32(xr[c]) - mean) * rstd;
        const float dln = bf16_to_f32(dr[c]) * (1.f + (scale ? bf16_to_f32(scale[c]) : 0.f));
        const float dxh = dln * (w ? bf16_to_f32(w[c]) : 1.f);
        float v = rstd * (dxh - m1 - xh * m2);
        if (ar) v = round_bf16(v) + bf16_to_f32(ar[c]);     // + the gradient arriving over the residual connection (both bf16 tensors in the reference)
        outr[c] = f32_to_bf16(v);
    }
}

// The same with 16-byte accesses (8 bf16 per lane per access; needs dim % 8 == 0 and 16-byte aligned rows): the scalar form above moved 2 bytes
// per lane per load and ran at ~1 TB/s.
__device__ __forceinline__ void unpack8(uint4 v, float (&f)[8]) {
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf16lo_to_f32(u[i]); f[2 * i + 1] = bf16hi_to_f32(u[i]); }
}
// NC > 0: the row's chunks (dim <= 512 NC) stay in registers as packed bf16 — x, dy and the modulation scale are read from memory ONCE (the NC = 0 form re-reads the row
// for each of its four passes: L1 / L2 hits, but four dependent load -> reduce chains per row; 3.2 TB/s of compulsory traffic at dim 3072).  Same arithmetic in the
// same order: bitwise the same result.
template <int NC>
__global__ __launch_bounds__(256) void adaln_bwd_kernel(const bf16_t* __restrict__ x, long ldx, long sxb, const bf16_t* __restrict__ dy, long ldd, long sdb,
                                                        bf16_t* __restrict__ dx, long ldo, long sob, const bf16_t* __restrict__ w,
                                                        const bf16_t* __restrict__ bvec, float eps, int tokens, int dim, int batch, int modulate,
                                                        tg_group_table g, float* __restrict__ t_dln, float* __restrict__ t_dlnx,
                                                        float* __restrict__ t_dyln, const bf16_t* __restrict__ add, long lda, long sab) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)tokens * batch) return;
    const int b = (int)(row / tokens), t = (int)(row % tokens);
    const bf16_t* xr = x + (long)b * sxb + (long)t * ldx;
    const bf16_t* dr = dy + (long)b * sdb + (long)t * ldd;
    bf16_t* outr = dx + (long)b * sob + (long)t * ldo;
    const int nch = dim >> 3;
    constexpr int NR = NC > 0 ? NC : 1;
    uint4 xq[NR], dq[NR], sq[NR];                      // (the residual rows are read in the last pass: holding them too costs a wave of occupancy and measured slower)
    const bf16_t* scale = nullptr;
    if (modulate) {
        const int gi = g.tok_group[t];
        scale = (const bf16_t*)g.mod + (long)b * g.mod_batch_stride + (long)g.row[gi] * g.mod_ld + g.scale_col[gi];
    }
    const bf16_t* ar = add ? add + (long)b * sab + (long)t * lda : nullptr;
    if (NC > 0) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int c = lane + 64 * k;
            const bool in = c < nch;
            xq[k] = in ? *(const uint4*)(xr + c * 8) : uint4{0, 0, 0, 0};
            dq[k] = in ? *(const uint4*)(dr + c * 8) : uint4{0, 0, 0, 0};
            sq[k] = in && scale ? *(const uint4*)(scale + c * 8) : uint4{0, 0, 0, 0};
        }
    }
    auto ld_x = [&](int k, int c, float (&f)[8]) { unpack8(NC > 0 ? xq[k] : *(const uint4*)(xr + c * 8), f); };
    auto ld_d = [&](int k, int c, float (&f)[8]) { unpack8(NC > 0 ? dq[k] : *(const uint4*)(dr + c * 8), f); };
    auto ld_s = [&](int k, int c, float (&f)[8]) { unpack8(NC > 0 ? sq[k] : *(const uint4*)(scale + c * 8), f); };
    float s = 0.f, f[8], e[8];
#pragma unroll NR
    for (int k = 0; k < (NC > 0 ? NC : 1 << 20); ++k) {
        const int c = lane + 64 * k;
        if (c >= nch) break;
        ld_x(k, c, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) s += f[i];
    }
    const float mean = wave_sum(s) / dim;
    float q = 0.f;
#pragma unroll NR
    for (int k = 0; k < (NC > 0 ? NC : 1 << 20); ++k) {
        const int c = lane + 64 * k;
        if (c >= nch) break;
        ld_x(k, c, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = f[i] - mean; q += d * d; }
    }
    const float rstd = rsqrtf(wave_sum(q) / dim + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll NR
    for (int k = 0; k < (NC > 0 ? NC : 1 << 20); ++k) {
        const int c = lane + 64 * k;
        if (c >= nch) break;
        float gam[8], bet[8], sc[8];
        ld_x(k, c, f);
        ld_d(k, c, e);
        if (w) unpack8(*(const uint4*)(w + c * 8), gam);
        if (bvec) unpack8(*(const uint4*)(bvec + c * 8), bet);
        if (scale) ld_s(k, c, sc);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float xh = (f[i] - mean) * rstd;
            const float ga = w ? gam[i] : 1.f;
            const float dln = e[i] * (1.f + (scale ? sc[i] : 0.f));
            if (t_dln) {
                const long o = row * dim + c * 8 + i;
                t_dln[o] = dln; t_dlnx[o] = dln * xh; t_dyln[o] = e[i] * round_bf16(xh * ga + (bvec ? bet[i] : 0.f));
            }
            const float dxh = dln * ga;
            m1 += dxh; m2 += dxh * xh;
        }
    }
    m1 = wave_sum(m1) / dim; m2 = wave_sum(m2) / dim;
#pragma unroll NR
    for (int k = 0; k < (NC > 0 ? NC : 1 << 20); ++k) {
        const int c = lane + 64 * k;
        if (c >= nch) break;
        float gam[8], sc[8], a8[8], v[8];
        ld_x(k, c, f);
        ld_d(k, c, e);
        if (w) unpack8(*(const uint4*)(w + c * 8), gam);
        if (scale) ld_s(k, c, sc);
        if (ar) unpack8(*(const uint4*)(ar + c * 8), a8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float xh = (f[i] - mean) * rstd;
            const float dxh = e[i] * (1.f + (scale ? sc[i] : 0.f)) * (w ? gam[i] : 1.f);
            v[i] = rstd * (dxh - m1 - xh * m2);
            if (ar) v[i] = round_bf16(v[i]) + a8[i];
        }
        *(uint4*)(outr + c * 8) = uint4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
    }
}

// Backward of the gated residual  out = res + gate[g] * y  (cogvideox_transformer_3d.py:290-293, 318-324):  dy = gate[g] * dout (bf16),
// t_dgate = dout * y (fp32; its column sums over the rows of group g are d gate[g]);  d res = dout.
__global__ __launch_bounds__(256) void gate_res_bwd_scalar_kernel(const bf16_t* __restrict__ dout, long ldd, long sdb, const bf16_t* __restrict__ y, long ldy,
                                                           long syb, bf16_t* __restrict__ dyo, long ldo, long sob, int tokens, int dim, int batch,
                                                           tg_group_table g, float* __restrict__ t_dgate, int t_row0) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)batch * tokens * dim;
    if (i >= total) return;
    const int c = (int)(i % dim);
    const long row = i / dim;
    const int b = (int)(row / tokens), t = (int)(row % tokens);
    const int gi = g.tok_group[t];
    const float gate = bf16_to_f32(((const bf16_t*)g.mod)[(long)b * g.mod_batch_stride + (long)g.row[gi] * g.mod_ld + g.gate_col[gi] + c]);
    const float d = bf16_to_f32(dout[(long)b * sdb + (long)t * ldd + c]);
    dyo[(long)b * sob + (long)t * ldo + c] = f32_to_bf16(gate * d);
    if (t >= t_row0) t_dgate[((long)b * (tokens - t_row0) + (t - t_row0)) * dim + c] = d * bf16_to_f32(y[(long)b * syb + (long)t * ldy + c]);
}

__global__ __launch_bounds__(256) void gate_res_bwd_kernel(const bf16_t* __restrict__ dout, long ldd, long sdb, const bf16_t* __restrict__ y, long ldy,
                                                           long syb, bf16_t* __restrict__ dyo, long ldo, long sob, int tokens, int dim, int batch,
                                                           tg_group_table g, float* __restrict__ t_dgate, int t_row0) {       // 8 elements per thread
    const int nch = dim >> 3;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)batch * tokens * nch) return;
    const int c = (int)(i % nch) * 8;
    const long row = i / nch;
    const int b = (int)(row / tokens), t = (int)(row % tokens);
    const int gi = g.tok_group[t];
    float ga[8], d[8], yv[8], o[8];
    unpack8(*(const uint4*)((const bf16_t*)g.mod + (long)b * g.mod_batch_stride + (long)g.row[gi] * g.mod_ld + g.gate_col[gi] + c), ga);
    unpack8(*(const uint4*)(dout + (long)b * sdb + (long)t * ldd + c), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = ga[k] * d[k];
    *(uint4*)(dyo + (long)b * sob + (long)t * ldo + c) = uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
    if (t >= t_row0) {
        unpack8(*(const uint4*)(y + (long)b * syb + (long)t * ldy + c), yv);
        float* dst = t_dgate + ((long)b * (tokens - t_row0) + (t - t_row0)) * dim + c;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = d[k] * yv[k];
    }
}

// mode 0: y = silu(x);  mode 1: dx = dy * gelu_tanh'(x)  (F.gelu(approximate="tanh"), diffusers FeedForward);  mode 2: y = gelu_tanh(x), the
// same function as the GEMM's GELU epilogue (the training forward keeps the pre-activation for mode 1 and applies the activation in this pass
// instead of running the FF1 GEMM a second time)
__device__ __forceinline__ float act_one(float v, float dyv, int mode) {
    if (mode == 0) return v / (1.f + __expf(-v));
    if (mode == 2) return gelu_tanh(v);
    return gelu_tanh_bwd(v, dyv);               // (common.h)
}
__global__ __launch_bounds__(256) void act_scalar_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, bf16_t* __restrict__ out, long n, int mode) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = f32_to_bf16(act_one(bf16_to_f32(x[i]), mode == 1 ? bf16_to_f32(dy[i]) : 0.f, mode));      // (the same function as the 16-byte form: same values)
}

__global__ __launch_bounds__(256) void act_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, bf16_t* __restrict__ out, long n8, int mode) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;                  // 8 elements per thread
    if (i >= n8) return;
    float v[8], d[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
    unpack8(*(const uint4*)(x + i * 8), v);
    if (mode == 1) unpack8(*(const uint4*)(dy + i * 8), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = act_one(v[k], d[k], mode);
    *(uint4*)(out + i * 8) = uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
}

// Column sums of SEVERAL matrices in one launch (a vip_norm's gradients need eight: 16 launches with their `partial.sum(0)`s, now 2).  Every item is cut into the
// same number of row blocks NB, so the partials form ONE [NB][total columns] matrix that a single fixed-order sum finishes; the table travels by value.
struct ColsumTable {
    const void* src[TG_COLSUM_MAX];
    long ld[TG_COLSUM_MAX];
    int rows[TG_COLSUM_MAX], cols[TG_COLSUM_MAX], col0[TG_COLSUM_MAX];      // col0: first column of the item in the joint partial matrix
    unsigned first_block[TG_COLSUM_MAX + 1];                                  // blockIdx.y ranges (256 columns per block)
    unsigned f32_mask;
    int count, total_cols;
};
__global__ __launch_bounds__(256) void colsum_multi_kernel(ColsumTable t, float* __restrict__ partial) {
    int it = 0;
    while (it + 1 < t.count && blockIdx.y >= t.first_block[it + 1]) ++it;
    const int c = (blockIdx.y - t.first_block[it]) * 256 + threadIdx.x;
    if (c >= t.cols[it]) return;
    const int rows = t.rows[it], per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
    const long ld = t.ld[it];
    float a = 0.f;
    if ((t.f32_mask >> it) & 1u) for (int r = r0; r < r1; ++r) a += ((const float*)t.src[it])[(long)r * ld + c];
    else for (int r = r0; r < r1; ++r) a += bf16_to_f32(((const bf16_t*)t.src[it])[(long)r * ld + c]);
    partial[(long)blockIdx.x * t.total_cols + t.col0[it] + c] = a;
}

__global__ __launch_bounds__(256) void colsum_f32_kernel(const float* __restrict__ src, long ld, int rows, int cols, float* __restrict__ partial, int CS_ROWS) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= cols) return;
    const int r0 = blockIdx.x * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    float a = 0.f;
    for (int r = r0; r < r1; ++r) a += src[(long)r * ld + c];
    partial[(long)blockIdx.x * cols + c] = a;
}

}  // namespace

extern "C" long tg_qk_layernorm_rope_bwd_partial_floats(int tokens, int heads, int batch) {
    const long rows = (long)batch * tokens * heads, per = (long)ROWS_PER_BLOCK * PASSES;
    return ((rows + per - 1) / per) * 128;
}

extern "C" int tg_qk_layernorm_rope_bwd(const void* x, long ld, long strideB, const float* dy, long dy_ld, long dy_strideB, void* dx, long dx_ld,
                                        long dx_strideB, int tokens, int heads, int batch, const void* ln_weight, float eps, int start0, int len0,
                                        const float* cos0, const float* sin0, int start1, int len1, const float* cos1, const float* sin1,
                                        float out_scale, float* partial, hipStream_t stream) {
    TG_REQUIRE(x && dy && dx && ln_weight && partial, TG_ERR_ARG, "tg_qk_layernorm_rope_bwd: null pointer");
    TG_REQUIRE(tokens > 0 && heads > 0 && batch > 0, TG_ERR_SHAPE, "tg_qk_layernorm_rope_bwd: bad shape");
    TG_REQUIRE(ld % 8 == 0 && strideB % 8 == 0 && dx_ld % 8 == 0 && dx_strideB % 8 == 0 && dy_ld % 4 == 0 && dy_strideB % 4 == 0 && tg_aligned16(x) &&
               tg_aligned16(dx) && tg_aligned16(dy) && tg_aligned16(ln_weight), TG_ERR_ALIGN, "tg_qk_layernorm_rope_bwd: rows must be 16-byte aligned");
    TG_REQUIRE((len0 == 0 || (cos0 && sin0 && tg_aligned16(cos0) && tg_aligned16(sin0))) && (len1 == 0 || (cos1 && sin1 && tg_aligned16(cos1) && tg_aligned16(sin1))),
               TG_ERR_ARG, "tg_qk_layernorm_rope_bwd: rope tables missing or unaligned");
    const long rows = (long)batch * tokens * heads, per = (long)ROWS_PER_BLOCK * PASSES;
    hipLaunchKernelGGL(qk_norm_rope_bwd_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, stream, (const bf16_t*)x, ld, strideB, dy, dy_ld,
                       dy_strideB, (bf16_t*)dx, dx_ld, dx_strideB, tokens, heads, batch, (const bf16_t*)ln_weight, eps, start0, len0, cos0, sin0, start1, len1,
                       cos1, sin1, out_scale, partial);
    TG_LAUNCH_CHECK("tg_qk_layernorm_rope_bwd");
    return TG_OK;
}

extern "C" int tg_transpose_2d(const void* src, long ld, int rows, int cols, void* dst, long ld_dst, int rows_pad, hipStream_t stream) {
    TG_REQUIRE(src && dst, TG_ERR_ARG, "tg_transpose_2d: null pointer");
    TG_REQUIRE(rows > 0 && cols > 0 && rows_pad >= rows && ld >= cols && ld_dst >= rows_pad, TG_ERR_SHAPE, "tg_transpose_2d: bad shape");
    const bool vec = cols % 8 == 0 && rows_pad % 8 == 0 && ld % 8 == 0 && ld_dst % 8 == 0 && tg_aligned16(src) && tg_aligned16(dst);
    if (vec)
        hipLaunchKernelGGL(transpose_2d_vec_kernel, dim3((unsigned)((rows_pad + 63) / 64), (unsigned)((cols + 63) / 64)), dim3(256), 0, stream, (const bf16_t*)src,
                           ld, rows, cols, (bf16_t*)dst, ld_dst, rows_pad);
    else
        hipLaunchKernelGGL(transpose_2d_kernel, dim3((unsigned)((rows_pad + 63) / 64), (unsigned)((cols + 63) / 64)), dim3(256), 0, stream, (const bf16_t*)src, ld,
                           rows, cols, (bf16_t*)dst, ld_dst, rows_pad);
    TG_LAUNCH_CHECK("tg_transpose_2d");
    return TG_OK;
}

extern "C" long tg_colsum_partial_floats(int rows, int cols) {
    const int CS_ROWS = cs_rows(rows, cols);
    return (long)((rows + CS_ROWS - 1) / CS_ROWS) * cols;
}

extern "C" int tg_colsum_multi(const tg_colsum_item* items, int count, int row_blocks, float* partial, hipStream_t stream) {
    TG_REQUIRE(items && partial && count > 0 && count <= TG_COLSUM_MAX && row_blocks > 0 && row_blocks <= 1024, TG_ERR_ARG, "tg_colsum_multi: 1..%d items, 1..1024 row blocks", TG_COLSUM_MAX);
    ColsumTable t{};
    t.count = count;
    unsigned nb = 0;
    int col0 = 0;
    for (int i = 0; i < count; ++i) {
        const tg_colsum_item& it = items[i];
        TG_REQUIRE(it.src && it.rows > 0 && it.cols > 0 && it.ld >= it.cols, TG_ERR_SHAPE, "tg_colsum_multi: item %d: bad shape", i);
        t.src[i] = it.src; t.ld[i] = it.ld; t.rows[i] = it.rows; t.cols[i] = it.cols; t.col0[i] = col0;
        if (it.src_is_f32) t.f32_mask |= 1u << i;
        t.first_block[i] = nb;
        nb += (unsigned)((it.cols + 255) / 256);
        col0 += it.cols;
    }
    t.first_block[count] = nb;
    t.total_cols = col0;
    hipLaunchKernelGGL(colsum_multi_kernel, dim3((unsigned)row_blocks, nb), dim3(256), 0, stream, t, partial);
    TG_LAUNCH_CHECK("tg_colsum_multi");
    return TG_OK;
}

extern "C" int tg_colsum(const void* src, long ld, int rows, int cols, float* partial, hipStream_t stream) {
    TG_REQUIRE(src && partial, TG_ERR_ARG, "tg_colsum: null pointer");
    TG_REQUIRE(rows > 0 && cols > 0 && ld >= cols, TG_ERR_SHAPE, "tg_colsum: bad shape");
    const int CS_ROWS = cs_rows(rows, cols);
    if (cols % 8 == 0 && ld % 8 == 0 && tg_aligned16(src) && tg_aligned16(partial))
        hipLaunchKernelGGL(colsum_vec_kernel, dim3((unsigned)((rows + CS_ROWS - 1) / CS_ROWS), (unsigned)((cols / 8 + 255) / 256)), dim3(256), 0, stream,
                           (const bf16_t*)src, ld, rows, cols, partial, CS_ROWS);
    else
        hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((rows + CS_ROWS - 1) / CS_ROWS), (unsigned)((cols + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)src, ld,
                           rows, cols, partial, CS_ROWS);
    TG_LAUNCH_CHECK("tg_colsum");
    return TG_OK;
}

extern "C" int tg_adaln_modulate_bwd(const void* x, long ldx, long strideX, const void* dy, long ld_dy, long stride_dy, void* dx, long ld_dx, long stride_dx,
                                     const void* ln_weight, const void* ln_bias, float eps, int tokens, int dim, int batch, int modulate,
                                     const tg_group_table* g, float* t_dln, float* t_dlnx, float* t_dyln, const void* add, long ld_add, long stride_add,
                                     hipStream_t stream) {
    TG_REQUIRE(x && dy && dx, TG_ERR_ARG, "tg_adaln_modulate_bwd: null pointer");
    TG_REQUIRE((t_dln && t_dlnx && t_dyln) || (!t_dln && !t_dlnx && !t_dyln), TG_ERR_ARG, "tg_adaln_modulate_bwd: give all three product tensors or none");
    TG_REQUIRE(tokens > 0 && dim > 0 && batch > 0 && (!modulate || g), TG_ERR_SHAPE, "tg_adaln_modulate_bwd: bad shape");
    tg_group_table gt{};
    if (g) gt = *g;
    const long rows = (long)tokens * batch;
    // 16-byte form: every row pointer the kernel forms (x, dy, dx, add, the LayerNorm vectors, the scale row of the group table) must be 16-byte aligned
    auto al = [](const void* p_, long ld, long sb) { return !p_ || (tg_aligned16(p_) && ld % 8 == 0 && sb % 8 == 0); };
    bool vec = dim % 8 == 0 && al(x, ldx, strideX) && al(dy, ld_dy, stride_dy) && al(dx, ld_dx, stride_dx) && al(add, ld_add, stride_add) &&
               al(ln_weight, 0, 0) && al(ln_bias, 0, 0);
    if (vec && modulate) {
        vec = tg_aligned16(gt.mod) && gt.mod_ld % 8 == 0 && gt.mod_batch_stride % 8 == 0;
        for (int i = 0; i < TG_MAX_GROUPS; ++i) vec = vec && gt.scale_col[i] % 8 == 0;
    }
    if (vec)
    {
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)x, ldx, strideX, (const bf16_t*)dy, ld_dy, stride_dy,
                               (bf16_t*)dx, ld_dx, stride_dx, (const bf16_t*)ln_weight, (const bf16_t*)ln_bias, eps, tokens, dim, batch, modulate, gt, t_dln, t_dlnx,
                               t_dyln, (const bf16_t*)add, ld_add, stride_add);
        };
        if (dim <= 512 * 6) go(adaln_bwd_kernel<6>);          // (the 5B model: 3072)
        else if (dim <= 512 * 8) go(adaln_bwd_kernel<8>);
        else go(adaln_bwd_kernel<0>);
    }
    else
        hipLaunchKernelGGL(adaln_bwd_scalar_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)x, ldx, strideX, (const bf16_t*)dy, ld_dy,
                           stride_dy, (bf16_t*)dx, ld_dx, stride_dx, (const bf16_t*)ln_weight, (const bf16_t*)ln_bias, eps, tokens, dim, batch, modulate, gt, t_dln,
                           t_dlnx, t_dyln, (const bf16_t*)add, ld_add, stride_add);
    TG_LAUNCH_CHECK("tg_adaln_modulate_bwd");
    return TG_OK;
}

extern "C" int tg_gate_residual_bwd(const void* dout, long ld_dout, long stride_dout, const void* y, long ldy, long strideY, void* dy, long ld_dy, long stride_dy,
                                    int tokens, int dim, int batch, const tg_group_table* gate, float* t_dgate, int t_row0, hipStream_t stream) {
    TG_REQUIRE(dout && y && dy && gate && t_dgate, TG_ERR_ARG, "tg_gate_residual_bwd: null pointer");
    TG_REQUIRE(tokens > 0 && dim > 0 && batch > 0 && t_row0 >= 0 && t_row0 < tokens, TG_ERR_SHAPE, "tg_gate_residual_bwd: bad shape");
    const long total = (long)batch * tokens * dim;
    bool vec = dim % 8 == 0 && tg_aligned16(dout) && tg_aligned16(y) && tg_aligned16(dy) && tg_aligned16(gate->mod) && tg_aligned16(t_dgate) && ld_dout % 8 == 0 &&
               stride_dout % 8 == 0 && ldy % 8 == 0 && strideY % 8 == 0 && ld_dy % 8 == 0 && stride_dy % 8 == 0 && gate->mod_ld % 8 == 0 &&
               gate->mod_batch_stride % 8 == 0;
    for (int i = 0; i < TG_MAX_GROUPS; ++i) vec = vec && gate->gate_col[i] % 8 == 0;
    if (vec)
        hipLaunchKernelGGL(gate_res_bwd_kernel, dim3((unsigned)((total / 8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)dout, ld_dout, stride_dout,
                           (const bf16_t*)y, ldy, strideY, (bf16_t*)dy, ld_dy, stride_dy, tokens, dim, batch, *gate, t_dgate, t_row0);
    else
        hipLaunchKernelGGL(gate_res_bwd_scalar_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)dout, ld_dout, stride_dout,
                           (const bf16_t*)y, ldy, strideY, (bf16_t*)dy, ld_dy, stride_dy, tokens, dim, batch, *gate, t_dgate, t_row0);
    TG_LAUNCH_CHECK("tg_gate_residual_bwd");
    return TG_OK;
}

extern "C" int tg_act(const void* x, const void* dy, void* out, long n, int mode, hipStream_t stream) {
    TG_REQUIRE(x && out && (mode != 1 || dy), TG_ERR_ARG, "tg_act: null pointer");
    TG_REQUIRE(n > 0 && mode >= 0 && mode <= 2, TG_ERR_SHAPE, "tg_act: bad arguments");
    if (n % 8 == 0 && tg_aligned16(x) && tg_aligned16(out) && (!dy || tg_aligned16(dy)))
        hipLaunchKernelGGL(act_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)out, n / 8, mode);
    else
        hipLaunchKernelGGL(act_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)out, n, mode);
    TG_LAUNCH_CHECK("tg_act");
    return TG_OK;
}

extern "C" int tg_colsum_f32(const float* src, long ld, int rows, int cols, float* partial, hipStream_t stream) {
    TG_REQUIRE(src && partial, TG_ERR_ARG, "tg_colsum_f32: null pointer");
    TG_REQUIRE(rows > 0 && cols > 0 && ld >= cols, TG_ERR_SHAPE, "tg_colsum_f32: bad shape");
    const int CS_ROWS = cs_rows(rows, cols);
    hipLaunchKernelGGL(colsum_f32_kernel, dim3((unsigned)((rows + CS_ROWS - 1) / CS_ROWS), (unsigned)((cols + 255) / 256)), dim3(256), 0, stream, src, ld, rows, cols, partial,
                       CS_ROWS);
    TG_LAUNCH_CHECK("tg_colsum_f32");
    return TG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Optimizer step on a flat arena (train_cogvideo_to2v.py:2012-2021: clip_grad_norm_ on the transformer's parameters, AdamW, zero_grad).
// All HBM-bound streaming passes: 16-byte accesses, grid-stride, no host synchronisation (the clip coefficient stays on the device).
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int OPT_BLOCK = 256, OPT_PER_THREAD = 8, OPT_MAX_BLOCKS = 2048;

// acc[i] += scale * g[i]   (g bf16 or fp32): gradient accumulation over micro-steps (accelerate's `accumulate`: loss / accumulation steps)
template <bool SRC_BF16>
__global__ __launch_bounds__(OPT_BLOCK) void grad_accum_kernel(const void* __restrict__ g, float* __restrict__ acc, long n, float scale, int overwrite) {
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * OPT_BLOCK) {
        const float v = SRC_BF16 ? bf16_to_f32(((const bf16_t*)g)[i]) : ((const float*)g)[i];
        acc[i] = overwrite ? scale * v : acc[i] + scale * v;
    }
}

// One launch for a whole dictionary of gradients (a block's ~20 parameters were 20 launches of 5 us): the table travels BY VALUE in the kernel arguments (no device
// copy); workgroup w finds its item by a search over the cumulative block counts and covers OPT_BLOCK * 8 elements of it.
struct AccumTable {
    const void* src[TG_ACCUM_MAX];
    float* dst[TG_ACCUM_MAX];
    long n[TG_ACCUM_MAX];
    unsigned first_block[TG_ACCUM_MAX + 1];
    unsigned bf16_mask[(TG_ACCUM_MAX + 31) / 32];
    int count;
};
__global__ __launch_bounds__(OPT_BLOCK) void grad_accum_multi_kernel(AccumTable t, float scale) {
    int lo = 0, hi = t.count;                                  // first_block[lo] <= blockIdx.x < first_block[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blockIdx.x >= t.first_block[mid]) lo = mid; else hi = mid;
    }
    const long base = (long)(blockIdx.x - t.first_block[lo]) * (OPT_BLOCK * 8);
    const bool bf = (t.bf16_mask[lo >> 5] >> (lo & 31)) & 1u;
    float* acc = t.dst[lo];
    const long n = t.n[lo];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long i = base + (long)k * OPT_BLOCK + threadIdx.x;
        if (i < n) acc[i] += scale * (bf ? bf16_to_f32(((const bf16_t*)t.src[lo])[i]) : ((const float*)t.src[lo])[i]);
    }
}

__global__ __launch_bounds__(OPT_BLOCK) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ partial) {
    float a = 0.f;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * OPT_BLOCK) { const float v = g[i]; a += v * v; }
    a = wave_sum(a);
    __shared__ float red[OPT_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// coef[0] = total norm, coef[1] = min(1, max_norm / (norm + 1e-6))  (torch.nn.utils.clip_grad_norm_); fixed summation order
__global__ void clip_coef_kernel(const float* __restrict__ partial, int n_partial, float max_norm, float* __restrict__ coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n_partial; ++i) s += (double)partial[i];
    const float norm = (float)sqrt(s);
    coef[0] = norm;
    coef[1] = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
}

// torch.optim.AdamW (decoupled weight decay, bias correction, eps outside the corrected sqrt) on fp32 moments; parameters are bf16 and are
// read / written once (fp32 arithmetic in between).  clip: optional device pointer to the coefficient of clip_coef_kernel (coef + 1).
// The gradient is read and (zero_grad) zeroed through ONE pointer: two __restrict__ names for the same buffer would be undefined behaviour.
__global__ __launch_bounds__(OPT_BLOCK) void adamw_kernel(bf16_t* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                                                          float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                          const float* __restrict__ clip, int zero_grad) {
    const float cs = clip ? *clip : 1.f;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * OPT_BLOCK) {
        const float gi = g[i] * cs;
        float pi = bf16_to_f32(p[i]);
        pi *= 1.f - lr * wd;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi -= (lr / bc1) * (mi / denom);
        p[i] = f32_to_bf16(pi);
        if (zero_grad) g[i] = 0.f;
    }
}

// Prodigy (header: tg_prodigy_step).  Everything that depends on d is computed on the device from the fp64 state buffer, so a step never waits for the host.
enum { PD_D = 0, PD_DMAX = 1, PD_NUM = 2, PD_DHAT = 3, PD_DEN = 4, PD_DLR = 5, PD_SKIP = 6 };
struct ProdigyHyper {
    double lr, bc, beta1, beta2, beta3, eps, wd, d0, d_coef, growth;
    int safeguard;
};
typedef __attribute__((ext_vector_type(4))) float pd_f4;
typedef __attribute__((ext_vector_type(4))) unsigned short pd_h4;

// a + b summed over the wave in a fixed (butterfly) order: every lane ends with the same bits, every run with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Pass 1: the three EMAs and the two sums of the d estimate.  Four elements per lane and iteration (16-byte fp32 accesses, 8 bytes of p0); n4 = n / 4 and
// clip4 = clip_n / 4 are whole numbers of vectors (n, clip_n multiples of 64).  WD_GRAD: weight decay added to the gradient (not decoupled) — the only case in
// which this pass needs x itself, hence p0.  g is read and zeroed through one pointer (as adamw_kernel).
template <bool WD_GRAD>
__global__ __launch_bounds__(OPT_BLOCK) void prodigy_stats_kernel(float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ s,
                                                                  const float* __restrict__ delta, const bf16_t* __restrict__ p0, long n4, long clip4,
                                                                  const float* __restrict__ clip, const double* __restrict__ state, double* __restrict__ ws,
                                                                  ProdigyHyper h, int zero_grad) {
#pragma clang fp contract(off)      // every product and sum rounds as written: where b1 * m and a1 * g cancel, a fused form differs by many ulps of the result
    const double d = state[PD_D];
    const double dlr = d * h.lr * h.bc;
    const float a1 = (float)(d * (1.0 - h.beta1)), a2 = (float)(d * d * (1.0 - h.beta2)), a3 = (float)((d / h.d0) * (h.safeguard ? d : dlr));
    const float b1 = (float)h.beta1, b2 = (float)h.beta2, b3 = (float)h.beta3, wd = (float)h.wd;
    const float cs = clip ? *clip : 1.f;
    double num = 0.0, den = 0.0;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_BLOCK) {
        const pd_f4 gv = reinterpret_cast<const pd_f4*>(g)[i], dv = reinterpret_cast<const pd_f4*>(delta)[i];
        pd_f4 mv = reinterpret_cast<const pd_f4*>(m)[i], vv = reinterpret_cast<const pd_f4*>(v)[i], sv = reinterpret_cast<const pd_f4*>(s)[i];
        pd_h4 ph = {0, 0, 0, 0};
        if (WD_GRAD) ph = reinterpret_cast<const pd_h4*>(p0)[i];
        const float c = i < clip4 ? cs : 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gi = c * gv[k];
            if (WD_GRAD) gi += wd * (bf16_to_f32(ph[k]) + dv[k]);
            num += (double)gi * (double)(-dv[k]);
            mv[k] = b1 * mv[k] + a1 * gi;
            vv[k] = b2 * vv[k] + a2 * gi * gi;
            sv[k] = b3 * sv[k] + a3 * gi;
            den += (double)fabsf(sv[k]);
        }
        reinterpret_cast<pd_f4*>(m)[i] = mv;
        reinterpret_cast<pd_f4*>(v)[i] = vv;
        reinterpret_cast<pd_f4*>(s)[i] = sv;
        if (zero_grad) reinterpret_cast<pd_f4*>(g)[i] = pd_f4{0.f, 0.f, 0.f, 0.f};
    }
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    __shared__ double red[2 * (OPT_BLOCK / 64)];
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = num; red[2 * (threadIdx.x >> 6) + 1] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2 * (long)blockIdx.x] = ((red[0] + red[2]) + red[4]) + red[6];
        ws[2 * (long)blockIdx.x + 1] = ((red[1] + red[3]) + red[5]) + red[7];
    }
}

// Finalize: the partial pairs in index order, then prodigyopt's scalar rules, all fp64, one thread.
__global__ void prodigy_finalize_kernel(const double* __restrict__ ws, int n_partial, double* __restrict__ state, ProdigyHyper h) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sum = 0.0, den = 0.0;
    for (int i = 0; i < n_partial; ++i) { sum += ws[2 * i]; den += ws[2 * i + 1]; }
    if (den == 0.0) { state[PD_SKIP] = 1.0; return; }       // every gradient so far was zero: the EMAs are still zero, pass 2 returns at once
    double d = state[PD_D], d_max = state[PD_DMAX];
    const double dlr = d * h.lr * h.bc;
    const double num = h.beta3 * state[PD_NUM] + (d / h.d0) * dlr * sum;
    const double d_hat = h.d_coef * num / den;
    if (d == h.d0) d = fmax(d, d_hat);
    d_max = fmax(d_max, d_hat);
    d = fmin(d_max, d * h.growth);
    state[PD_D] = d; state[PD_DMAX] = d_max; state[PD_NUM] = num; state[PD_DHAT] = d_hat; state[PD_DEN] = den; state[PD_DLR] = dlr; state[PD_SKIP] = 0.0;
}

// Pass 2: the Adam-shaped update of the exact displacement with the d of THIS step in the denominator and the dlr of the d before it, then the parameter.
// WD_DEC: decoupled weight decay (on x = p0 + delta as it was before the update).
template <bool WD_DEC>
__global__ __launch_bounds__(OPT_BLOCK) void prodigy_update_kernel(bf16_t* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                                   float* __restrict__ delta, const bf16_t* __restrict__ p0, long n4,
                                                                   const double* __restrict__ state, double eps, double wd) {
#pragma clang fp contract(off)
    if (state[PD_SKIP] != 0.0) return;
    const float dlr = (float)state[PD_DLR], deps = (float)(state[PD_D] * eps), wdl = (float)(wd * state[PD_DLR]);
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_BLOCK) {
        const pd_f4 mv = reinterpret_cast<const pd_f4*>(m)[i], vv = reinterpret_cast<const pd_f4*>(v)[i];
        pd_f4 dv = reinterpret_cast<const pd_f4*>(delta)[i];
        const pd_h4 ph = reinterpret_cast<const pd_h4*>(p0)[i];
        pd_h4 po;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x0 = bf16_to_f32(ph[k]);
            float upd = dlr * (mv[k] / (sqrtf(vv[k]) + deps));
            if (WD_DEC) upd += wdl * (x0 + dv[k]);
            dv[k] -= upd;
            po[k] = f32_to_bf16(x0 + dv[k]);
        }
        reinterpret_cast<pd_f4*>(delta)[i] = dv;
        reinterpret_cast<pd_h4*>(p)[i] = po;
    }
}

// Stochastic bf16 rounding of the parameter write (header: tg_adamw_step_sr; not in the reference).  Philox4x32-10 (Salmon et al., SC'11)
// in plain integer arithmetic: the random bits of an element are a function of (seed, step, arena index) alone, so launch geometry, the two-segment
// launch of AdamW.step and the rank never enter them.  One call serves the 8 consecutive elements of arena group g = index >> 3.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
struct SrKey {
    uint32_t k0, k1, step;                                     // key = the seed's two halves; the step is counter word 2
};
__device__ __forceinline__ void sr_group_bits(const SrKey& key, long group, uint32_t (&w)[4]) {
    philox4x32_10((uint32_t)group, (uint32_t)((unsigned long long)group >> 32), key.step, 0u, key.k0, key.k1, w);
}
// the 16 random bits of element j (0..7) of a group; selects, no indexed register array (j is a constant wherever EPL == 8)
__device__ __forceinline__ uint32_t sr_r16(const uint32_t (&w)[4], int j) {
    const int h = j >> 1;
    const uint32_t ww = h == 0 ? w[0] : h == 1 ? w[1] : h == 2 ? w[2] : w[3];
    return (ww >> (16 * (j & 1))) & 0xffffu;
}
// x to one of its two bf16 neighbours, the magnitude away from zero with probability low16(bits) / 65536: E[result] = x.  A bf16-exact x is
// unchanged; NaN / Inf take the round-to-nearest conversion; a carry into the all-ones exponent is dropped (a finite x never becomes Inf).
__device__ __forceinline__ bf16_t f32_to_bf16_sr(float x, uint32_t r16) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) return f32_to_bf16(x);
    uint32_t s = u + r16;
    if ((s & 0x7f800000u) == 0x7f800000u) s = u;
    return (bf16_t)(s >> 16);
}

// Block-wise 8-bit AdamW (header: tg_adamw8bit_step).  One 256-lane workgroup per quantisation block of OPT_BLOCK * EPL elements, EPL contiguous
// elements per lane (16-byte bf16 / 2 x 16-byte fp32 / 8-byte code accesses at EPL = 8).  The workgroup finds its tensor by a binary search over the
// table's first_block (the same index in every lane: scalar loads).  A lane whose chunk starts inside the tensor reads its whole chunk: the chunk ends
// inside the tensor's 64-element-aligned arena slot, so the tail lane's extra elements are padding that is read, masked out and never written.
// SR (tg_adamw8bit_step_sr): the parameter write rounds stochastically with the bits of arena index a + k; a lane's chunk lies inside one group of 8
// (a is a multiple of EPL), so with EPL < 8 the 8 / EPL lanes of a group each compute the group's Philox and pick their own halves.  SR = false
// compiles to the code without it (sr is never read).
template <int EPL>
struct Chunk {
    typedef __attribute__((ext_vector_type(EPL))) float f;
    typedef __attribute__((ext_vector_type(EPL))) unsigned short h;
    typedef __attribute__((ext_vector_type(EPL))) unsigned char b;
};

// index of the nearest entry of the ascending 256-entry map q to x (ties: the lower index)
__device__ __forceinline__ int quantize_nearest(const float* q, float x) {
    int j = 0;
#pragma unroll
    for (int s = 128; s > 0; s >>= 1)
        if (q[j + s] <= x) j += s;                  // j = largest index with q[j] <= x (0 when x < q[0])
    j = j < 254 ? j : 254;
    return (q[j + 1] - x) < (x - q[j]) ? j + 1 : j;
}

template <int EPL, bool SR>
__global__ __launch_bounds__(OPT_BLOCK) void adamw8bit_kernel(bf16_t* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ s1, uint8_t* __restrict__ s2,
                                                              float* __restrict__ amax1, float* __restrict__ amax2, float* __restrict__ sm, float* __restrict__ sv,
                                                              const float* __restrict__ qmap1, const float* __restrict__ qmap2,
                                                              const tg_adamw8bit_row* __restrict__ rows, int nrows, float lr, float b1, float b2, float eps, float wd,
                                                              float bc1, float bc2_sqrt, const float* __restrict__ clip, int zero_grad, SrKey sr) {
    typedef typename Chunk<EPL>::f fv;
    typedef typename Chunk<EPL>::h hv;
    typedef typename Chunk<EPL>::b bv;
    __shared__ float q1[256], q2[256];
    __shared__ float red[2][OPT_BLOCK / 64];
    const int tid = threadIdx.x;
    q1[tid] = qmap1[tid];                                      // OPT_BLOCK == 256 == map entries
    q2[tid] = qmap2[tid];
    int lo = 0, hi = nrows;                                    // rows[lo].first_block <= blockIdx.x < rows[hi].first_block
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)blockIdx.x >= rows[mid].first_block) lo = mid; else hi = mid;
    }
    const long off = rows[lo].offset, n = rows[lo].numel, st = rows[lo].state, blk = (long)blockIdx.x - rows[lo].first_block;
    const int kind = rows[lo].kind;
    const float cs = (rows[lo].clipped && clip) ? *clip : 1.f;
    const long e0 = blk * (OPT_BLOCK * EPL) + (long)tid * EPL;   // first element of this lane's chunk, inside the tensor
    const int nv = e0 < n ? (n - e0 < EPL ? (int)(n - e0) : EPL) : 0;
    const long a = off + e0;                                   // its arena index
    float pf[EPL] = {}, gf[EPL] = {}, mf[EPL], vf[EPL];
    if (nv > 0) {
        const hv ph = *reinterpret_cast<const hv*>(p + a);
        const fv gg = *reinterpret_cast<const fv*>(g + a);
#pragma unroll
        for (int k = 0; k < EPL; ++k) { pf[k] = bf16_to_f32(ph[k]); gf[k] = gg[k]; }
    }
    if (kind == TG_ADAMW8BIT_FP32) {                           // uniform over the workgroup: no barrier below is skipped by part of it
        if (nv == 0) return;
        const fv mm = *reinterpret_cast<const fv*>(sm + st + e0), vv = *reinterpret_cast<const fv*>(sv + st + e0);
#pragma unroll
        for (int k = 0; k < EPL; ++k) { mf[k] = mm[k]; vf[k] = vv[k]; }
    } else {
        bv c1 = {}, c2 = {};
        if (nv > 0) { c1 = *reinterpret_cast<const bv*>(s1 + a); c2 = *reinterpret_cast<const bv*>(s2 + a); }
        const float am1 = amax1[st + blk], am2 = amax2[st + blk];
        __syncthreads();                                       // maps in LDS
#pragma unroll
        for (int k = 0; k < EPL; ++k) { mf[k] = q1[c1[k]] * am1; vf[k] = q2[c2[k]] * am2; }
    }
    // the tg_adamw_step arithmetic (adamw_kernel), fp32
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
        const float gi = gf[k] * cs;
        float pi = pf[k];
        pi *= 1.f - lr * wd;
        const float mi = b1 * mf[k] + (1.f - b1) * gi;
        const float vi = b2 * vf[k] + (1.f - b2) * gi * gi;
        mf[k] = mi; vf[k] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi -= (lr / bc1) * (mi / denom);
        pf[k] = pi;
    }
    if (kind == TG_ADAMW8BIT_FP32) {
        if (nv == EPL) {
            fv mm, vv;
#pragma unroll
            for (int k = 0; k < EPL; ++k) { mm[k] = mf[k]; vv[k] = vf[k]; }
            *reinterpret_cast<fv*>(sm + st + e0) = mm;
            *reinterpret_cast<fv*>(sv + st + e0) = vv;
        } else {
            for (int k = 0; k < nv; ++k) { sm[st + e0 + k] = mf[k]; sv[st + e0 + k] = vf[k]; }
        }
    } else {
        float x1 = 0.f, x2 = 0.f;                              // new absmax over the block's valid elements
#pragma unroll
        for (int k = 0; k < EPL; ++k)
            if (k < nv) { x1 = fmaxf(x1, fabsf(mf[k])); x2 = fmaxf(x2, fabsf(vf[k])); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { x1 = fmaxf(x1, __shfl_xor(x1, o, 64)); x2 = fmaxf(x2, __shfl_xor(x2, o, 64)); }
        if ((tid & 63) == 0) { red[0][tid >> 6] = x1; red[1][tid >> 6] = x2; }
        __syncthreads();
        x1 = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
        x2 = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        if (tid == 0) { amax1[st + blk] = x1; amax2[st + blk] = x2; }
        const float r1 = x1 > 0.f ? 1.f / x1 : 0.f, r2 = x2 > 0.f ? 1.f / x2 : 0.f;   // all-zero block: every element maps to 0.0
        bv c1, c2;
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            int c = quantize_nearest(q1, mf[k] * r1);
            if (mf[k] != 0.f && signbit(q1[c]) != signbit(mf[k])) c += mf[k] > 0.f ? 1 : -1;   // keep the sign of m (bitsandbytes)
            c1[k] = (unsigned char)c;
            c2[k] = (unsigned char)quantize_nearest(q2, vf[k] * r2);
        }
        if (nv == EPL) {
            *reinterpret_cast<bv*>(s1 + a) = c1;
            *reinterpret_cast<bv*>(s2 + a) = c2;
        } else {
            for (int k = 0; k < nv; ++k) { s1[a + k] = c1[k]; s2[a + k] = c2[k]; }
        }
    }
    uint32_t w[4] = {};
    if constexpr (SR) sr_group_bits(sr, a >> 3, w);
    const int j0 = EPL == 8 ? 0 : (int)(a & 7);                // EPL == 8: a is a multiple of 8 (the 16-byte accesses above)
    auto to_bf16 = [&](int k) -> bf16_t {
        if constexpr (SR) return f32_to_bf16_sr(pf[k], sr_r16(w, j0 + k));
        else return f32_to_bf16(pf[k]);
    };
    if (nv == EPL) {
        hv ph;
        fv z = {};
#pragma unroll
        for (int k = 0; k < EPL; ++k) ph[k] = to_bf16(k);
        *reinterpret_cast<hv*>(p + a) = ph;
        if (zero_grad) *reinterpret_cast<fv*>(g + a) = z;
    } else {
        for (int k = 0; k < nv; ++k) {
            p[a + k] = to_bf16(k);
            if (zero_grad) g[a + k] = 0.f;
        }
    }
}

// tg_adamw_step_sr: adamw_kernel's arithmetic with the stochastic parameter write.  A lane owns the 8 consecutive elements of one arena group (one
// Philox call per group; 16-byte bf16 / 2 x 16-byte fp32 accesses); elem0 = arena index of p[0], a multiple of 8, so group q of this segment is
// arena group elem0 / 8 + q.  The last group of a segment whose n is no multiple of 8 is stepped element by element and writes nothing past n.
__global__ __launch_bounds__(OPT_BLOCK) void adamw_sr_kernel(bf16_t* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                                                             float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                             const float* __restrict__ clip, int zero_grad, long group0, SrKey sr) {
    typedef Chunk<8>::f fv;
    typedef Chunk<8>::h hv;
    const float cs = clip ? *clip : 1.f;
    const long groups = (n + 7) >> 3;
    for (long q = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; q < groups; q += (long)gridDim.x * OPT_BLOCK) {
        const long i0 = q << 3;
        const int nv = n - i0 < 8 ? (int)(n - i0) : 8;
        float pf[8] = {}, gf[8] = {}, mf[8] = {}, vf[8] = {};
        if (nv == 8) {
            const hv ph = *reinterpret_cast<const hv*>(p + i0);
            const fv gg = *reinterpret_cast<const fv*>(g + i0), mm = *reinterpret_cast<const fv*>(m + i0), vv = *reinterpret_cast<const fv*>(v + i0);
#pragma unroll
            for (int k = 0; k < 8; ++k) { pf[k] = bf16_to_f32(ph[k]); gf[k] = gg[k]; mf[k] = mm[k]; vf[k] = vv[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < nv) { pf[k] = bf16_to_f32(p[i0 + k]); gf[k] = g[i0 + k]; mf[k] = m[i0 + k]; vf[k] = v[i0 + k]; }
        }
        uint32_t w[4];
        sr_group_bits(sr, group0 + q, w);
        bf16_t pb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {                          // the adamw_kernel expression, term for term
            const float gi = gf[k] * cs;
            float pi = pf[k];
            pi *= 1.f - lr * wd;
            const float mi = b1 * mf[k] + (1.f - b1) * gi;
            const float vi = b2 * vf[k] + (1.f - b2) * gi * gi;
            mf[k] = mi; vf[k] = vi;
            const float denom = sqrtf(vi) / bc2_sqrt + eps;
            pi -= (lr / bc1) * (mi / denom);
            pb[k] = f32_to_bf16_sr(pi, sr_r16(w, k));
        }
        if (nv == 8) {
            hv ph;
            fv mm, vv, z = {};
#pragma unroll
            for (int k = 0; k < 8; ++k) { ph[k] = pb[k]; mm[k] = mf[k]; vv[k] = vf[k]; }
            *reinterpret_cast<hv*>(p + i0) = ph;
            *reinterpret_cast<fv*>(m + i0) = mm;
            *reinterpret_cast<fv*>(v + i0) = vv;
            if (zero_grad) *reinterpret_cast<fv*>(g + i0) = z;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < nv) {
                    p[i0 + k] = pb[k]; m[i0 + k] = mf[k]; v[i0 + k] = vf[k];
                    if (zero_grad) g[i0 + k] = 0.f;
                }
        }
    }
}

inline unsigned opt_blocks(long n) { const long b = (n + OPT_BLOCK - 1) / OPT_BLOCK; return (unsigned)(b < OPT_MAX_BLOCKS ? (b > 0 ? b : 1) : OPT_MAX_BLOCKS); }
}  // namespace

extern "C" int tg_grad_accumulate(const void* grad, int grad_is_bf16, float* acc, long n, float scale, int overwrite, hipStream_t stream) {
    TG_REQUIRE(grad && acc, TG_ERR_ARG, "tg_grad_accumulate: null pointer");
    TG_REQUIRE(n > 0, TG_ERR_SHAPE, "tg_grad_accumulate: n must be positive");
    if (grad_is_bf16) hipLaunchKernelGGL(grad_accum_kernel<true>, dim3(opt_blocks(n)), dim3(OPT_BLOCK), 0, stream, grad, acc, n, scale, overwrite);
    else hipLaunchKernelGGL(grad_accum_kernel<false>, dim3(opt_blocks(n)), dim3(OPT_BLOCK), 0, stream, grad, acc, n, scale, overwrite);
    TG_LAUNCH_CHECK("tg_grad_accumulate");
    return TG_OK;
}

extern "C" int tg_grad_accumulate_multi(const tg_accum_item* items, int count, float scale, hipStream_t stream) {
    TG_REQUIRE(items && count > 0, TG_ERR_ARG, "tg_grad_accumulate_multi: no items");
    for (int i0 = 0; i0 < count; i0 += TG_ACCUM_MAX) {
        AccumTable t{};
        t.count = count - i0 < TG_ACCUM_MAX ? count - i0 : TG_ACCUM_MAX;
        unsigned nb = 0;
        for (int i = 0; i < t.count; ++i) {
            const tg_accum_item& it = items[i0 + i];
            TG_REQUIRE(it.grad && it.acc && it.n > 0, TG_ERR_ARG, "tg_grad_accumulate_multi: item %d: null pointer or empty", i0 + i);
            t.src[i] = it.grad; t.dst[i] = it.acc; t.n[i] = it.n;
            if (it.grad_is_bf16) t.bf16_mask[i >> 5] |= 1u << (i & 31);
            t.first_block[i] = nb;
            const long blocks = (it.n + OPT_BLOCK * 8 - 1) / (OPT_BLOCK * 8);
            TG_REQUIRE(blocks < (1L << 30) && nb + blocks < (1L << 31), TG_ERR_SHAPE, "tg_grad_accumulate_multi: too many elements");
            nb += (unsigned)blocks;
        }
        t.first_block[t.count] = nb;
        hipLaunchKernelGGL(grad_accum_multi_kernel, dim3(nb), dim3(OPT_BLOCK), 0, stream, t, scale);
    }
    TG_LAUNCH_CHECK("tg_grad_accumulate_multi");
    return TG_OK;
}

extern "C" long tg_grad_norm_ws_floats(void) { return OPT_MAX_BLOCKS; }

extern "C" int tg_grad_clip_coef(const float* grad, long n, float max_norm, float* ws, float* coef, hipStream_t stream) {
    TG_REQUIRE(grad && ws && coef, TG_ERR_ARG, "tg_grad_clip_coef: null pointer");
    TG_REQUIRE(n > 0, TG_ERR_SHAPE, "tg_grad_clip_coef: n must be positive");
    const unsigned nb = opt_blocks(n);
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(OPT_BLOCK), 0, stream, grad, n, ws);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, stream, (const float*)ws, (int)nb, max_norm, coef);
    TG_LAUNCH_CHECK("tg_grad_clip_coef");
    return TG_OK;
}

extern "C" int tg_adamw_step(void* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, int step, float lr, float beta1, float beta2, float eps,
                             float weight_decay, const float* clip_coef, int zero_grad, hipStream_t stream) {
    TG_REQUIRE(param && grad && exp_avg && exp_avg_sq, TG_ERR_ARG, "tg_adamw_step: null pointer");
    TG_REQUIRE(n > 0 && step >= 1, TG_ERR_SHAPE, "tg_adamw_step: n and step must be positive");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2s = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3(opt_blocks(n)), dim3(OPT_BLOCK), 0, stream, (bf16_t*)param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                       weight_decay, bc1, bc2s, clip_coef, zero_grad);
    TG_LAUNCH_CHECK("tg_adamw_step");
    return TG_OK;
}

extern "C" int tg_adamw_step_sr(void* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, int step, float lr, float beta1, float beta2, float eps,
                                float weight_decay, const float* clip_coef, int zero_grad, long elem0, unsigned long long seed, hipStream_t stream) {
    TG_REQUIRE(param && grad && exp_avg && exp_avg_sq, TG_ERR_ARG, "tg_adamw_step_sr: null pointer");
    TG_REQUIRE(n > 0 && step >= 1, TG_ERR_SHAPE, "tg_adamw_step_sr: n and step must be positive");
    TG_REQUIRE(elem0 >= 0 && elem0 % 8 == 0, TG_ERR_SHAPE, "tg_adamw_step_sr: elem0 %ld must be a non-negative multiple of 8 (one Philox call per 8 arena elements)", elem0);
    TG_REQUIRE(tg_aligned16(param) && tg_aligned16(grad) && tg_aligned16(exp_avg) && tg_aligned16(exp_avg_sq), TG_ERR_ALIGN,
               "tg_adamw_step_sr: arenas must be 16-byte aligned");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2s = sqrtf(1.f - powf(beta2, (float)step));
    const SrKey sr = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)step};
    hipLaunchKernelGGL(adamw_sr_kernel, dim3(opt_blocks((n + 7) / 8)), dim3(OPT_BLOCK), 0, stream, (bf16_t*)param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2,
                       eps, weight_decay, bc1, bc2s, clip_coef, zero_grad, elem0 / 8, sr);
    TG_LAUNCH_CHECK("tg_adamw_step_sr");
    return TG_OK;
}

extern "C" long tg_prodigy_ws_doubles(void) { return 2L * OPT_MAX_BLOCKS; }

extern "C" int tg_prodigy_step(void* param, float* grad, float* exp_avg, float* exp_avg_sq, float* s, float* delta, const void* p0, double* state, double* ws,
                               long n, long clip_n, int step, double lr, double beta1, double beta2, double beta3, double eps, double weight_decay, double d0,
                               double d_coef, double growth_rate, int decouple, int use_bias_correction, int safeguard_warmup, const float* clip_coef,
                               int zero_grad, hipStream_t stream) {
    TG_REQUIRE(param && grad && exp_avg && exp_avg_sq && s && delta && p0 && state && ws, TG_ERR_ARG, "tg_prodigy_step: null pointer");
    TG_REQUIRE(n > 0 && step >= 1, TG_ERR_SHAPE, "tg_prodigy_step: n and step must be positive");
    TG_REQUIRE(clip_n >= 0 && clip_n <= n, TG_ERR_SHAPE, "tg_prodigy_step: clip_n %ld outside [0, %ld]", clip_n, n);
    TG_REQUIRE(n % 64 == 0 && clip_n % 64 == 0, TG_ERR_SHAPE, "tg_prodigy_step: n %ld and clip_n %ld must be multiples of 64 (arena slots)", n, clip_n);
    TG_REQUIRE(lr > 0.0 && eps > 0.0 && d0 > 0.0, TG_ERR_SHAPE, "tg_prodigy_step: lr, eps and d0 must be positive (a step at lr 0 is the caller's no-op)");
    TG_REQUIRE(tg_aligned16(grad) && tg_aligned16(exp_avg) && tg_aligned16(exp_avg_sq) && tg_aligned16(s) && tg_aligned16(delta) && tg_aligned16(param) &&
               tg_aligned16(p0) && tg_aligned16(state) && tg_aligned16(ws), TG_ERR_ALIGN, "tg_prodigy_step: arenas must be 16-byte aligned");
    ProdigyHyper h;
    h.lr = lr; h.beta1 = beta1; h.beta2 = beta2; h.beta3 = beta3; h.eps = eps; h.wd = weight_decay; h.d0 = d0; h.d_coef = d_coef; h.growth = growth_rate;
    h.bc = use_bias_correction ? sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step)) : 1.0;
    h.safeguard = safeguard_warmup ? 1 : 0;
    const long n4 = n / 4, clip4 = clip_n / 4;
    const unsigned nb = opt_blocks(n4);
    const bool wd_grad = weight_decay != 0.0 && !decouple, wd_dec = weight_decay != 0.0 && decouple;
    if (wd_grad)
        hipLaunchKernelGGL(prodigy_stats_kernel<true>, dim3(nb), dim3(OPT_BLOCK), 0, stream, grad, exp_avg, exp_avg_sq, s, (const float*)delta, (const bf16_t*)p0, n4,
                           clip4, clip_coef, (const double*)state, ws, h, zero_grad);
    else
        hipLaunchKernelGGL(prodigy_stats_kernel<false>, dim3(nb), dim3(OPT_BLOCK), 0, stream, grad, exp_avg, exp_avg_sq, s, (const float*)delta, (const bf16_t*)p0, n4,
                           clip4, clip_coef, (const double*)state, ws, h, zero_grad);
    hipLaunchKernelGGL(prodigy_finalize_kernel, dim3(1), dim3(64), 0, stream, (const double*)ws, (int)nb, state, h);
    if (wd_dec)
        hipLaunchKernelGGL(prodigy_update_kernel<true>, dim3(nb), dim3(OPT_BLOCK), 0, stream, (bf16_t*)param, (const float*)exp_avg, (const float*)exp_avg_sq, delta,
                           (const bf16_t*)p0, n4, (const double*)state, eps, weight_decay);
    else
        hipLaunchKernelGGL(prodigy_update_kernel<false>, dim3(nb), dim3(OPT_BLOCK), 0, stream, (bf16_t*)param, (const float*)exp_avg, (const float*)exp_avg_sq, delta,
                           (const bf16_t*)p0, n4, (const double*)state, eps, weight_decay);
    TG_LAUNCH_CHECK("tg_prodigy_step");
    return TG_OK;
}

namespace {
// tg_adamw8bit_step / tg_adamw8bit_step_sr: the checks and the launch; `sr` NULL = round to nearest (the kernel instantiation without the generator)
int adamw8bit_launch(const char* who, void* param, float* grad, uint8_t* state1, uint8_t* state2, float* absmax1, float* absmax2, float* small_m, float* small_v,
                     const float* qmap1, const float* qmap2, const tg_adamw8bit_row* rows, int nrows, long nblocks, int block_size, int step, float lr,
                     float beta1, float beta2, float eps, float weight_decay, const float* clip_coef, int zero_grad, const SrKey* sr, hipStream_t stream) {
    TG_REQUIRE(param && grad && state1 && state2 && absmax1 && absmax2 && small_m && small_v && qmap1 && qmap2 && rows, TG_ERR_ARG, "%s: null pointer", who);
    TG_REQUIRE(nrows > 0 && nblocks > 0 && step >= 1, TG_ERR_SHAPE, "%s: nrows, nblocks and step must be positive", who);
    TG_REQUIRE(nblocks < (1L << 31), TG_ERR_SHAPE, "%s: %ld workgroups", who, nblocks);
    TG_REQUIRE(block_size == OPT_BLOCK || block_size == 2 * OPT_BLOCK || block_size == 4 * OPT_BLOCK || block_size == 8 * OPT_BLOCK, TG_ERR_SHAPE,
               "%s: block_size %d not in {256, 512, 1024, 2048}", who, block_size);
    TG_REQUIRE(tg_aligned16(param) && tg_aligned16(grad) && tg_aligned16(state1) && tg_aligned16(state2) && tg_aligned16(small_m) && tg_aligned16(small_v),
               TG_ERR_ALIGN, "%s: arenas must be 16-byte aligned", who);
    const float bc1 = 1.f - powf(beta1, (float)step), bc2s = sqrtf(1.f - powf(beta2, (float)step));
    const SrKey key = sr ? *sr : SrKey{0u, 0u, 0u};
#define TG_ADAM8_LAUNCH(E, SR)                                                                                                                              \
    hipLaunchKernelGGL((adamw8bit_kernel<E, SR>), dim3((unsigned)nblocks), dim3(OPT_BLOCK), 0, stream, (bf16_t*)param, grad, state1, state2, absmax1, absmax2, \
                       small_m, small_v, qmap1, qmap2, rows, nrows, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, clip_coef, zero_grad, key)
#define TG_ADAM8_SWITCH(SR)                     \
    switch (block_size / OPT_BLOCK) {           \
        case 1: TG_ADAM8_LAUNCH(1, SR); break;  \
        case 2: TG_ADAM8_LAUNCH(2, SR); break;  \
        case 4: TG_ADAM8_LAUNCH(4, SR); break;  \
        default: TG_ADAM8_LAUNCH(8, SR); break; \
    }
    if (sr) { TG_ADAM8_SWITCH(true) } else { TG_ADAM8_SWITCH(false) }
#undef TG_ADAM8_SWITCH
#undef TG_ADAM8_LAUNCH
    TG_LAUNCH_CHECK(who);
    return TG_OK;
}
}  // namespace

extern "C" int tg_adamw8bit_step(void* param, float* grad, uint8_t* state1, uint8_t* state2, float* absmax1, float* absmax2, float* small_m, float* small_v,
                                 const float* qmap1, const float* qmap2, const tg_adamw8bit_row* rows, int nrows, long nblocks, int block_size, int step,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, const float* clip_coef, int zero_grad, hipStream_t stream) {
    return adamw8bit_launch("tg_adamw8bit_step", param, grad, state1, state2, absmax1, absmax2, small_m, small_v, qmap1, qmap2, rows, nrows, nblocks, block_size,
                            step, lr, beta1, beta2, eps, weight_decay, clip_coef, zero_grad, nullptr, stream);
}

extern "C" int tg_adamw8bit_step_sr(void* param, float* grad, uint8_t* state1, uint8_t* state2, float* absmax1, float* absmax2, float* small_m, float* small_v,
                                    const float* qmap1, const float* qmap2, const tg_adamw8bit_row* rows, int nrows, long nblocks, int block_size, int step,
                                    float lr, float beta1, float beta2, float eps, float weight_decay, const float* clip_coef, int zero_grad,
                                    unsigned long long seed, hipStream_t stream) {
    const SrKey sr = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)step};
    return adamw8bit_launch("tg_adamw8bit_step_sr", param, grad, state1, state2, absmax1, absmax2, small_m, small_v, qmap1, qmap2, rows, nrows, nblocks, block_size,
                            step, lr, beta1, beta2, eps, weight_decay, clip_coef, zero_grad, &sr, stream);
}
