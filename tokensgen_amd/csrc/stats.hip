// Streaming statistics of the Resampler's condensed tokens for the T2To stage: what pca.pt / mean.pt / std.pt are fitted from (pca.py:40-58 `fit` / `transform`,
// consumed by train_cogvideo_t2to.py:1761-1773 `pca_normalization`).  Two passes over bf16 token rows X [rows][D]:
//   tg_gram_accumulate: G += X^T X, colsum += sum_r X[r] with fp64 running totals: the covariance G - n mu mu^T is diagonalised once on the host side.  A square TN
//                  product: both MFMA operands are COLUMN blocks of the same row-major slabs and the contraction runs over the slow (token) axis.  A workgroup
//                  owns one upper-triangle 128 x 128 tile for ALL rows: 32-row chunks of the two [32][128] slabs go to LDS as they lie in memory (coalesced 16-byte
//                  loads, no register transpose) and every operand fragment is a pair of ds_read_b64_tr_b16 transposed reads.  The fp32 MFMA accumulators are
//                  folded into fp64 registers every GRAM_FOLD rows, and the tile and its mirror are written once at the end: one owner per element pair, no
//                  atomics, no workspace; the summation order is a function of the shape alone.
//   tg_pca_coef_stats: y = (X - pmean) comp^T in fp32 (the arithmetic of tg_pca_project16 before its normalisation: fp32 inputs, so no MFMA), then per coefficient
//                  sum / sum of squares in fp64 and the signed value of largest magnitude (the u-based sign rule of pca.py:30-32 needs the row where |y_j| peaks:
//                  u[:, j] = y[:, j] / s_j).  64 rows per workgroup leave one partial each; a one-block kernel adds the partials in row order.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int GRAM_T = 128;        // tile edge (columns of X per slab)
constexpr int GRAM_KT = 32;        // token rows per LDS chunk (two k-steps of the 32x32x16 MFMA)
constexpr int GRAM_FOLD = 256;     // rows summed in fp32 before the partial joins the fp64 total
constexpr int GRAM_SLAB = GRAM_KT * GRAM_T;     // elements of one slab chunk (8 KiB)

// LDS image of a [32 tokens][128 columns] slab chunk: plain 256-byte rows, the sixteen 16-byte chunks of a row permuted by an XOR of the row's low four bits so
// that the 4 x 16 blocks of the transposed reads fall on distinct banks.  Byte offset of chunk `ch` of row `row`.
__device__ __forceinline__ uint32_t gram_off(int row, int ch) { return (uint32_t)(256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)))); }

__device__ __forceinline__ uint32_t gram_lds_addr(const void* p) { return (uint32_t)(uintptr_t)p; }      // the low 32 bits of a flat LDS address are the LDS offset

// the hardware delivers the 4 rows x 16 columns block, whose sixteen 8-byte pieces the 16 lanes of a group address, column-major: lane i of the group gets column i
__device__ __forceinline__ void gram_tr_read(uint2& dst, uint32_t addr) { asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(addr) : "memory"); }

union GramFrag {
    uint2 h[2];
    bf16x8 v;
};

__global__ __launch_bounds__(256) void gram_kernel(const bf16_t* __restrict__ X, long ldx, long rows, int D, int nblk, double* __restrict__ gram,
                                                   double* __restrict__ colsum) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 2 * GRAM_SLAB];      // [buffer][slab I | slab J][32][128], 32 KiB
    __shared__ double scol[GRAM_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i31 = lane & 31, hi = lane >> 5, wm = wave >> 1, wn = wave & 1;
    // upper-triangle tile (bi <= bj) of this workgroup: linear index -> (bi, bj), row bi holds nblk - bi tiles
    int t = blockIdx.x, bi = 0;
    while (t >= nblk - bi) { t -= nblk - bi; ++bi; }
    const int bj = bi + t;
    const bool diag = bi == bj;
    if (tid < GRAM_T) scol[tid] = 0.0;

    // staging: 1024 16-byte pieces per chunk (2 slabs x 32 rows x 16), four per thread; piece = (slab, row, ch)
    const bf16_t* src[4];
    int srow[4];
    uint32_t sdst[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = tid + 256 * k, slab = idx >> 9, row = (idx >> 4) & 31, ch = idx & 15;
        src[k] = X + (long)(slab ? bj : bi) * GRAM_T + 8 * ch;
        srow[k] = row;
        sdst[k] = (uint32_t)(slab * GRAM_SLAB * 2) + gram_off(row, ch);
    }
    uint4 v[4];
    auto load = [&](long r0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long g = r0 + srow[k];
            v[k] = make_uint4(0u, 0u, 0u, 0u);                 // rows past `rows` count as zeros and are never read
            if (g < rows) v[k] = *(const uint4*)(src[k] + g * ldx);
        }
    };

    // transposed-read addresses inside a slab chunk: group g = lane >> 4 reads, for half k-step n, the block of token rows 8 (g >> 1) + 4 n + {0..3} and
    // columns 32 cb + 16 (g & 1) + {0..15}; lane 4 q + p of the group addresses row q, columns 4 p .. 4 p + 3.  Lane (i31, hi) then holds column 32 cb + i31 at
    // tokens 8 hi + 4 n + {0..3}: elements 4 n .. 4 n + 3 of the 32x32x16 operand (A[row i31][k = 8 hi + j] and B[k = 8 hi + j][col i31] alike).
    const int q = (lane & 15) >> 2, p = lane & 3, half = (lane >> 4) & 1;
    uint32_t offA[2][2], offB[2][2];                           // [column block of the wave][n]
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int row = 8 * hi + 4 * n + q;
            offA[b][n] = gram_off(row, 4 * (2 * wm + b) + 2 * half + (p >> 1)) + 8 * (p & 1);
            offB[b][n] = (uint32_t)(GRAM_SLAB * 2) + gram_off(row, 4 * (2 * wn + b) + 2 * half + (p >> 1)) + 8 * (p & 1);
        }
    const uint32_t lds0 = gram_lds_addr(smem);

    f32x16 acc[2][2], cacc[2];
    double tot[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) cacc[a][r] = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[a][b][r] = 0.f;
                tot[a][b][r] = 0.0;
            }
    }
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (short)0x3f80;       // bf16 1.0: the column sums are one more MFMA against a block of ones

    auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[a][b][r] += (double)acc[a][b][r];
                    acc[a][b][r] = 0.f;
                }
        if (diag && wn == 0) {                                 // every column of the ones product holds the same sums: lanes i31 == 0 own them
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (i31 == 0) scol[32 * (2 * wm + a) + (r & 3) + 8 * (r >> 2) + 4 * hi] += (double)cacc[a][r];
                    cacc[a][r] = 0.f;
                }
        }
    };

    load(0);
    int buf = 0, infold = 0;
    for (long r0 = 0; r0 < rows; r0 += GRAM_KT) {
        bf16_t* sb = smem + buf * 2 * GRAM_SLAB;
#pragma unroll
        for (int k = 0; k < 4; ++k) *(uint4*)((char*)sb + sdst[k]) = v[k];
        __syncthreads();                                       // one barrier per chunk: the other buffer was last read before the previous barrier
        if (r0 + GRAM_KT < rows) load(r0 + GRAM_KT);           // the next chunk's rows are in flight while this one is multiplied
        const uint32_t base = lds0 + (uint32_t)(buf * 2 * GRAM_SLAB * 2);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            GramFrag fa[2], fb[2];
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    gram_tr_read(fa[b].h[n], base + offA[b][n] + (uint32_t)(ks * 16 * 256));
                    gram_tr_read(fb[b].h[n], base + offB[b][n] + (uint32_t)(ks * 16 * 256));
                }
            // the compiler cannot see the pending LDS reads: wait, and tie the fragments to the wait so that no use moves above it
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(fa[0].h[0]), "+v"(fa[0].h[1]), "+v"(fa[1].h[0]), "+v"(fa[1].h[1]), "+v"(fb[0].h[0]), "+v"(fb[0].h[1]), "+v"(fb[1].h[0]),
                           "+v"(fb[1].h[1])
                         :
                         : "memory");
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a].v, fb[b].v, acc[a][b], 0, 0, 0);
            if (diag && wn == 0) {
#pragma unroll
                for (int a = 0; a < 2; ++a) cacc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a].v, ones, cacc[a], 0, 0, 0);
            }
        }
        buf ^= 1;
        infold += GRAM_KT;
        if (infold == GRAM_FOLD) {
            fold();
            infold = 0;
        }
    }
    if (infold) fold();
    __syncthreads();

    // lane (i31, hi), register r of block (a, b) holds G[i][j], i = 128 bi + 32 (2 wm + a) + (r & 3) + 8 (r >> 2) + 4 hi, j = 128 bj + 32 (2 wn + b) + i31.
    // The new total is formed once, from the upper element, and stored to both places: gram stays bitwise symmetric.
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = GRAM_T * bi + 32 * (2 * wm + a) + (r & 3) + 8 * (r >> 2) + 4 * hi, j = GRAM_T * bj + 32 * (2 * wn + b) + i31;
                if (i <= j) {
                    const double g = gram[(long)i * D + j] + tot[a][b][r];
                    gram[(long)i * D + j] = g;
                    gram[(long)j * D + i] = g;
                }
            }
    if (diag && tid < GRAM_T) colsum[GRAM_T * bi + tid] += scol[tid];
}

// ---------------------------------------------------------------- tg_pca_coef_stats ----------------------------------------------------------------
constexpr int CS_ROWS = 64;        // token rows per workgroup
constexpr int CS_KC = 32;          // columns of X per LDS stage
constexpr int CS_XP = 68;          // pitch of the [k][row] image in floats (272 B: float4 reads stay aligned)
constexpr int CS_CP = 65;          // pitch of the [k][coefficient] image

// partial of one workgroup, as the reduce kernel reads it: [wg][5][ncoef] floats = sum (2 floats: a double), sumsq (2), extreme (1)
template <int NB>                  // ncoef = 16 NB
__global__ __launch_bounds__(256) void coef_stats_kernel(const bf16_t* __restrict__ X, long ldx, long rows, int D, const float* __restrict__ comp,
                                                         const float* __restrict__ pmean, float* __restrict__ ws) {
    constexpr int NC = 16 * NB;
    __shared__ __attribute__((aligned(16))) float xs[CS_KC * CS_XP];
    __shared__ float cs[CS_KC * CS_CP];
    __shared__ double rsum[16][NC], rsq[16][NC];
    __shared__ float rext[16][NC];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long r0 = (long)blockIdx.x * CS_ROWS;
    const int lr = tid & 63, lc = tid >> 6;                    // staging of X: row lr, columns 8 lc .. 8 lc + 7 of the stage
    const bool rowok = r0 + lr < rows;
    const bf16_t* xrow = X + (r0 + lr) * ldx + 8 * lc;
    float acc[4][NB];
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int m = 0; m < NB; ++m) acc[y][m] = 0.f;
    for (int c0 = 0; c0 < D; c0 += CS_KC) {
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (rowok) raw = *(const uint4*)(xrow + c0);           // rows past `rows` are never read
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xv = (e & 1) ? bf16hi_to_f32(w[e >> 1]) : bf16lo_to_f32(w[e >> 1]);
            xs[(8 * lc + e) * CS_XP + lr] = xv - pmean[c0 + 8 * lc + e];
        }
#pragma unroll
        for (int it = 0; it < (NC * CS_KC / 4 + 255) / 256; ++it) {
            const int idx = tid + 256 * it;                    // float4 piece: coefficient idx / 8, columns 4 (idx % 8) ..
            if (idx < NC * CS_KC / 4) {
                const int j = idx >> 3, k4 = (idx & 7) * 4;
                const float4 c = *(const float4*)(comp + (long)j * D + c0 + k4);
                cs[(k4 + 0) * CS_CP + j] = c.x; cs[(k4 + 1) * CS_CP + j] = c.y; cs[(k4 + 2) * CS_CP + j] = c.z; cs[(k4 + 3) * CS_CP + j] = c.w;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < CS_KC; ++k) {
            const float4 xv = *(const float4*)(xs + k * CS_XP + 4 * ty);
            const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                const float c = cs[k * CS_CP + tx + 16 * m];
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[y][m] = fmaf(x4[y], c, acc[y][m]);
            }
        }
        __syncthreads();
    }
    // thread (ty, tx): rows 4 ty .. 4 ty + 3, coefficients tx + 16 m; rows in ascending order, so the first row of a tie keeps the extreme
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        double s = 0.0, s2 = 0.0;
        float ex = 0.f;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            if (r0 + 4 * ty + y < rows) {
                const float yv = acc[y][m];
                s += (double)yv;
                s2 += (double)yv * (double)yv;
                if (fabsf(yv) > fabsf(ex)) ex = yv;
            }
        }
        rsum[ty][tx + 16 * m] = s; rsq[ty][tx + 16 * m] = s2; rext[ty][tx + 16 * m] = ex;
    }
    __syncthreads();
    if (tid < NC) {
        double s = 0.0, s2 = 0.0;
        float ex = 0.f;
        for (int g = 0; g < 16; ++g) {
            s += rsum[g][tid];
            s2 += rsq[g][tid];
            if (fabsf(rext[g][tid]) > fabsf(ex)) ex = rext[g][tid];
        }
        float* o = ws + (long)blockIdx.x * 5 * NC;
        *(double*)(o + 2 * tid) = s;
        *(double*)(o + 2 * NC + 2 * tid) = s2;
        o[4 * NC + tid] = ex;
    }
}

__global__ void coef_stats_reduce_kernel(const float* __restrict__ ws, long nwg, int NC, double* __restrict__ sum, double* __restrict__ sumsq,
                                         float* __restrict__ extreme) {
    const int j = threadIdx.x;
    if (j >= NC) return;
    double s = 0.0, s2 = 0.0;
    float ex = extreme[j];
    for (long g = 0; g < nwg; ++g) {                           // partials in row order
        const float* o = ws + g * 5 * NC;
        s += *(const double*)(o + 2 * j);
        s2 += *(const double*)(o + 2 * NC + 2 * j);
        const float e = o[4 * NC + j];
        if (fabsf(e) > fabsf(ex)) ex = e;
    }
    sum[j] += s;
    sumsq[j] += s2;
    extreme[j] = ex;
}

bool stats_shape_ok(long ldx, long rows, int D) { return D % GRAM_T == 0 && D >= 128 && D <= 4096 && rows >= 1 && ldx >= D; }

}  // namespace

extern "C" long tg_gram_fold_rows(void) { return GRAM_FOLD; }

extern "C" int tg_gram_accumulate(const void* x, long ldx, long rows, int D, double* gram, double* colsum, hipStream_t stream) {
    TG_REQUIRE(x && gram && colsum, TG_ERR_ARG, "tg_gram_accumulate: null pointer");
    TG_REQUIRE(stats_shape_ok(ldx, rows, D), TG_ERR_SHAPE, "tg_gram_accumulate: need D %% 128 == 0, 128 <= D <= 4096, rows >= 1, ldx >= D (rows=%ld D=%d ldx=%ld)", rows,
               D, ldx);
    TG_REQUIRE(tg_aligned16(x) && ldx % 8 == 0, TG_ERR_ALIGN, "tg_gram_accumulate: x and its row stride must be 16-byte aligned");
    TG_REQUIRE((((uintptr_t)gram) & 7) == 0 && (((uintptr_t)colsum) & 7) == 0, TG_ERR_ALIGN, "tg_gram_accumulate: gram / colsum misaligned");
    const int nblk = D / GRAM_T;
    hipLaunchKernelGGL(gram_kernel, dim3((unsigned)(nblk * (nblk + 1) / 2)), dim3(256), 0, stream, (const bf16_t*)x, ldx, rows, D, nblk, gram, colsum);
    TG_LAUNCH_CHECK("tg_gram_accumulate");
    return TG_OK;
}

extern "C" long tg_pca_coef_stats_ws_floats(long rows, int ncoef) {
    if (rows <= 0 || ncoef <= 0) return 0;
    return ((rows + CS_ROWS - 1) / CS_ROWS) * 5 * ncoef;
}

extern "C" int tg_pca_coef_stats(const void* x, long ldx, long rows, int D, const float* comp, int ncoef, const float* pmean, double* sum, double* sumsq,
                                 float* extreme, float* ws, hipStream_t stream) {
    TG_REQUIRE(x && comp && pmean && sum && sumsq && extreme && ws, TG_ERR_ARG, "tg_pca_coef_stats: null pointer");
    TG_REQUIRE(stats_shape_ok(ldx, rows, D), TG_ERR_SHAPE, "tg_pca_coef_stats: need D %% 128 == 0, 128 <= D <= 4096, rows >= 1, ldx >= D (rows=%ld D=%d ldx=%ld)", rows, D,
               ldx);
    TG_REQUIRE(ncoef % 16 == 0 && ncoef >= 16 && ncoef <= 64, TG_ERR_SHAPE, "tg_pca_coef_stats: ncoef=%d must be a multiple of 16 in 16..64", ncoef);
    TG_REQUIRE((rows + CS_ROWS - 1) / CS_ROWS < (1L << 31), TG_ERR_SHAPE, "tg_pca_coef_stats: rows=%ld too many for one launch", rows);
    TG_REQUIRE(tg_aligned16(x) && ldx % 8 == 0 && tg_aligned16(comp), TG_ERR_ALIGN, "tg_pca_coef_stats: x, its row stride and comp must be 16-byte aligned");
    TG_REQUIRE((((uintptr_t)sum) & 7) == 0 && (((uintptr_t)sumsq) & 7) == 0 && (((uintptr_t)ws) & 7) == 0, TG_ERR_ALIGN, "tg_pca_coef_stats: sum / sumsq / ws misaligned");
    const long nwg = (rows + CS_ROWS - 1) / CS_ROWS;
    const dim3 grid((unsigned)nwg), block(256);
    switch (ncoef / 16) {
        case 1: hipLaunchKernelGGL(coef_stats_kernel<1>, grid, block, 0, stream, (const bf16_t*)x, ldx, rows, D, comp, pmean, ws); break;
        case 2: hipLaunchKernelGGL(coef_stats_kernel<2>, grid, block, 0, stream, (const bf16_t*)x, ldx, rows, D, comp, pmean, ws); break;
        case 3: hipLaunchKernelGGL(coef_stats_kernel<3>, grid, block, 0, stream, (const bf16_t*)x, ldx, rows, D, comp, pmean, ws); break;
        default: hipLaunchKernelGGL(coef_stats_kernel<4>, grid, block, 0, stream, (const bf16_t*)x, ldx, rows, D, comp, pmean, ws); break;
    }
    TG_LAUNCH_CHECK("tg_pca_coef_stats");
    hipLaunchKernelGGL(coef_stats_reduce_kernel, dim3(1), dim3(64), 0, stream, (const float*)ws, nwg, ncoef, sum, sumsq, extreme);
    TG_LAUNCH_CHECK("tg_pca_coef_stats (reduce)");
    return TG_OK;
}
