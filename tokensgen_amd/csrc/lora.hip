// LoRA on the DiT attention projections (peft LoraLayer on nn.Linear; train_cogvideo_to2v.py:1326-1338 adds the adapters, :1345-1416 saves / loads them).
//   tg_lora_wgrad: the low-rank weight gradient G = beta G + scale Y^T T, reduced over the TOKEN axis (35 552 rows at the training shape) into a 3072 x 128
//                  output.  Y [M][N] and T [M][R] are read once in their natural row-major layout; a workgroup owns 64 columns of Y and a range of token
//                  rows, transposes 64-row tiles into LDS ([column][token], so both MFMA operands are token-contiguous ds_read_b128 fragments), accumulates
//                  in fp32 on v_mfma_f32_32x32x16_bf16 and leaves a partial [64][R] block; a second kernel adds the partials in range order.  The cut of
//                  the token axis depends on the shape only: same inputs, same bits.
//   tg_lora_merge: W' = bf16(W + scale B A), one rounding (diffusers fuse_lora on a bf16 model).  The sum runs in fp64: where W and scale B A cancel, an fp32
//                  sum's error is many bf16 ulps of the small result; in fp64 every element is the correctly rounded value or its neighbour.  168 launches per load.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int LW_ROWS = 64;        // token rows per LDS tile
constexpr int LW_COLS = 64;        // columns of Y per workgroup
constexpr int LW_PITCH = 72;       // LDS row pitch in elements (144 B: the sixteen lanes of a ds_read_b128 group fall on distinct banks)
constexpr int LW_TARGET_WG = 512;  // workgroups the token axis is cut for (a constant, NOT the device's CU count: the summation order is a function of the shape)

struct WgradParams {
    const bf16_t* Y; long ldy, sYb;
    const bf16_t* T; long ldt, sTb;
    int M;                         // rows per batch item
    long Mtot;                     // batch * M
    int N, R;
    float* part;                   // [splits][N][R]
    int ntiles;                    // N / 64
    long rps;                      // token rows per split (a multiple of 64)
};

// token-axis cut: (splits, rows per split) from the shape alone
inline void wgrad_cut(long Mtot, int N, int* splits, long* rps) {
    const long tiles = (Mtot + LW_ROWS - 1) / LW_ROWS;
    long s = LW_TARGET_WG / (N / LW_COLS);
    if (s < 1) s = 1;
    if (s > tiles) s = tiles;
    const long tps = (tiles + s - 1) / s;
    *splits = (int)((tiles + tps - 1) / tps);
    *rps = tps * LW_ROWS;
}

template <int JB>                  // R = 64 JB
__global__ __launch_bounds__(256) void lora_wgrad_kernel(WgradParams p) {
    constexpr int R = 64 * JB, NU = 64 + R, ROUNDS = (NU + 255) / 256;
    __shared__ __attribute__((aligned(16))) bf16_t smem[(64 + R) * LW_PITCH];     // rows 0..63: Y^T [column][token]; rows 64..: T^T [rank column][token]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i31 = lane & 31, hi = lane >> 5, wn = wave & 1, wj = wave >> 1;
    // XCD-aware: the workgroups of one token range (they all read the same rows of T) sit on one XCD's L2
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int split = lid / p.ntiles, n0 = (lid - split * p.ntiles) * LW_COLS;
    const long r0 = (long)split * p.rps, r1 = min(p.Mtot, r0 + p.rps);

    // a "unit" is an [8 tokens][8 columns] block: eight 16-byte row loads, transposed in registers, eight 16-byte LDS writes
    const bf16_t* src[ROUNDS];
    long ld[ROUNDS], sb[ROUNDS];
    int col[ROUNDS], mg[ROUNDS], lrow[ROUNDS];
    bool on[ROUNDS];
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int u = tid + rd * 256;
        on[rd] = u < NU;
        if (u < 64) {
            src[rd] = p.Y; ld[rd] = p.ldy; sb[rd] = p.sYb;
            mg[rd] = u >> 3; col[rd] = n0 + 8 * (u & 7); lrow[rd] = 8 * (u & 7);
        } else {
            const int t = u - 64, jg = t % (R / 8);
            src[rd] = p.T; ld[rd] = p.ldt; sb[rd] = p.sTb;
            mg[rd] = t / (R / 8); col[rd] = 8 * jg; lrow[rd] = 64 + 8 * jg;
        }
    }
    uint32_t v[ROUNDS][8][4];
    auto load = [&](long t0) {
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            if (!on[rd]) continue;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const long g = t0 + 8 * mg[rd] + r;
                uint4 q = make_uint4(0u, 0u, 0u, 0u);
                if (g < r1) {                                  // rows past the range (and past the matrix) count as zeros, never read
                    const unsigned b = (unsigned)g / (unsigned)p.M, m = (unsigned)g - b * (unsigned)p.M;
                    q = *(const uint4*)(src[rd] + (long)b * sb[rd] + (long)m * ld[rd] + col[rd]);
                }
                v[rd][r][0] = q.x; v[rd][r][1] = q.y; v[rd][r][2] = q.z; v[rd][r][3] = q.w;
            }
        }
    };

    f32x16 acc[JB];
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jb][r] = 0.f;

    load(r0);
    for (long t0 = r0; t0 < r1; t0 += LW_ROWS) {
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            if (!on[rd]) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e) {                      // column e of the unit: its eight token values, packed two per dword
                uint4 o;
                uint32_t d[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t a = v[rd][2 * k][e >> 1], b = v[rd][2 * k + 1][e >> 1];
                    d[k] = (e & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
                }
                o.x = d[0]; o.y = d[1]; o.z = d[2]; o.w = d[3];
                *(uint4*)(smem + (lrow[rd] + e) * LW_PITCH + 8 * mg[rd]) = o;
            }
        }
        __syncthreads();
        if (t0 + LW_ROWS < r1) load(t0 + LW_ROWS);             // the next tile's rows are in flight while this one is multiplied
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 fy = *(const bf16x8*)(smem + (wn * 32 + i31) * LW_PITCH + ks * 16 + 8 * hi);
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                const bf16x8 ft = *(const bf16x8*)(smem + (64 + (wj * JB + jb) * 32 + i31) * LW_PITCH + ks * 16 + 8 * hi);
                acc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fy, ft, acc[jb], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // lane (i31, hi), register r holds D[column of Y = 8 (r / 4) + 4 hi + r % 4][rank column = i31] of the wave's 32 x 32 block
    float* dst = p.part + ((long)split * p.N + n0 + wn * 32) * R;
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(long)((r >> 2) * 8 + hi * 4 + (r & 3)) * R + (wj * JB + jb) * 32 + i31] = acc[jb][r];
}

// G[n][j] = beta G[n][j] + scale * (partials summed in range order)
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* part, int splits, long NR, int R, float* G, long gsn, long gsj, float beta, float scale) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= NR) return;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += part[(long)sp * NR + idx];
    const long n = idx / R, j = idx - n * R;
    float* g = G + n * gsn + j * gsj;
    float o = scale * s;
    if (beta != 0.f) o += beta * *g;                           // beta == 0: G is write-only (it may hold anything)
    *g = o;
}

// W'[n][k] = bf16(W[n][k] + scale sum_j B[n][j] A[j][k]): 64 x 64 outputs per workgroup, 4 x 4 per thread, fp64 FMAs in a fixed order
__global__ __launch_bounds__(256) void lora_merge_kernel(const bf16_t* W, long ldw, const bf16_t* B, long ldb, const bf16_t* A, long lda, bf16_t* O, long ldo,
                                                         int N, int K, int R, float scale) {
    __shared__ float Bs[32][65];                               // [j][n]
    __shared__ float As[32][64];                               // [j][k]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    double acc[4][4];
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) acc[y][x] = 0.0;
    for (int j0 = 0; j0 < R; j0 += 32) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = tid + it * 256;
            const int bn = idx >> 5, bj = idx & 31;
            Bs[bj][bn] = (n0 + bn < N && j0 + bj < R) ? bf16_to_f32(B[(long)(n0 + bn) * ldb + j0 + bj]) : 0.f;
            const int aj = idx >> 6, ak = idx & 63;
            As[aj][ak] = (k0 + ak < K && j0 + aj < R) ? bf16_to_f32(A[(long)(j0 + aj) * lda + k0 + ak]) : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
            double a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) a[x] = As[j][tx * 4 + x];
#pragma unroll
            for (int y = 0; y < 4; ++y) b[y] = Bs[j][ty * 4 + y];
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) acc[y][x] = fma(b[y], a[x], acc[y][x]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int n = n0 + ty * 4 + y, k = k0 + tx * 4 + x;
            if (n < N && k < K) {
                const bf16_t w = W[(long)n * ldw + k];
                const double d = (double)scale * acc[y][x];
                O[(long)n * ldo + k] = d == 0.0 ? w : f32_to_bf16((float)((double)bf16_to_f32(w) + d));      // a zero update returns W's own bits (-0 included)
            }
        }
}

}  // namespace

extern "C" long tg_lora_wgrad_ws_floats(int rows, int N, int R) {
    if (rows <= 0 || N <= 0 || R <= 0 || N % LW_COLS != 0) return 0;
    int splits; long rps;
    wgrad_cut(rows, N, &splits, &rps);
    return (long)splits * N * R;
}

extern "C" int tg_lora_wgrad(const void* Y, long ldy, long y_batch_stride, const void* T, long ldt, long t_batch_stride, int M, int batch, int N, int R,
                             float* G, long g_stride_n, long g_stride_j, float beta, float scale, float* ws, hipStream_t stream) {
    TG_REQUIRE(Y && T && G && ws, TG_ERR_ARG, "tg_lora_wgrad: null pointer");
    TG_REQUIRE(M > 0 && batch > 0 && N > 0 && R > 0, TG_ERR_SHAPE, "tg_lora_wgrad: M=%d batch=%d N=%d R=%d must be positive", M, batch, N, R);
    TG_REQUIRE(N % LW_COLS == 0, TG_ERR_SHAPE, "tg_lora_wgrad: N=%d must be a multiple of 64", N);
    TG_REQUIRE(R % 64 == 0 && R <= 384, TG_ERR_SHAPE, "tg_lora_wgrad: R=%d must be a multiple of 64, at most 384", R);
    TG_REQUIRE((long)M * batch < (1L << 31), TG_ERR_SHAPE, "tg_lora_wgrad: batch * M = %ld rows do not fit 31 bits", (long)M * batch);
    TG_REQUIRE(ldy >= N && ldt >= R, TG_ERR_SHAPE, "tg_lora_wgrad: row strides ldy=%ld / ldt=%ld shorter than N=%d / R=%d", ldy, ldt, N, R);
    TG_REQUIRE(tg_aligned16(Y) && tg_aligned16(T) && ldy % 8 == 0 && ldt % 8 == 0 && y_batch_stride % 8 == 0 && t_batch_stride % 8 == 0, TG_ERR_ALIGN,
               "tg_lora_wgrad: Y / T and their strides must be 16-byte aligned");
    TG_REQUIRE((((uintptr_t)G) & 3) == 0 && tg_aligned16(ws), TG_ERR_ALIGN, "tg_lora_wgrad: G / ws misaligned");
    WgradParams p;
    p.Y = (const bf16_t*)Y; p.ldy = ldy; p.sYb = y_batch_stride;
    p.T = (const bf16_t*)T; p.ldt = ldt; p.sTb = t_batch_stride;
    p.M = M; p.Mtot = (long)M * batch; p.N = N; p.R = R; p.part = ws; p.ntiles = N / LW_COLS;
    int splits;
    wgrad_cut(p.Mtot, N, &splits, &p.rps);
    const dim3 grid((unsigned)(p.ntiles * splits)), block(256);
    switch (R / 64) {
        case 1: hipLaunchKernelGGL(lora_wgrad_kernel<1>, grid, block, 0, stream, p); break;
        case 2: hipLaunchKernelGGL(lora_wgrad_kernel<2>, grid, block, 0, stream, p); break;
        case 3: hipLaunchKernelGGL(lora_wgrad_kernel<3>, grid, block, 0, stream, p); break;
        case 4: hipLaunchKernelGGL(lora_wgrad_kernel<4>, grid, block, 0, stream, p); break;
        case 5: hipLaunchKernelGGL(lora_wgrad_kernel<5>, grid, block, 0, stream, p); break;
        default: hipLaunchKernelGGL(lora_wgrad_kernel<6>, grid, block, 0, stream, p); break;
    }
    TG_LAUNCH_CHECK("tg_lora_wgrad");
    const long NR = (long)N * R;
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, stream, (const float*)ws, splits, NR, R, G, g_stride_n, g_stride_j,
                       beta, scale);
    TG_LAUNCH_CHECK("tg_lora_wgrad (reduce)");
    return TG_OK;
}

extern "C" int tg_lora_merge(const void* W, long ldw, const void* B, long ldb, const void* A, long lda, void* W_out, long ldo, int N, int K, int R, float scale,
                             hipStream_t stream) {
    TG_REQUIRE(W && B && A && W_out, TG_ERR_ARG, "tg_lora_merge: null pointer");
    TG_REQUIRE(N > 0 && K > 0 && R > 0, TG_ERR_SHAPE, "tg_lora_merge: N=%d K=%d R=%d must be positive", N, K, R);
    TG_REQUIRE(ldw >= K && ldo >= K && ldb >= R && lda >= K, TG_ERR_SHAPE, "tg_lora_merge: a row stride is shorter than its row (ldw=%ld ldo=%ld ldb=%ld lda=%ld)", ldw, ldo,
               ldb, lda);
    TG_REQUIRE((N + 63) / 64 <= 65535, TG_ERR_SHAPE, "tg_lora_merge: N=%d too large", N);
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), 0, stream, (const bf16_t*)W, ldw, (const bf16_t*)B, ldb,
                       (const bf16_t*)A, lda, (bf16_t*)W_out, ldo, N, K, R, scale);
    TG_LAUNCH_CHECK("tg_lora_merge");
    return TG_OK;
}
