// Which kernel the four GEMM entry points of gemm.hip launch for a shape, with what grid, block, LDS and tile order, and which shapes they refuse: ONE pure
// host function.  No HIP, no globals, no knob or device reads: the entry points pass the live TG_GEMM_W4 knob and the CU count in, a CPU test
// (tests/csrc/gemm_plan_table.cpp) passes its own.
#pragma once
#include <stdio.h>

#include "tg_errors.h"
#include "tokensgen_hip.h"      // the TG_EPI_* epilogue codes (plain C declarations only)

// ---- tile and LDS sizes that the kernels of gemm.hip and their launches share (a namespace: conv_plan.h has global BM, BN, BK, TILE_BYTES, STAGE_BYTES) ----
namespace gemm_cfg {
// gemm_bf16_kernel: 128x128x64 tile, 4 waves
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;          // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;      // A + W
// gemm256_kernel: 256x256x32 tile, 8 waves, a ring of 4 stages
constexpr int BM2 = 256, BN2 = 256, BK2 = 32, NS2 = 4;
constexpr int OPER2_BYTES = BM2 * BK2 * 2;       // 16 KiB per operand per stage
constexpr int STAGE2_BYTES = 2 * OPER2_BYTES;    // 32 KiB
constexpr int RING2_BYTES = NS2 * STAGE2_BYTES;  // 128 KiB
// gemm256w4_kernel: 256x256x64 tile, 4 waves, two stages
constexpr int BK3 = 64;
constexpr int OPER3_BYTES = 256 * BK3 * 2;       // 32 KiB per operand per stage
constexpr int STAGE3_BYTES = 2 * OPER3_BYTES;    // 64 KiB
constexpr int W4_STG_OFF = 2 * STAGE3_BYTES;     // epilogue staging behind the two stages
constexpr int W4_BIAS_OFF = W4_STG_OFF + 4 * 4096;   // 256 B of bias per wave
constexpr int W4_TOK_OFF = W4_BIAS_OFF + 4 * 256;    // gated-residual epilogue: group id of this wave's 128 rows, one dword each
constexpr int W4_GTAB_OFF = W4_TOK_OFF + 4 * 512;    // ... and the gate-row element offset of every group (16 dwords per wave)
constexpr int W4_LDS_BYTES = W4_GTAB_OFF + 4 * 64;
}  // namespace gemm_cfg

enum GemmEntry { GEMM_PLAIN, GEMM_PAIR, GEMM_QKV, GEMM_LORA };     // tg_gemm_bf16, tg_gemm_bf16_pair, tg_gemm_bf16_qkv, tg_gemm_bf16_lora

struct GemmShape {
    GemmEntry entry;
    int M, M2;
    bool second;                        // a second problem of M2 rows is present (pair: always; qkv: optional)
    int N, K, batch, epilogue, R, v_col0;
    long lda, ldw, ldt, ldb, vt_ld1, vt_ld2;
};

enum GemmKernel {          // the values are tg_gemm_kernel()'s answers (include/tokensgen_hip.h)
    GEMM_K128 = 0,         // gemm_bf16_kernel
    GEMM_K256W8 = 1,       // gemm256_kernel
    GEMM_K256W4 = 2,       // gemm256w4_kernel
};

struct GemmPlan {
    int err;                       // TG_OK, or the code of a refused shape with its text in msg
    char msg[256];
    GemmKernel kernel;
    unsigned grid;
    int block, lds;                // lds: dynamic LDS bytes of the launch
    int group_m;                   // m-tiles per n sweep of the 256^2 kernels' tile order (0: the 128x128 kernel has its own, fixed, order)
};

// the 256x256 kernels' shapes (large M; the 128x128 kernel takes the rest)
inline bool gemm_256_shape(int M, int N) { return M >= 1024 && N % gemm_cfg::BN2 == 0; }
// what the 4-wave kernel needs on top: two full stages of K in flight ...
inline bool gemm_w4_k(int K) { return K >= 4 * gemm_cfg::BK3; }
// ... and 32-bit buffer offsets: 256 rows * ld * 2 B < 2^31
inline bool gemm_w4_ld(long ld) { return ld < (1L << 21); }
// the 4-wave condition.  w4_knob: TG_GEMM_W4, 0 (cross-check tests) = the 8-wave kernel for every shape
inline bool gemm_w4_shape(int M, int N, int K, long lda, long ldw, int w4_knob) {
    return gemm_256_shape(M, N) && gemm_w4_k(K) && gemm_w4_ld(lda) && gemm_w4_ld(ldw) && w4_knob != 0;
}

#define GEMM_PLAN_REQUIRE(cond, code, ...)                   \
    do {                                                     \
        if (!(cond)) {                                       \
            pl.err = (code);                                 \
            snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__);   \
            return pl;                                       \
        }                                                    \
    } while (0)

inline GemmPlan gemm_plan(const GemmShape& s, int w4_knob, int n_cu) {
    using namespace gemm_cfg;
    GemmPlan pl{};
    const int M = s.M, M2 = s.M2, N = s.N, K = s.K, batch = s.batch;
    const char* name = "tg_gemm_bf16";
    // ---- the shapes each entry point refuses.  (The same fault, TG_GEMM_W4 = 0 where only the 4-wave kernel will do, is TG_ERR_ARG from the qkv entry and
    // TG_ERR_SHAPE from the lora entry and the activation epilogues: the codes are ABI and stay) ----
    switch (s.entry) {
        case GEMM_PLAIN:
            GEMM_PLAN_REQUIRE(M > 0 && N > 0 && K > 0 && batch > 0, TG_ERR_SHAPE, "tg_gemm_bf16: bad dims M=%d N=%d K=%d batch=%d", M, N, K, batch);
            GEMM_PLAN_REQUIRE(N % BN == 0 && K % BK == 0, TG_ERR_SHAPE, "tg_gemm_bf16: need N%%128==0 and K%%64==0 (N=%d K=%d)", N, K);
            GEMM_PLAN_REQUIRE(s.epilogue >= TG_EPI_BIAS && s.epilogue <= TG_EPI_BIAS_MUL_GELU_GRAD, TG_ERR_ARG, "tg_gemm_bf16: unknown epilogue %d", s.epilogue);
            GEMM_PLAN_REQUIRE((s.epilogue != TG_EPI_BIAS_KEEP_GELU && s.epilogue != TG_EPI_BIAS_MUL_GELU_GRAD) || gemm_w4_shape(M, N, K, s.lda, s.ldw, w4_knob), TG_ERR_SHAPE,
                              "tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%%256 == 0, K >= 256)");
            break;
        case GEMM_PAIR:
            name = "tg_gemm_bf16_pair";
            GEMM_PLAN_REQUIRE(gemm_256_shape(M, N) && M2 >= 1024 && N > 0 && K > 0 && batch > 0 && K % BK == 0, TG_ERR_SHAPE,
                              "tg_gemm_bf16_pair: both problems must be 256^2-kernel shapes (M >= 1024, N%%256 == 0, K%%64 == 0)");
            GEMM_PLAN_REQUIRE(s.epilogue == TG_EPI_BIAS || s.epilogue == TG_EPI_BIAS_GELU || s.epilogue == TG_EPI_BIAS_SILU, TG_ERR_ARG,
                              "tg_gemm_bf16_pair: bias / GELU / SiLU epilogues only");
            break;
        case GEMM_QKV:
            name = "tg_gemm_bf16_qkv";
            GEMM_PLAN_REQUIRE(gemm_256_shape(M, N) && (!s.second || M2 >= 1024) && N > 0 && batch > 0 && K % BK3 == 0 && gemm_w4_k(K), TG_ERR_SHAPE,
                              "tg_gemm_bf16_qkv: needs the 4-wave kernel's shapes (M >= 1024, N%%256 == 0, K%%64 == 0, K >= 256)");
            GEMM_PLAN_REQUIRE(s.v_col0 > 0 && s.v_col0 < N && s.v_col0 % BN2 == 0, TG_ERR_SHAPE, "tg_gemm_bf16_qkv: v_col0 must be a multiple of 256 inside (0, N)");
            GEMM_PLAN_REQUIRE(s.vt_ld1 % 64 == 0 && s.vt_ld1 >= M && (!s.second || (s.vt_ld2 % 64 == 0 && s.vt_ld2 >= M2)), TG_ERR_SHAPE,
                              "tg_gemm_bf16_qkv: vt_ld must be a multiple of 64 and >= M");
            GEMM_PLAN_REQUIRE(gemm_w4_ld(s.lda) && gemm_w4_ld(s.ldw), TG_ERR_SHAPE, "tg_gemm_bf16_qkv: leading dimensions must be < 2^21 elements");
            GEMM_PLAN_REQUIRE(w4_knob != 0, TG_ERR_ARG, "tg_gemm_bf16_qkv: only the 4-wave GEMM kernel has the V^T epilogue (TG_GEMM_W4=0 is set)");
            break;
        case GEMM_LORA:
            name = "tg_gemm_bf16_lora";
            GEMM_PLAN_REQUIRE(gemm_256_shape(M, N) && N > 0 && batch > 0 && K % BK3 == 0 && gemm_w4_k(K), TG_ERR_SHAPE,
                              "tg_gemm_bf16_lora: needs the 4-wave kernel's shapes (M >= 1024, N%%256 == 0, K%%64 == 0, K >= 256): M=%d N=%d K=%d batch=%d", M, N, K, batch);
            GEMM_PLAN_REQUIRE(s.R % BK3 == 0 && s.R >= BK3 && s.R <= 6 * BK3, TG_ERR_SHAPE, "tg_gemm_bf16_lora: the rank must be a multiple of 64 in 64..384 (R=%d)", s.R);
            GEMM_PLAN_REQUIRE(gemm_w4_ld(s.lda) && gemm_w4_ld(s.ldw) && gemm_w4_ld(s.ldt) && gemm_w4_ld(s.ldb) && s.lda >= K && s.ldw >= K && s.ldt >= s.R && s.ldb >= s.R,
                              TG_ERR_SHAPE, "tg_gemm_bf16_lora: leading dimensions must cover their rows and be < 2^21 elements");
            GEMM_PLAN_REQUIRE(w4_knob != 0, TG_ERR_SHAPE, "tg_gemm_bf16_lora: only the 4-wave GEMM kernel has the low-rank tail (TG_GEMM_W4=0 is set)");
            break;
    }
    // ---- the kernel: what the qkv and lora entries and the activation epilogues let through is a 4-wave shape ----
    const bool big = gemm_256_shape(M, N);
    const int tile = big ? BM2 : BM;       // both kinds of tile are square
    // (the kernels count their tiles in `int`: a launch with 2^31 of them or more was never valid)
    const long tiles = (((long)M + tile - 1) / tile + (s.second ? ((long)M2 + tile - 1) / tile : 0)) * (N / tile) * batch;
    GEMM_PLAN_REQUIRE(tiles < (1L << 31), TG_ERR_SHAPE, "%s: too many tiles", name);
    if (!big) {
        pl.kernel = GEMM_K128; pl.grid = (unsigned)tiles; pl.block = 256; pl.lds = 2 * STAGE_BYTES;
        return pl;
    }
    // the 256^2 kernels are persistent: one workgroup per CU walks the tile list (a second problem's tiles appended to the first one's).
    // tile order: groups of group_m m-tiles x all n-tiles, m fastest; the 32 tiles resident on one XCD then share group_m A panels and
    // 32/group_m W panels.  A (activations) is the big, XCD-private operand, W (weights) is shared by every XCD through the
    // Infinity Cache, so small groups win: measured sum over the four block GEMMs 7.61 (8) / 7.48 (4) / 7.53 (6) / 7.62 (2) ms,
    // and for K = 12288 (6.3 MB per A panel) a single m-tile per group is another 3 % faster (2.31 vs 2.34 vs 2.40 ms)
    pl.group_m = K >= 8192 ? 1 : 4;
    pl.grid = (unsigned)(tiles < n_cu ? tiles : n_cu);
    if (gemm_w4_shape(M, N, K, s.lda, s.ldw, w4_knob)) {
        pl.kernel = GEMM_K256W4; pl.block = 256; pl.lds = W4_LDS_BYTES;
    } else {
        pl.kernel = GEMM_K256W8; pl.block = 512; pl.lds = RING2_BYTES;
    }
    return pl;
}
#undef GEMM_PLAN_REQUIRE
