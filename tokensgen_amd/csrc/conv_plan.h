// Which kernel tg_conv3d_cl (vae.hip) launches for a shape, and with what grid, block and LDS: ONE pure host function.  No HIP, no globals, no knob or
// device reads: the launcher passes the live knobs and CU count in, a CPU test (tests/csrc/conv_plan_table.cpp) passes its own.
#pragma once
#include <stdio.h>

#include "tg_errors.h"

// ---- tile and LDS sizes that the kernels of vae.hip and their launches share ----
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int GN_GROUPS = 32;
constexpr int TILE_BYTES = BM * BK * 2;
constexpr int STAGE_BYTES = 2 * TILE_BYTES;

// conv3d_halo2_kernel / conv3d_halo_narrow_kernel / conv3d_in_kernel: a 16 x 32 patch of one output frame per workgroup
constexpr int H2_PH = 16, H2_PW = 32, H2_LW = H2_PW + 2, H2_ROWS = (H2_PH + 2) * H2_LW;      // 612 halo voxels
constexpr int H2_STRIDE = 80;
constexpr int H2_HALO_PIECES = (H2_ROWS * H2_STRIDE + 1023) / 1024;                            // 48
constexpr int H2_HALO_BYTES = H2_HALO_PIECES * 1024;                                           // 49152
constexpr int H2_W_BYTES = 128 * 64;                  // ring slot: 128 output channels x 32 k, 64-byte rows (16-byte slots XOR-swizzled by (row >> 2) & 3): 8 pieces, 2 per wave
constexpr int H2_RING = 4;                            // weight stages in flight: the DMA of stage s+3 is issued at the top of stage s
constexpr int H2_LDS = 2 * H2_HALO_BYTES + H2_RING * H2_W_BYTES;                               // 131072
constexpr int HN_WROW = 27 * 128 * 2 + 64;            // conv3d_halo_narrow_kernel<128, 3>: one resident weight row (its WROW); cout real rows + one zero row, cout <= 4

constexpr int CI_WROW = 208;                                   // LDS stride of a weight row: 96 k x 2 B + 16
constexpr int CI_HALO = 3 * H2_ROWS * 16;                      // three frames x 612 voxels x 8 channels
constexpr int CI_LDS = CI_HALO + 128 * CI_WROW;

constexpr int CW_OPER = 256 * 64 * 2;            // 32 KiB per operand per stage
constexpr int CW_STAGE = 2 * CW_OPER;            // 64 KiB
constexpr int CW_LDS = 2 * CW_STAGE;             // 128 KiB
constexpr int CW_LDS_N128 = 2 * (512 * 128 + 128 * 128);   // conv3d_w4_kernel<128>: 80 KiB per stage, all 160 KiB of LDS

struct ConvShape {
    int T, H, W, Cin, cout, cout_pad, kt, kh, kw, stride, pad, up, To, Ho, Wo;
    bool t_map, residual, gn_partial;          // whether the optional arguments are present
};

// TG_CONV_HALO and TG_CONV_W4: 0 never, 1 (default) at launch scale, 2 whenever legal (cross-check tests, tg_debug_set).  TG_CONV_SPLITK: 0 disables split-K
// (A/B runs, and the bitwise 4-wave-vs-128 test)
struct ConvKnobs { int halo, w4, splitk; };

enum ConvKernel {      // the values are tg_conv3d_kernel()'s answers (include/tokensgen_hip.h)
    CONV_IN8,           // conv3d_in_kernel: the encoder's conv_in, 8-channel input
    CONV_HALO_NARROW,   // conv3d_halo_narrow_kernel<128, 3>: the decoder's conv_out
    CONV_N16,           // conv3d_cl_kernel<1, 2, 1>: 128 voxels x 16 channels
    CONV_HALO2,         // conv3d_halo2_kernel<8>
    CONV_W4_256,        // conv3d_w4_kernel<256>
    CONV_W4_128,        // conv3d_w4_kernel<128>
    CONV_128,           // conv3d_cl_kernel<2, 4, 4>
    CONV_128_SPLITK,    // conv3d_cl_kernel<2, 4, 4> over ksplit K ranges, then conv_splitk_reduce_kernel
};

struct ConvPlan {
    int err;                       // TG_OK, or the code of a refused shape with its text in msg
    char msg[256];
    ConvKernel kernel;
    unsigned grid;
    int block, lds;                // lds: dynamic LDS bytes of the launch
    int ksplit;                    // 1 unless CONV_128_SPLITK
    unsigned rgrid_x, rgrid_y;     // CONV_128_SPLITK: grid of conv_splitk_reduce_kernel<reduce_ks> ...
    int reduce_ks;                 // ... and its template case: ksplit if that is 2, 4 or 8, else 0 (the generic loop)
};

// the 32-bit-offset guard of the halo-tiled and w4 kernels: the input, two more frames (the cache) included, must be addressable with 32-bit offsets
inline bool conv_offsets_fit32(int T, int H, int W, int Cin) { return (long)(T + 2) * H * W * Cin < (1L << 31); }

// K ranges per tile for the 128 x 128 kernel (1: no split-K): only when the plain launch would leave most CUs idle (fewer tiles than CUs) and the reduction
// is long; aims at ~2 workgroups per CU (the kernel waits on every stage: a second resident workgroup hides that), >= 8 K steps per range.
inline long conv_tiles128(long M, int cout_pad) { return ((M + BM - 1) / BM) * (cout_pad / BN); }    // tiles of the 128 x 128 kernel
inline int conv_ksplit(long M, int cout, int cout_pad, long nk, int splitk_knob, int n_cu) {
    if (!splitk_knob || cout != cout_pad || cout_pad % BN != 0 || cout > 512 || nk < 32) return 1;
    const long tiles = conv_tiles128(M, cout_pad);
    if (tiles < 1 || tiles >= n_cu) return 1;
    long ks = (2L * n_cu) / tiles;            // FLOOR: tiles * ks must not exceed the 2 n_cu resident slots — the first version rounded up, and the most common
    if (ks > 8) ks = 8;                       // shape (88 tiles: 2 x 30 x 45 latent voxels x 512 channels) ran 528 workgroups = one full round + 16 stragglers
    if (ks > nk / 8) ks = nk / 8;
    return ks < 2 ? 1 : (int)ks;
}

#define CONV_PLAN_REQUIRE(cond, ...)                         \
    do {                                                     \
        if (!(cond)) {                                       \
            pl.err = TG_ERR_SHAPE;                           \
            snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__);   \
            return pl;                                       \
        }                                                    \
    } while (0)

inline ConvPlan conv_plan(const ConvShape& s, const ConvKnobs& knobs, int n_cu) {
    ConvPlan pl{};
    pl.ksplit = 1;
    auto launch = [&pl](ConvKernel kernel, long grid, int block, int lds) {
        pl.kernel = kernel; pl.grid = (unsigned)grid; pl.block = block; pl.lds = lds;
        return pl;
    };
    const int T = s.T, H = s.H, W = s.W, Cin = s.Cin, cout = s.cout, cout_pad = s.cout_pad, kt = s.kt, kh = s.kh, kw = s.kw, stride = s.stride, pad = s.pad,
              up = s.up, To = s.To, Ho = s.Ho, Wo = s.Wo;
    CONV_PLAN_REQUIRE(T > 0 && H > 0 && W > 0 && To > 0 && Ho > 0 && Wo > 0, "tg_conv3d_cl: bad spatial shape");
    const long M = (long)To * Ho * Wo, rows128 = (M + BM - 1) / BM;
    const long h2tiles = (long)To * ((Ho + H2_PH - 1) / H2_PH) * ((Wo + H2_PW - 1) / H2_PW);    // 16 x 32 patches: the grid of the halo-tiled kernels
    const bool same_dims = To == T && Ho == H && Wo == W;
    const bool off32 = conv_offsets_fit32(T, H, W, Cin);
    if (Cin == 8) {                    // the encoder's conv_in: 8-channel input (3 used), weights packed [128][96] with k = tap * 3 + channel
        CONV_PLAN_REQUIRE(cout == 128 && cout_pad == 128 && kt == 3 && kh == 3 && kw == 3 && stride == 1 && pad == 1 && up == 1 && !s.t_map && !s.residual && same_dims,
                          "tg_conv3d_cl: Cin = 8 is the 3x3x3, stride-1, 128-output-channel input convolution only");
        CONV_PLAN_REQUIRE(h2tiles < (1L << 31) && off32, "tg_conv3d_cl: too many tiles");
        // (cannot fail, like the same limit of the halo kernel below: a 16 x 32 patch is 512 voxels, so rows128 <= 4 h2tiles for every shape.  Kept as the
        // statement of what the epilogue's GroupNorm rows rely on; no test case can reach it)
        CONV_PLAN_REQUIRE(!s.gn_partial || rows128 <= 4 * h2tiles, "tg_conv3d_cl: GroupNorm sums need <= 4 rows of 128 voxels per 16 x 32 patch");
        // every patch writes gn_partial[patch * 64 ..]: the buffer (tg_conv3d_gn_partial_floats) has one row per 128 voxels, so there may not be more patches than rows
        CONV_PLAN_REQUIRE(!s.gn_partial || h2tiles <= rows128, "tg_conv3d_cl: GroupNorm sums need at least as many 128-voxel rows (%ld) as 16 x 32 patches (%ld)",
                          rows128, h2tiles);
        return launch(CONV_IN8, h2tiles, 512, CI_LDS);
    }
    CONV_PLAN_REQUIRE(Cin % BK == 0 && (cout_pad % BN == 0 || (cout_pad < BN && cout_pad % 16 == 0)) && cout > 0 && cout <= cout_pad,
                      "tg_conv3d_cl: need Cin%%64==0 and cout_pad%%128==0 (or cout_pad in {16, 32, ..., 112}) (Cin=%d cout=%d cout_pad=%d)", Cin, cout, cout_pad);
    CONV_PLAN_REQUIRE(kt >= 1 && kt <= 3 && kh >= 1 && kh <= 3 && kw >= 1 && kw <= 3 && (stride == 1 || stride == 2) && (up == 1 || up == 2) && pad >= 0 && pad <= 1,
                      "tg_conv3d_cl: unsupported kernel/stride/pad/up");
    // BN % (cout / 32): every epilogue gives a 128-channel tile BN / (cout / 32) whole groups.  cout = 384 (12 channels per group: 10.67 groups per tile) passed the
    // first two conditions alone and got sums that missed the channels of every group straddling a tile
    CONV_PLAN_REQUIRE(!s.gn_partial || (cout == cout_pad && cout % BN == 0 && (cout / GN_GROUPS) % 4 == 0 && BN % (cout / GN_GROUPS) == 0),
                      "tg_conv3d_cl: fused GroupNorm sums need cout in {128, 256, 512, ...} (cout=%d)", cout);
    const long nk = (long)kt * kh * kw * (Cin / BK);    // K steps of 64
    const bool halo_scale = knobs.halo == 2 || h2tiles >= n_cu;
    if (cout_pad % BN != 0) {
        // the decoder's conv_out: halo-tiled, weights resident in LDS (17.7 -> 3 ms per decode against the 128 x 16 GEMM-shaped tile below)
        if (knobs.halo && cout <= 4 && Cin == 128 && kt == 3 && kh == 3 && kw == 3 && pad == 1 && stride == 1 && up == 1 && !s.t_map && !s.residual && same_dims &&
            off32 && halo_scale && h2tiles < (1L << 31))
            return launch(CONV_HALO_NARROW, h2tiles, 512, 2 * H2_HALO_BYTES + (cout + 1) * HN_WROW);
        // narrow output (conv_out): 128 voxels x 16 channels per workgroup
        const long tiles16 = rows128 * (cout_pad / 16);
        CONV_PLAN_REQUIRE(tiles16 < (1L << 31), "tg_conv3d_cl: too many tiles");
        return launch(CONV_N16, tiles16, 256, 2 * STAGE_BYTES);
    }
    const long tiles = conv_tiles128(M, cout_pad);
    CONV_PLAN_REQUIRE(tiles < (1L << 31), "tg_conv3d_cl: too many tiles");
    // Cout = 128, 3x3 spatial taps, stride 1, no upsampling: the halo-tiled kernel.  Against the GEMM-shaped kernels on the 8 x 240 x 360 layers:
    // 128 -> 128: 0.70 vs 0.74 ms per launch; per clip 64 -> 128 (encoder conv_in) 13.3 vs 17.5 ms, 256 -> 128 45.6 vs 51.2 ms.  Why not more:
    // see the stage loop's comment (the fill does not overlap with the issuing wave's MFMAs).
    // Cout = 256 (two 128-channel slabs per patch) is legal but measured SLOWER than the 256 x 256 GEMM-shaped kernel (0.66 vs 0.55 ms on 256 -> 256 at
    // 8 x 120 x 180: each slab re-stages the halo and the weights dominate the fill either way): taken only when forced (TG_CONV_HALO=2, tests).
    // 8 waves (two per SIMD): 0.716 vs 0.730 ms (128 -> 128 at 8 x 240 x 360), 1.19 vs 1.26 ms (256 -> 128) against the one-wave-per-SIMD form of
    // the same kernel, same box (profiles/NOTES.md, round 4)
    if (knobs.halo && (cout == 128 || (cout == 256 && knobs.halo == 2)) && cout_pad == cout && kh == 3 && kw == 3 && pad == 1 && stride == 1 && up == 1 && !s.t_map &&
        (kt == 1 || kt == 3) && same_dims && halo_scale && h2tiles <= rows128 && rows128 <= 4 * h2tiles && off32 && h2tiles < (1L << 31))
        return launch(CONV_HALO2, h2tiles * (cout / 128), 512, H2_LDS);
    // 4-wave kernel: 256x256 tiles.  Its launch threshold was "at least 2 tiles per CU" (set from single-stream timings in round 2: a launch of 270 tiles pays
    // two rounds for 1.05); under the three tile streams a partial round is filled by the other tiles' launches, and what counts is the fill-path bytes per
    // flop — half of the 128 x 128 kernel's.  Swept in round 4 (decode / encode wall, same box): 2 n_cu 0.469 / 0.246 s, n_cu 0.461 / 0.233, n_cu/2 0.446 / 0.228,
    // n_cu/5 0.441 / 0.226, n_cu/8 0.436 / 0.220, n_cu/12 0.451 / 0.224 (there the 512-channel layers at 30 x 45 — 22 tiles — leave split-K).
    // TG_CONV_W4 governs both w4 kernels; w4_ok: the range conditions they share
    const bool w4_ok = knobs.w4 && !s.t_map && nk >= 4 && H * up < 2048 && W * up < 2048 && To < 512 && Ho < 2048 && Wo < 2048 &&
                       (long)kt * kh * kw * Cin < (1L << 21) && off32;
    const long tiles256 = ((M + 255) / 256) * (cout / 256), tiles512 = (M + 511) / 512;
    if (w4_ok && (knobs.w4 == 2 || tiles256 >= n_cu / 8) && cout == cout_pad && cout % 256 == 0 && M >= 1024)
        return launch(CONV_W4_256, tiles256, 256, CW_LDS);
    // Cout = 128: the 512x128 variant ("plain" convolutions only — stride 1, no upsampling, whatever the taps: 3x3x3, 1x3x3, and the 1x1x1, pad 0 shortcut of the
    // decoder's last 256 -> 128 block, nk = 4, which takes this branch at full size; 16 A pieces per wave are too many for the general address path)
    // (TG_CONV_W4 governs this variant too; measured: 128->128 layers 203 -> 187 ms per decode, 181 -> 162 ms per encode)
    if (w4_ok && (knobs.w4 == 2 || tiles512 >= 2L * n_cu) && cout == 128 && cout_pad == 128 && stride == 1 && up == 1 && M >= 2048)
        return launch(CONV_W4_128, tiles512, 256, CW_LDS_N128);
    // split-K: the small-M layers (the 512-channel layers at 30 x 45 latent: 88 tiles for 256 CUs, each walking 216 K steps alone on its CU).
    // The w4 kernels are chosen first where they apply.
    pl.ksplit = conv_ksplit(M, cout, cout_pad, nk, knobs.splitk, n_cu);
    if (pl.ksplit > 1) {
        pl.rgrid_x = (unsigned)rows128; pl.rgrid_y = (unsigned)(cout / 128);
        pl.reduce_ks = pl.ksplit == 2 || pl.ksplit == 4 || pl.ksplit == 8 ? pl.ksplit : 0;
        return launch(CONV_128_SPLITK, tiles * pl.ksplit, 256, 2 * STAGE_BYTES);
    }
    return launch(CONV_128, tiles, 256, 2 * STAGE_BYTES);
}
#undef CONV_PLAN_REQUIRE

// Floats of split-K workspace the caller must hand to tg_conv3d_cl for this shape (0: none).  The 128 x 128 kernel's size whether or not a halo or w4 form
// would be taken first (= the plan with both knobs at 0): callers cache the value per shape and the cross-check tests flip those two knobs afterwards.
inline long conv_splitk_floats(int Cin, int cout, int cout_pad, int kt, int kh, int kw, int To, int Ho, int Wo, int splitk_knob, int n_cu) {
    const long M = (long)To * Ho * Wo;
    const int ks = conv_ksplit(M, cout, cout_pad, (long)kt * kh * kw * (Cin / BK), splitk_knob, n_cu);
    return ks > 1 ? (long)ks * M * cout_pad : 0;
}

// nearest x2 upsampling + 3x3 convolution as four 2x2 phase convolutions on the LOW-resolution input (tg_conv3d_up2_subpixel): is the shape in the
// 256 x 256 kernel's range and at its launch scale (the four phases are one launch: 4 x the tiles against the w4 threshold above)
inline bool up2_subpixel_shape_ok(int T, int H, int W, int Cin, int cout, int n_cu) {
    const long M = (long)T * H * W;
    return Cin % 64 == 0 && cout % 256 == 0 && M >= 1024 && 4 * ((M + 255) / 256) * (cout / 256) >= n_cu / 8 && 4L * (Cin / 64) >= 4 && H < 1024 && W < 1024 && T < 512 &&
           4L * Cin < (1L << 21) && conv_offsets_fit32(T, H, W, Cin) && 4L * M * cout < (1L << 40);
}
