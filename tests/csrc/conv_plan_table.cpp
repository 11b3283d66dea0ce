// Prints what conv_plan() (tokensgen_amd/csrc/conv_plan.h) decides for a table of shapes, one line per case: host only, no GPU.
// tests/test_host_cpu.py::test_conv_plan_table holds the expected lines.  Every case: 256 CUs, kernel kt x 3 x 3, stride 1, pad 1, up 1, output dims = input dims.
#include <stdio.h>

#include "conv_plan.h"

namespace {

constexpr int N_CU = 256;
const char* const kKernelName[] = {"in8", "halo_narrow", "n16", "halo2", "w4_256", "w4_128", "k128", "k128_splitk"};

struct Opt { int halo = 1, w4 = 1, splitk = 1, kt = 3; bool gn = false; };

void conv(const char* name, int Cin, int cout, int cout_pad, int T, int H, int W, Opt o = {}) {
    const ConvShape s{T, H, W, Cin, cout, cout_pad, o.kt, 3, 3, 1, 1, 1, T, H, W, false, false, o.gn};
    const ConvPlan pl = conv_plan(s, ConvKnobs{o.halo, o.w4, o.splitk}, N_CU);
    if (pl.err != TG_OK) {
        printf("%s: error %d: %s\n", name, pl.err, pl.msg);
        return;
    }
    printf("%s: %s grid %u block %d lds %d ksplit %d reduce %ux%u case %d splitk_floats %ld\n", name, kKernelName[pl.kernel], pl.grid, pl.block, pl.lds, pl.ksplit,
           pl.rgrid_x, pl.rgrid_y, pl.reduce_ks, conv_splitk_floats(Cin, cout, cout_pad, o.kt, 3, 3, T, H, W, o.splitk, N_CU));
}

void up2(const char* name, int T, int H, int W, int Cin, int cout) { printf("%s: up2_subpixel_shape_ok %d\n", name, (int)up2_subpixel_shape_ok(T, H, W, Cin, cout, N_CU)); }

Opt halo(int v) { Opt o; o.halo = v; return o; }
Opt w4(int v) { Opt o; o.w4 = v; return o; }

}  // namespace

int main() {
    // the layers of the real workload
    conv("conv_in 8->128 8x240x360", 8, 128, 128, 8, 240, 360);
    conv("conv_out 128->3 8x240x360", 128, 3, 16, 8, 240, 360);
    conv("conv_out 128->3 2x32x32", 128, 3, 16, 2, 32, 32);
    conv("128->128 8x240x360", 128, 128, 128, 8, 240, 360);
    conv("128->128 8x240x360 halo=0", 128, 128, 128, 8, 240, 360, halo(0));
    conv("256->256 8x120x180", 256, 256, 256, 8, 120, 180);
    conv("512->512 2x30x45", 512, 512, 512, 2, 30, 45);
    conv("128->128 2x32x32", 128, 128, 128, 2, 32, 32);
    { Opt o; o.splitk = 0; conv("128->128 2x32x32 splitk=0", 128, 128, 128, 2, 32, 32, o); }
    // halo tiles at n_cu - 1 and n_cu (both with rows128 == 4 x halo tiles, the most that limit allows: a 16 x 32 patch is four rows of 128 voxels)
    conv("128->128 1x240x544 (255 patches)", 128, 128, 128, 1, 240, 544);
    conv("128->128 1x256x512 (256 patches)", 128, 128, 128, 1, 256, 512);
    conv("conv_out 128->3 1x240x544 (255 patches)", 128, 3, 16, 1, 240, 544);
    conv("conv_out 128->3 1x256x512 (256 patches)", 128, 3, 16, 1, 256, 512);
    // more patches than 128-voxel rows: never the halo kernel
    conv("128->128 256x1x1 (256 patches, 2 rows)", 128, 128, 128, 256, 1, 1);
    // w4 256-wide tiles at n_cu / 8 - 1 and n_cu / 8
    conv("256->256 1x62x128 (31 tiles)", 256, 256, 256, 1, 62, 128);
    conv("256->256 1x64x128 (32 tiles)", 256, 256, 256, 1, 64, 128);
    // M at 1023 and 1024 (2048 output channels: 32 tiles of 256 x 256 either way)
    conv("128->2048 1x33x31 (M 1023)", 128, 2048, 2048, 1, 33, 31);
    conv("128->2048 1x32x32 (M 1024)", 128, 2048, 2048, 1, 32, 32);
    // M at 2047 and 2048 (below the w4 128-wide launch scale: forced with the knob)
    conv("128->128 1x23x89 (M 2047) w4=2", 128, 128, 128, 1, 23, 89, w4(2));
    conv("128->128 1x32x64 (M 2048) w4=2", 128, 128, 128, 1, 32, 64, w4(2));
    // split-K: 128 x 128 tiles at n_cu - 1 and n_cu
    conv("128->128 1x120x272 (255 tiles)", 128, 128, 128, 1, 120, 272);
    conv("128->128 1x128x256 (256 tiles)", 128, 128, 128, 1, 128, 256);
    // the knobs at 2, below launch scale
    conv("128->128 2x32x32 halo=2", 128, 128, 128, 2, 32, 32, halo(2));
    conv("256->256 2x32x32 halo=2", 256, 256, 256, 2, 32, 32, halo(2));
    conv("conv_out 128->3 2x32x32 halo=2", 128, 3, 16, 2, 32, 32, halo(2));
    conv("256->256 1x32x32", 256, 256, 256, 1, 32, 32);
    conv("256->256 1x32x32 w4=2", 256, 256, 256, 1, 32, 32, w4(2));
    // one refused shape per message.  ("GroupNorm sums need <= 4 rows of 128 voxels per 16 x 32 patch" cannot be reached: see conv_plan.h)
    conv("refused: T = 0", 128, 128, 128, 0, 32, 32);
    conv("refused: 8->64", 8, 64, 128, 2, 32, 32);
    conv("refused: 8->128 100x2048x2048", 8, 128, 128, 100, 2048, 2048);
    { Opt o; o.gn = true; conv("refused: 8->128 2x1x1 with GroupNorm sums", 8, 128, 128, 2, 1, 1, o); }
    conv("refused: Cin 100", 100, 128, 128, 2, 32, 32);
    { Opt o; o.kt = 4; conv("refused: kt 4", 128, 128, 128, 2, 32, 32, o); }
    { Opt o; o.gn = true; conv("refused: 128->3 with GroupNorm sums", 128, 3, 16, 2, 32, 32, o); }
    conv("refused: 128->7 (cout_pad 112) 4096x4096x4096", 128, 7, 112, 4096, 4096, 4096);
    conv("refused: 128->1024 4096x4096x4096", 128, 1024, 1024, 4096, 4096, 4096);
    // tg_conv3d_up2_subpixel: one shape that qualifies, then M at 1023 / 1024 and the four phases' tiles at n_cu / 8 - 4 / n_cu / 8
    up2("up2 256->256 8x120x180", 8, 120, 180, 256, 256);
    up2("up2 256->512 1x33x31 (M 1023)", 1, 33, 31, 256, 512);
    up2("up2 256->512 1x32x32 (M 1024)", 1, 32, 32, 256, 512);
    up2("up2 256->256 1x28x64 (4 x 7 tiles)", 1, 28, 64, 256, 256);
    up2("up2 256->256 1x29x64 (4 x 8 tiles)", 1, 29, 64, 256, 256);
    return 0;
}
