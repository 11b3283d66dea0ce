// What the JPEG encoder (jpeg.hip) and decoder (jpeg_decode.hip) share: the literal DCT table, the zigzag order and the MCU geometry of a frame.
#pragma once
#include <stdint.h>

namespace {

// A[u][x] = rint(8192 / 2 c_u cos((2 x + 1) u pi / 16))
constexpr int DCT_A[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017}, {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
    {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},   {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// natural index of zigzag position k, and its inverse
constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct Unzig { uint8_t at[64]; };
constexpr Unzig make_unzig() {
    Unzig u{};
    for (int k = 0; k < 64; ++k) u.at[ZIGZAG[k]] = (uint8_t)k;
    return u;
}
constexpr Unzig UNZIG = make_unzig();

struct Geometry { int mcu, bpm, rows, cols; long n_mcu; };
inline bool geometry(int H, int W, int subsampling, Geometry& g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (subsampling != 420 && subsampling != 444)) return false;
    g.mcu = subsampling == 420 ? 16 : 8;
    g.bpm = subsampling == 420 ? 6 : 3;
    g.rows = (H + g.mcu - 1) / g.mcu;
    g.cols = (W + g.mcu - 1) / g.mcu;
    g.n_mcu = (long)g.rows * g.cols;
    return true;
}

}  // namespace
