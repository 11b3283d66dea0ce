// Motion-compensated interpolation of in-between frames, in integers: the consumer of tg_block_motion's vectors.
//   tg_mci_select: per pair, phase k = 1 .. n - 1 and block of the in-between frame the best of at most 19 candidate vectors ((0, 0), the 3 x 3 neighbourhood of the
//                  forward field, the negated 3 x 3 neighbourhood of the backward field) by the bilateral SAD of the two luma blocks the vector joins.  Both blocks of
//                  a candidate move with it, so there is no sliding window: a lane assembles four bytes of each block and takes v_sad_u8.  BLK = 16: the 64 lanes
//                  of a wave hold one candidate's 256 pixels; BLK = 8: 16 lanes hold a candidate and the wave takes four at a time.  The tuple (bisad, dy^2 + dx^2,
//                  dy, dx) packs into the 64-bit key of the search and the winner is an unsigned minimum by shuffles: no atomics, no workspace, no order.
//   tg_mci_render: overlapped block compensation.  A pixel blends the predictions of the (up to) four blocks whose centres surround it, each prediction the
//                  (n - k) : k mix of the previous frame at (y, x) - a and the next frame at (y, x) - a + v, coordinates clamped to the frame.  A workgroup of four
//                  waves owns 16 rows x 64 pixels, a wave a 16 x 16 tile whose origin is (-8, -8) plus multiples of 16, a lane four neighbouring pixels of a row.
//                  BLK = 16: the blocks that weigh in change every 16 pixels from 8 on, which is where the tiles start, so the four vectors, their roundings and
//                  block indices are the same for the whole wave, computed from the tile origin; BLK = 8: they change at 4 + 8 m, never inside a lane's four
//                  pixels, and are per lane.  With interleaved RGB and no clamped column a lane's four source pixels are 12 neighbouring bytes of any alignment:
//                  one 12-byte load per source (8 per lane) and one 12-byte store, 48 contiguous bytes per tile row; otherwise (planar input, frame borders,
//                  the last columns) bytes.  The division by D = n 4 BLK^2 is a shift and one multiplication by a host-made reciprocal.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int MCI_NMAX = 8;
constexpr int MCI_VMAX = 32;                    // a field component beyond the largest search radius is never admitted: the key holds 12 bits of dy^2 + dx^2

struct RgbSrc { const uint8_t* p; long so, si, sr, sp, sc; };                   // byte strides: outer index, inner index, row, pixel, channel

// (2 k d + n) // (2 n) with floor division: k d / n rounded, halves toward +inf
__device__ __forceinline__ int rnd_kdn(int k, int d, int n) {
    const int num = 2 * k * d + n, den = 2 * n;
    return num >= 0 ? num / den : -((-num + den - 1) / den);
}

// four neighbouring bytes of any alignment as one dword (the compiler picks the load: one dword where the target reads unaligned, which gfx950 does)
__device__ __forceinline__ uint32_t bytes4(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// prev, next: packed luma planes, `pitch` bytes per row.  One wave per (pair, phase, block), four per workgroup.
template <int BLK>
__global__ __launch_bounds__(256) void mci_select_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ next, long prev_so, long prev_si, long next_so,
                                                         long next_si, const int16_t* __restrict__ fwd, const int16_t* __restrict__ bwd, int n_inner, int H, int W,
                                                         int pitch, int n, int Hb, int Wb, long items, int16_t* __restrict__ mvi, int32_t* __restrict__ cost) {
    constexpr int BD = BLK / 4;                 // dwords per block row
    constexpr int LPC = BLK * BD;               // lanes per candidate: 64 or 16
    constexpr int GROUPS = 64 / LPC;            // candidates per pass: 1 or 4
    const long o = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= items) return;                     // wave-uniform
    const int lane = threadIdx.x & 63, sub = lane % LPC, grp = lane / LPC;
    const int row = sub / BD, col = (sub % BD) * 4;
    const int bx = (int)(o % Wb);
    long t = o / Wb;
    const int by = (int)(t % Hb);
    t /= Hb;
    const int k = (int)(t % (n - 1)) + 1;
    const long pair = t / (n - 1), po = pair / n_inner, pi = pair - po * n_inner;
    const uint8_t* pp = prev + po * prev_so + pi * prev_si;
    const uint8_t* np = next + po * next_so + pi * next_si;
    const long field0 = pair * Hb * Wb;
    const int ncand = bwd ? 19 : 10;

    // lane c < ncand fetches candidate c once; the passes below read it from that lane, so that no pass waits for a field before it can address its blocks
    int cdy = 0, cdx = 0;
    if (lane > 0 && lane < ncand) {
        const int j = (lane - 1) % 9;
        const int y = min(max(by + j / 3 - 1, 0), Hb - 1), x = min(max(bx + j % 3 - 1, 0), Wb - 1);
        const int16_t* f = (lane <= 9 ? fwd : bwd) + 2 * (field0 + (long)y * Wb + x);
        cdy = lane <= 9 ? f[0] : -(int)f[0];
        cdx = lane <= 9 ? f[1] : -(int)f[1];
    }
    unsigned long long best = ~0ull;
    for (int c0 = 0; c0 < ncand; c0 += GROUPS) {                                // the same trip count for every lane: the shuffles below are never divergent
        const int ci = c0 + grp;
        bool ok = ci < ncand;
        int dy = __shfl(cdy, ok ? ci : 0, 64), dx = __shfl(cdx, ok ? ci : 0, 64);
        ok = ok && dy >= -MCI_VMAX && dy <= MCI_VMAX && dx >= -MCI_VMAX && dx <= MCI_VMAX;
        if (!ok) dy = dx = 0;
        const int py = by * BLK - rnd_kdn(k, dy, n), px = bx * BLK - rnd_kdn(k, dx, n);
        const int qy = py + dy, qx = px + dx;
        ok = ok && py >= 0 && py + BLK <= H && px >= 0 && px + BLK <= W && qy >= 0 && qy + BLK <= H && qx >= 0 && qx + BLK <= W;
        uint32_t s = 0;
        if (ok)                                                                 // both blocks inside the frame: rows py + row < H, bytes px + col + 3 < W <= pitch
            s = __builtin_amdgcn_sad_u8(bytes4(pp + (long)(py + row) * pitch + px + col), bytes4(np + (long)(qy + row) * pitch + qx + col), 0u);
#pragma unroll
        for (int off = LPC / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);           // stays inside the candidate's LPC lanes
        const unsigned long long key = ((unsigned long long)s << 26) | ((unsigned long long)(dy * dy + dx * dx) << 14) | ((unsigned long long)(dy + 64) << 7) |
                                       (unsigned long long)(dx + 64);
        if (ok && key < best) best = key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)best, off, 64), hi = __shfl_xor((uint32_t)(best >> 32), off, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other < best ? other : best;
    }
    if (lane == 0) {                                                            // (0, 0) is always admitted: never ~0
        mvi[2 * o] = (int16_t)((int)((best >> 7) & 127) - 64);
        mvi[2 * o + 1] = (int16_t)((int)(best & 127) - 64);
        cost[o] = (int32_t)(best >> 26);
    }
}

// the two blocks along one axis that weigh in on pixel coordinate y, and the second one's weight f (the first weighs 2 BLK - f)
template <int BLK>
__device__ __forceinline__ void taps(int y, int nb, int& r_lo, int& r_hi) {
    const int r0 = (2 * y + 1 + BLK) / (2 * BLK) - 1;                          // floor((2 y + 1 - BLK) / (2 BLK)), >= -1
    r_lo = min(max(r0, 0), nb - 1);
    r_hi = min(max(r0 + 1, 0), nb - 1);
}
template <int BLK>
__device__ __forceinline__ int tap_weight(int y) {
    const int c = 2 * y + 1 + BLK;                                              // c + 2 BLK > 0
    return c - (c / (2 * BLK)) * (2 * BLK);                                     // f, odd, in [1, 2 BLK - 1]
}

template <int BLK>
__global__ __launch_bounds__(256) void mci_render_kernel(RgbSrc A, RgbSrc B, const int16_t* __restrict__ mvi, int n_inner, int H, int W, int n, int recip, int Hb, int Wb,
                                                         int tiles_x, int tiles_y, uint8_t* __restrict__ dst, long dst_so, long dst_sf) {
    constexpr int SHIFT = BLK == 16 ? 10 : 8;                                   // 4 BLK^2
    long blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x);
    blk /= tiles_x;
    const int ty = (int)(blk % tiles_y);
    blk /= tiles_y;
    const int k = (int)(blk % (n - 1)) + 1;
    const long pair = blk / (n - 1), po = pair / n_inner, pi = pair - po * n_inner;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int y0 = ty * 16 - 8, x0 = tx * 64 + wave * 16 - 8;                   // the tile: 16 x 16 pixels from (y0, x0), where the weights' blocks change
    const int y = y0 + (lane >> 2), x = x0 + (lane & 3) * 4;                    // the lane: pixels x .. x + 3 of row y (x is a multiple of 4: all four left of 0 or none)
    if (y < 0 || y >= H || x < 0 || x >= W) return;
    const int cnt = min(4, W - x);
    // BLK = 16: every pixel of the tile has the blocks of the tile's origin (wave-uniform); BLK = 8: the blocks change at 4 + 8 m, never inside a lane's four pixels
    int rr[2], cc[2];
    taps<BLK>(BLK == 16 ? y0 : y, Hb, rr[0], rr[1]);
    taps<BLK>(BLK == 16 ? x0 : x, Wb, cc[0], cc[1]);
    const int fy = tap_weight<BLK>(y);
    const int wy[2] = {2 * BLK - fy, fy};
    int wx[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        wx[1][q] = tap_weight<BLK>(x + q);
        wx[0][q] = 2 * BLK - wx[1][q];
    }
    const uint8_t* a = A.p + po * A.so + pi * A.si;
    const uint8_t* b = B.p + po * B.so + pi * B.si;
    const int16_t* mv = mvi + 2 * ((pair * (n - 1) + (k - 1)) * Hb * Wb);
    const bool packed = A.sp == 3 && A.sc == 1 && B.sp == 3 && B.sc == 1;       // interleaved RGB: a lane's four source pixels are 12 neighbouring bytes
    int acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int16_t* v = mv + 2 * ((long)rr[i] * Wb + cc[j]);             // 0 <= rr < Hb, 0 <= cc < Wb
            const int dy = v[0], dx = v[1];
            const int sy = y - rnd_kdn(k, dy, n), sx = x - rnd_kdn(k, dx, n);
            const long tx2 = (long)sx + dx;
            const uint8_t* prow = a + (long)min(max(sy, 0), H - 1) * A.sr;      // rows and columns clamped: inside the frame whatever v
            const uint8_t* qrow = b + (long)min(max(sy + dy, 0), H - 1) * B.sr;
            uint32_t pb[3] = {0, 0, 0}, qb[3] = {0, 0, 0};                          // the four pixels' 12 bytes, packed
            if (packed && sx >= 0 && sx + 3 < W && tx2 >= 0 && tx2 + 3 < W) {   // no column is clamped: bytes 3 sx .. 3 sx + 11 of the row, of any alignment
                __builtin_memcpy(pb, prow + 3 * (long)sx, 12);
                __builtin_memcpy(qb, qrow + 3 * tx2, 12);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint8_t* p = prow + (long)min(max(sx + q, 0), W - 1) * A.sp;
                    const uint8_t* r = qrow + (long)min(max(sx + q + dx, 0), W - 1) * B.sp;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        pb[(3 * q + c) >> 2] |= (uint32_t)p[c * A.sc] << (8 * ((3 * q + c) & 3));
                        qb[(3 * q + c) >> 2] |= (uint32_t)r[c * B.sc] << (8 * ((3 * q + c) & 3));
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int w = wy[i] * wx[j][q];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int e = 3 * q + c;
                    acc[e] += w * ((n - k) * (int)((pb[e >> 2] >> (8 * (e & 3))) & 255u) + k * (int)((qb[e >> 2] >> (8 * (e & 3))) & 255u));
                }
            }
        }
    // frame pair * n + k of the output; 0 <= y < H, 0 <= x, x + cnt <= W
    uint8_t* d = dst + po * dst_so + (pi * n + k) * dst_sf + ((long)y * W + x) * 3;
    const int half = n << (SHIFT - 1);                                          // D / 2
    uint32_t ob[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < 12; ++e) ob[e >> 2] |= (uint32_t)((((acc[e] + half) >> SHIFT) * recip) >> 16) << (8 * (e & 3));    // t = .. >> SHIFT <= 256 n; t * recip >> 16 == t / n for t < 4096
    if (cnt == 4) {
        __builtin_memcpy(d, ob, 12);                                            // 12 bytes of any alignment
    } else {
#pragma unroll
        for (int e = 0; e < 9; ++e)
            if (e < 3 * cnt) d[e] = (uint8_t)(ob[e >> 2] >> (8 * (e & 3)));
    }
}

bool strides_ok(long so, long si, long sr, long sp, long sc) { return so >= 0 && si >= 0 && sr >= 0 && sp >= 0 && sc >= 0; }

}  // namespace

extern "C" int tg_mci_select(const void* prev, long prev_so, long prev_si, const void* next, long next_so, long next_si, const void* fwd, const void* bwd,
                             int n_outer, int n_inner, int H, int W, long pitch, int block, int n, void* mvi, void* cost, hipStream_t stream) {
    TG_REQUIRE(prev && next && fwd && mvi && cost, TG_ERR_ARG, "tg_mci_select: null pointer");
    TG_REQUIRE(block == 8 || block == 16, TG_ERR_ARG, "tg_mci_select: block must be 8 or 16 (got %d)", block);
    TG_REQUIRE(n >= 2 && n <= MCI_NMAX, TG_ERR_ARG, "tg_mci_select: n must be in 2..%d (got %d)", MCI_NMAX, n);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && H >= block && W >= block, TG_ERR_SHAPE, "tg_mci_select: bad shape n_outer=%d n_inner=%d H=%d W=%d for block %d", n_outer,
               n_inner, H, W, block);
    TG_REQUIRE(pitch >= W && pitch < (1L << 30) && prev_so >= 0 && prev_si >= 0 && next_so >= 0 && next_si >= 0, TG_ERR_SHAPE,
               "tg_mci_select: pitch must be in W..2^30 - 1, plane strides non-negative");
    TG_REQUIRE((((uintptr_t)cost) & 3) == 0 && (((uintptr_t)fwd | (uintptr_t)bwd | (uintptr_t)mvi) & 1) == 0, TG_ERR_ALIGN,
               "tg_mci_select: cost must be 4-byte aligned, fwd, bwd and mvi 2-byte");
    const int Hb = H / block, Wb = W / block;
    const long items = (long)n_outer * n_inner * (n - 1) * Hb * Wb, grid = (items + 3) / 4;
    TG_REQUIRE(grid < (1L << 31), TG_ERR_SHAPE, "tg_mci_select: too many blocks");
    if (block == 16)
        hipLaunchKernelGGL(mci_select_kernel<16>, dim3((unsigned)grid), dim3(256), 0, stream, (const uint8_t*)prev, (const uint8_t*)next, prev_so, prev_si, next_so,
                           next_si, (const int16_t*)fwd, (const int16_t*)bwd, n_inner, H, W, (int)pitch, n, Hb, Wb, items, (int16_t*)mvi, (int32_t*)cost);
    else
        hipLaunchKernelGGL(mci_select_kernel<8>, dim3((unsigned)grid), dim3(256), 0, stream, (const uint8_t*)prev, (const uint8_t*)next, prev_so, prev_si, next_so,
                           next_si, (const int16_t*)fwd, (const int16_t*)bwd, n_inner, H, W, (int)pitch, n, Hb, Wb, items, (int16_t*)mvi, (int32_t*)cost);
    TG_LAUNCH_CHECK("tg_mci_select");
    return TG_OK;
}

extern "C" int tg_mci_render(const void* prev, long a_so, long a_si, long a_sr, long a_sp, long a_sc, const void* next, long b_so, long b_si, long b_sr, long b_sp,
                             long b_sc, const void* mvi, int n_outer, int n_inner, int H, int W, int block, int n, void* out, long out_so, long out_sf,
                             hipStream_t stream) {
    TG_REQUIRE(prev && next && mvi && out, TG_ERR_ARG, "tg_mci_render: null pointer");
    TG_REQUIRE(block == 8 || block == 16, TG_ERR_ARG, "tg_mci_render: block must be 8 or 16 (got %d)", block);
    TG_REQUIRE(n >= 2 && n <= MCI_NMAX, TG_ERR_ARG, "tg_mci_render: n must be in 2..%d (got %d)", MCI_NMAX, n);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && H >= block && W >= block, TG_ERR_SHAPE, "tg_mci_render: bad shape n_outer=%d n_inner=%d H=%d W=%d for block %d", n_outer,
               n_inner, H, W, block);
    TG_REQUIRE(strides_ok(a_so, a_si, a_sr, a_sp, a_sc) && strides_ok(b_so, b_si, b_sr, b_sp, b_sc), TG_ERR_SHAPE, "tg_mci_render: negative stride");
    TG_REQUIRE((long)H * W < (1L << 31) / 3 && out_sf >= 3L * H * W && (out_so >= out_sf * ((long)n_inner * n + 1) || n_outer == 1), TG_ERR_SHAPE,
               "tg_mci_render: a frame must stay below 2^31 bytes, out_sf hold one (3 H W), out_so hold the n_inner * n + 1 frames of an item");
    TG_REQUIRE(((uintptr_t)mvi & 1) == 0, TG_ERR_ALIGN, "tg_mci_render: mvi must be 2-byte aligned");
    const int Hb = H / block, Wb = W / block, tiles_x = (W + 8 + 63) / 64, tiles_y = (H + 8 + 15) / 16;      // tiles start at (-8, -8)
    const long grid = (long)n_outer * n_inner * (n - 1) * tiles_x * tiles_y;
    TG_REQUIRE(grid < (1L << 31), TG_ERR_SHAPE, "tg_mci_render: too many tiles");
    const RgbSrc A{(const uint8_t*)prev, a_so, a_si, a_sr, a_sp, a_sc}, B{(const uint8_t*)next, b_so, b_si, b_sr, b_sp, b_sc};
    const int recip = 65535 / n + 1;
    if (block == 16)
        hipLaunchKernelGGL(mci_render_kernel<16>, dim3((unsigned)grid), dim3(256), 0, stream, A, B, (const int16_t*)mvi, n_inner, H, W, n, recip, Hb, Wb, tiles_x, tiles_y,
                           (uint8_t*)out, out_so, out_sf);
    else
        hipLaunchKernelGGL(mci_render_kernel<8>, dim3((unsigned)grid), dim3(256), 0, stream, A, B, (const int16_t*)mvi, n_inner, H, W, n, recip, Hb, Wb, tiles_x, tiles_y,
                           (uint8_t*)out, out_so, out_sf);
    TG_LAUNCH_CHECK("tg_mci_render");
    return TG_OK;
}
