// Motion between the frames of a video, in integers: exhaustive block matching on 8-bit luma and the motion-compensated squared error.
//   tg_luma_u8:        Y = (77 R + 150 G + 29 B + 128) >> 8 of strided uint8 RGB -> packed planes [n_outer * n_inner][H][pitch], pitch a multiple of 4 (pad bytes 0),
//                      four pixels per thread and one dword store.
//   tg_block_motion:   for every pair and every block x block block of the current plane (block in {8, 16}, tiled from the top left) the minimum over all
//                      (dy, dx), |dy|, |dx| <= R, whose displaced block lies wholly inside the other plane, of the tuple (sad, dy^2 + dx^2, dy, dx).
//                      A workgroup of four waves owns a strip of four neighbouring blocks.  It stages the part of the other plane the strip can reach as bytes in
//                      LDS once, block + 2R rows by 4 * block + 2R columns laid out on dword boundaries (LDS column 0 is frame column x0 - R4, R4 = R rounded up to
//                      4, so every staging load is one aligned dword; bytes outside the plane are 0 and never part of an admitted candidate).  Each wave takes one
//                      block and keeps it in registers (the address is wave-uniform: 64 dwords for 16 x 16).  A lane takes a group of 4 x 4 neighbouring
//                      candidates: 4 values of dy share block + 3 staged rows, and the 4 values of dx are the four 16-bit sums of v_qsad_pk_u16_u8, whose 8-byte
//                      window slides over two neighbouring staged dwords, so that no unaligned dword is ever assembled.  The packed sums cannot wrap: the largest
//                      cost is 16 * 16 * 255 = 65 280 < 65 536.  (v_msad_u8 / v_mqsad_* skip reference bytes equal to 0: they are not this sum.)  The tuple packs into one
//                      64-bit key, sad << 26 | distance << 14 | (dy + 64) << 7 | (dx + 64), and the winner is an unsigned minimum over the lane's candidates and then
//                      over the wave by shuffles: no atomics, no dependence on any order.
//   tg_block_warp_sse: per pair and block the sum over the block's pixels and three channels of (cur - ref displaced by the block's vector)^2 and the same at zero
//                      displacement, one wave per block, exact in int32.  A vector that leaves the frame is clamped and counted in a device status word.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int BM_STRIP = 4;                    // blocks per workgroup, one per wave
constexpr int BM_RMAX = 32;
constexpr int BM_DYN = 4;                      // values of dy per lane and pass
constexpr int BM_MAX_G = (BM_RMAX + BM_RMAX) / 4 + 1;                           // 17 groups of four dx
constexpr int BM_MAX_DG = (2 * BM_RMAX + 1 + BM_DYN - 1) / BM_DYN;              // 17 groups of four dy
constexpr int BM_MAX_ROWS = 16 + BM_DYN * BM_MAX_DG;                            // 84 staged rows
constexpr int BM_MAX_LPD = BM_STRIP * 16 / 4 + BM_MAX_G + 1;                    // 34 dwords per staged row

struct RgbSrc { const uint8_t* p; long so, si, sr, sp, sc; };                   // byte strides: outer index, inner index, row, pixel, channel

__device__ __forceinline__ uint32_t luma_u8(const uint8_t* p, long sc) {
    return (77u * p[0] + 150u * p[sc] + 29u * p[2 * sc] + 128u) >> 8;
}

__global__ __launch_bounds__(256) void luma_kernel(RgbSrc S, int n_inner, int H, int W, int pitch4, long total, uint32_t* __restrict__ dst) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c4 = (int)(idx % pitch4);
        long t = idx / pitch4;
        const int y = (int)(t % H);
        const long plane = t / H, o = plane / n_inner, i = plane - o * n_inner;
        const uint8_t* row = S.p + o * S.so + i * S.si + (long)y * S.sr;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = c4 * 4 + q;
            if (x < W) v |= luma_u8(row + (long)x * S.sp, S.sc) << (8 * q);     // 0 <= x < W, 0 <= y < H
        }
        dst[idx] = v;
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// cur, ref: packed luma planes, `pitch` bytes per row (a multiple of 4), 4-byte aligned.  Pair p = (o, i): planes cur + o * cur_so + i * cur_si and ref + ...
template <int BLK>
__global__ __launch_bounds__(256) void block_motion_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ ref, long cur_so, long cur_si, long ref_so,
                                                           long ref_si, int n_inner, int H, int W, int pitch, int R, int Hb, int Wb, int strips,
                                                           int16_t* __restrict__ mv, int32_t* __restrict__ sad_out, int32_t* __restrict__ sad0_out) {
    constexpr int BD = BLK / 4;                                                 // dwords per block row
    __shared__ uint32_t win[BM_MAX_ROWS * BM_MAX_LPD];
    const int tid = threadIdx.x;
    long blk = blockIdx.x;
    const int strip = (int)(blk % strips);
    blk /= strips;
    const int by = (int)(blk % Hb);
    const long pair = blk / Hb, po = pair / n_inner, pi = pair - po * n_inner;
    const uint8_t* cp = cur + po * cur_so + pi * cur_si;
    const uint8_t* rp = ref + po * ref_so + pi * ref_si;

    const int R4 = (R + 3) & ~3;
    const int G = (R4 + R) / 4 + 1;                                             // groups of four dx: LDS columns R4 - R .. R4 + R of a block
    const int NDG = (2 * R + 1 + BM_DYN - 1) / BM_DYN;                          // groups of four dy
    const int LPD = BM_STRIP * BD + G + 1;                                      // staged dwords per row (<= BM_MAX_LPD)
    const int rows = BLK + BM_DYN * NDG;                                        // staged rows (<= BM_MAX_ROWS); row 0 is frame row y0 - R
    const int y0 = by * BLK, x0 = strip * BM_STRIP * BLK;
    const int pitch4 = pitch >> 2;
    for (int idx = tid; idx < rows * LPD; idx += 256) {
        const int r = idx / LPD, c = idx - r * LPD;
        const int fy = y0 - R + r, fc4 = (x0 - R4) / 4 + c;                     // x0 - R4 is a multiple of 4 (possibly negative: exact division)
        uint32_t v = 0;
        if (fy >= 0 && fy < H && fc4 >= 0 && fc4 < pitch4) v = ((const uint32_t*)(rp + (long)fy * pitch))[fc4];
        win[idx] = v;
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int bx = strip * BM_STRIP + wave;
    if (bx >= Wb) return;
    const int x = bx * BLK;

    uint32_t cb[BLK][BD];                                                       // the current block: wave-uniform
#pragma unroll
    for (int i = 0; i < BLK; ++i)
#pragma unroll
        for (int k = 0; k < BD; ++k) cb[i][k] = ((const uint32_t*)(cp + (long)(y0 + i) * pitch + x))[k];     // y0 + i < H, x + 4k + 3 < W <= pitch

    unsigned long long best = ~0ull;
    for (int u = lane; u < NDG * G; u += 64) {
        const int dg = u / G, g = u - dg * G;
        const uint32_t* wp = win + (BM_DYN * dg) * LPD + wave * BD + g;         // rows 4 dg .. 4 dg + BLK + 2 < rows, dwords .. wave * BD + g + BD < LPD
        unsigned long long acc[BM_DYN];
#pragma unroll
        for (int j = 0; j < BM_DYN; ++j) acc[j] = 0;
#pragma unroll
        for (int r = 0; r < BLK + BM_DYN - 1; ++r) {
            uint32_t d[BD + 1];
#pragma unroll
            for (int k = 0; k <= BD; ++k) d[k] = wp[r * LPD + k];
#pragma unroll
            for (int j = 0; j < BM_DYN; ++j) {
                if (r - j >= 0 && r - j < BLK) {
#pragma unroll
                    for (int k = 0; k < BD; ++k)
                        acc[j] = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)d[k + 1] << 32) | d[k], cb[r - j][k], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < BM_DYN; ++j) {
            const int dy = BM_DYN * dg + j - R;
            const bool oky = dy <= R && y0 + dy >= 0 && y0 + dy + BLK <= H;     // dy >= -R by construction
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int dx = 4 * g + q - R4;
                const bool ok = oky && dx >= -R && dx <= R && x + dx >= 0 && x + dx + BLK <= W;
                const unsigned long long s = (acc[j] >> (16 * q)) & 0xffffu;
                const unsigned long long key = (s << 26) | ((unsigned long long)(dy * dy + dx * dx) << 14) | ((unsigned long long)(dy + 64) << 7) |
                                               (unsigned long long)(dx + 64);
                if (ok && key < best) best = key;
                if (ok && dy == 0 && dx == 0) sad0_out[(pair * Hb + by) * Wb + bx] = (int32_t)s;           // exactly one lane of the wave
            }
        }
    }
    best = wave_min_u64(best);                                                  // (0, 0) is always admitted: never ~0
    if (lane == 0) {
        const long o = (pair * Hb + by) * Wb + bx;
        mv[2 * o] = (int16_t)((int)((best >> 7) & 127) - 64);
        mv[2 * o + 1] = (int16_t)((int)(best & 127) - 64);
        sad_out[o] = (int32_t)(best >> 26);
    }
}

// one wave per block, four blocks per workgroup
__global__ __launch_bounds__(256) void block_warp_sse_kernel(RgbSrc A, RgbSrc B, const int16_t* __restrict__ mv, int n_inner, int H, int W, int block, int Hb, int Wb,
                                                             long blocks, int32_t* __restrict__ sse, int32_t* __restrict__ sse0, int* __restrict__ status) {
    const long o = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= blocks) return;
    const int lane = threadIdx.x & 63;
    const int bx = (int)(o % Wb);
    long t = o / Wb;
    const int by = (int)(t % Hb);
    const long pair = t / Hb, po = pair / n_inner, pi = pair - po * n_inner;
    const int y = by * block, x = bx * block;
    const int ty = y + mv[2 * o], tx = x + mv[2 * o + 1];
    const int ry = min(max(ty, 0), H - block), rx = min(max(tx, 0), W - block); // the displaced origin, clamped into the frame
    if (lane == 0 && (ry != ty || rx != tx)) atomicAdd(status, 1);
    const uint8_t* a = A.p + po * A.so + pi * A.si + (long)y * A.sr + (long)x * A.sp;
    const uint8_t* b0 = B.p + po * B.so + pi * B.si + (long)y * B.sr + (long)x * B.sp;
    const uint8_t* b1 = B.p + po * B.so + pi * B.si + (long)ry * B.sr + (long)rx * B.sp;
    int s = 0, s0 = 0;
    for (int idx = lane; idx < block * block; idx += 64) {
        const int i = idx / block, j = idx - i * block;                         // 0 <= y + i, ry + i < H and 0 <= x + j, rx + j < W
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int va = a[(long)i * A.sr + (long)j * A.sp + c * A.sc];
            const int d0 = va - (int)b0[(long)i * B.sr + (long)j * B.sp + c * B.sc], d1 = va - (int)b1[(long)i * B.sr + (long)j * B.sp + c * B.sc];
            s0 += d0 * d0;
            s += d1 * d1;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        s0 += __shfl_xor(s0, off, 64);
    }
    if (lane == 0) {
        sse[o] = s;
        sse0[o] = s0;
    }
}

bool strides_ok(long so, long si, long sr, long sp, long sc) { return so >= 0 && si >= 0 && sr >= 0 && sp >= 0 && sc >= 0; }

}  // namespace

extern "C" long tg_luma_pitch(int W) { return W < 1 ? 0 : ((long)W + 3) & ~3L; }

extern "C" int tg_luma_u8(const void* src, long so, long si, long sr, long sp, long sc, int n_outer, int n_inner, int H, int W, void* dst, hipStream_t stream) {
    TG_REQUIRE(src && dst, TG_ERR_ARG, "tg_luma_u8: null pointer");
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && H >= 1 && W >= 1, TG_ERR_SHAPE, "tg_luma_u8: bad shape n_outer=%d n_inner=%d H=%d W=%d", n_outer, n_inner, H, W);
    TG_REQUIRE(strides_ok(so, si, sr, sp, sc), TG_ERR_SHAPE, "tg_luma_u8: negative stride");
    TG_REQUIRE(((uintptr_t)dst & 3) == 0, TG_ERR_ALIGN, "tg_luma_u8: dst must be 4-byte aligned");
    const int pitch4 = (int)(tg_luma_pitch(W) / 4);
    const long total = (long)n_outer * n_inner * H * pitch4;
    const long grid = (total + 255) / 256;
    const RgbSrc S{(const uint8_t*)src, so, si, sr, sp, sc};
    hipLaunchKernelGGL(luma_kernel, dim3((unsigned)(grid < (1L << 20) ? grid : (1L << 20))), dim3(256), 0, stream, S, n_inner, H, W, pitch4, total, (uint32_t*)dst);
    TG_LAUNCH_CHECK("tg_luma_u8");
    return TG_OK;
}

extern "C" int tg_block_motion(const void* cur, long cur_so, long cur_si, const void* ref, long ref_so, long ref_si, int n_outer, int n_inner, int H, int W, long pitch,
                               int block, int radius, void* mv, void* sad, void* sad0, hipStream_t stream) {
    TG_REQUIRE(cur && ref && mv && sad && sad0, TG_ERR_ARG, "tg_block_motion: null pointer");
    TG_REQUIRE(block == 8 || block == 16, TG_ERR_ARG, "tg_block_motion: block must be 8 or 16 (got %d)", block);
    TG_REQUIRE(radius >= 1 && radius <= BM_RMAX, TG_ERR_ARG, "tg_block_motion: radius must be in 1..%d (got %d)", BM_RMAX, radius);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && H >= block && W >= block, TG_ERR_SHAPE, "tg_block_motion: bad shape n_outer=%d n_inner=%d H=%d W=%d for block %d", n_outer,
               n_inner, H, W, block);
    TG_REQUIRE(pitch >= W && pitch % 4 == 0 && pitch < (1L << 30) && cur_so >= 0 && cur_si >= 0 && ref_so >= 0 && ref_si >= 0 &&
                   ((cur_so | cur_si | ref_so | ref_si) & 3) == 0,
               TG_ERR_SHAPE, "tg_block_motion: pitch must be a multiple of 4 and >= W, plane strides non-negative multiples of 4");
    TG_REQUIRE((((uintptr_t)cur | (uintptr_t)ref | (uintptr_t)sad | (uintptr_t)sad0) & 3) == 0 && ((uintptr_t)mv & 1) == 0, TG_ERR_ALIGN,
               "tg_block_motion: planes, sad and sad0 must be 4-byte aligned, mv 2-byte");
    const int Hb = H / block, Wb = W / block, strips = (Wb + BM_STRIP - 1) / BM_STRIP;
    const long grid = (long)n_outer * n_inner * Hb * strips;
    TG_REQUIRE(grid < (1L << 31), TG_ERR_SHAPE, "tg_block_motion: too many blocks");
    if (block == 16)
        hipLaunchKernelGGL(block_motion_kernel<16>, dim3((unsigned)grid), dim3(256), 0, stream, (const uint8_t*)cur, (const uint8_t*)ref, cur_so, cur_si, ref_so, ref_si,
                           n_inner, H, W, (int)pitch, radius, Hb, Wb, strips, (int16_t*)mv, (int32_t*)sad, (int32_t*)sad0);
    else
        hipLaunchKernelGGL(block_motion_kernel<8>, dim3((unsigned)grid), dim3(256), 0, stream, (const uint8_t*)cur, (const uint8_t*)ref, cur_so, cur_si, ref_so, ref_si,
                           n_inner, H, W, (int)pitch, radius, Hb, Wb, strips, (int16_t*)mv, (int32_t*)sad, (int32_t*)sad0);
    TG_LAUNCH_CHECK("tg_block_motion");
    return TG_OK;
}

extern "C" int tg_block_warp_sse(const void* cur, long a_so, long a_si, long a_sr, long a_sp, long a_sc, const void* ref, long b_so, long b_si, long b_sr, long b_sp,
                                 long b_sc, const void* mv, int n_outer, int n_inner, int H, int W, int block, void* sse, void* sse0, int* status, hipStream_t stream) {
    TG_REQUIRE(cur && ref && mv && sse && sse0 && status, TG_ERR_ARG, "tg_block_warp_sse: null pointer");
    TG_REQUIRE(block == 8 || block == 16, TG_ERR_ARG, "tg_block_warp_sse: block must be 8 or 16 (got %d)", block);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && H >= block && W >= block, TG_ERR_SHAPE, "tg_block_warp_sse: bad shape n_outer=%d n_inner=%d H=%d W=%d for block %d",
               n_outer, n_inner, H, W, block);
    TG_REQUIRE(strides_ok(a_so, a_si, a_sr, a_sp, a_sc) && strides_ok(b_so, b_si, b_sr, b_sp, b_sc), TG_ERR_SHAPE, "tg_block_warp_sse: negative stride");
    TG_REQUIRE((((uintptr_t)sse | (uintptr_t)sse0 | (uintptr_t)status) & 3) == 0 && ((uintptr_t)mv & 1) == 0, TG_ERR_ALIGN,
               "tg_block_warp_sse: sse, sse0 and status must be 4-byte aligned, mv 2-byte");
    const int Hb = H / block, Wb = W / block;
    const long blocks = (long)n_outer * n_inner * Hb * Wb, grid = (blocks + 3) / 4;
    TG_REQUIRE(grid < (1L << 31), TG_ERR_SHAPE, "tg_block_warp_sse: too many blocks");
    const RgbSrc A{(const uint8_t*)cur, a_so, a_si, a_sr, a_sp, a_sc}, B{(const uint8_t*)ref, b_so, b_si, b_sr, b_sp, b_sc};
    hipLaunchKernelGGL(block_warp_sse_kernel, dim3((unsigned)grid), dim3(256), 0, stream, A, B, (const int16_t*)mv, n_inner, H, W, block, Hb, Wb, blocks, (int32_t*)sse,
                       (int32_t*)sse0, status);
    TG_LAUNCH_CHECK("tg_block_warp_sse");
    return TG_OK;
}
