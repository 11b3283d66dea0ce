// Reading PNG: the zlib streams of a batch of frames -> filtered rows -> uint8 [F, H, W, 3].  The definition is the comment of
// include/tokensgen_hip.h, restated by tests/png_dec_ref.py; the decoder itself, the filter inverses and the checksum arithmetic are csrc/png_inflate.h, which
// tests/csrc/png_inflate_host.cpp compiles for the host and runs over clean and damaged streams under the sanitizers: the kernels below call the same functions.
//   tg_png_inflate:  one wave per piece.  A piece is a frame's whole deflate stream (mode 0), or one IDAT payload of a stream that is cut into independent pieces
//                  (mode 1 counts its output, mode 2 writes it where the prefix sum of the counts says).  The 64 lanes hold the same decoder state and follow the same
//                  symbols; lane 0 stores a literal, all lanes share a stored block or a match (byte i of a match of distance d is out[pos - d + i mod d], so an
//                  overlapping copy is parallel too).  A match never reads global memory: the last 64 KiB of the piece's output live in an LDS ring, every byte goes to
//                  the ring and, by a plain store that nothing reads again in this launch, to the frame's filtered rows; a workgroup barrier stands between the stores
//                  of the tokens so far and the loads of a match.  The Adler sums ride on the stores: a lane adds d and (i mod 65521) d for the bytes it stores, one
//                  reduction at the end gives the piece's pair.
//   tg_png_unfilter: one wave per frame, one lane per row, 64 rows at a time as a diagonal wavefront: at step s lane r undoes pixel s - r of its row, and what it needs
//                  of the row above, the pixels s - r and s - r - 1, are the last two results of lane r - 1, taken by a shuffle.  Lane 0 reads them from the output of
//                  the 64 rows before (a barrier stands between the passes).  First it folds the pieces' Adler pairs and compares; a frame whose status is not 0 by
//                  then is zeros.
#include "common.h"
#include "png_inflate.h"
#include "tokensgen_hip.h"

namespace {

constexpr int PNGD_THREADS = 64;

struct PiWave {
    static PD_HD int lane() {
#if defined(__HIP_DEVICE_COMPILE__)
        return (int)threadIdx.x;
#else
        return 0;
#endif
    }
    static PD_HD int lanes() { return PNGD_THREADS; }
    static PD_HD void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
    static PD_HD uint64_t sum(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
        for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
#endif
        return v;
    }
};

bool pngd_geom(int H, int W, int bpp, long& row, long& frame) {
    if (H < 1 || W < 1 || (bpp != 3 && bpp != 4)) return false;
    row = 1 + (long)bpp * W;
    frame = row * H;
    return frame < (1L << 31) && (long)H * W * 3 < (1L << 31);
}

__global__ __launch_bounds__(PNGD_THREADS) void png_inflate_kernel(const uint8_t* __restrict__ data, long data_bytes, const long long* __restrict__ piece_begin,
                                                                   const long long* __restrict__ piece_end, const int32_t* __restrict__ piece_frame,
                                                                   const int32_t* __restrict__ piece_last, int mode, const long long* __restrict__ piece_at,
                                                                   uint8_t* filtered, long frame_bytes, int F, int32_t* piece_bytes, uint32_t* adler3,
                                                                   int32_t* status) {
    __shared__ PiTables tables;
    extern __shared__ __align__(16) uint8_t ring[];                             // PI_RING bytes
    const long p = blockIdx.x;
    const long long begin = piece_begin[p], end = piece_end[p];
    const int f = piece_frame[p];
    const long long at = mode == PI_CHUNK_WRITE ? piece_at[p] : 0;
    if (f < 0 || f >= F || begin < 0 || end < begin || end > data_bytes) {     // the whole wave
        if (threadIdx.x == 0) {
            atomicOr(&status[f >= 0 && f < F ? f : 0], PI_BAD_RANGE);
            if (mode == PI_CHUNK_SIZE) piece_bytes[p] = 0;
        }
        return;
    }
    long produced = 0;
    uint32_t pair[3] = {1, 0, 0};
    const int st = pi_inflate<PiWave>(data, (long)begin, (long)end, mode, piece_last[p] != 0, &tables, ring, filtered + (long)f * frame_bytes, (long)at, frame_bytes,
                                      &produced, pair);
    if (threadIdx.x == 0) {
        if (st) atomicOr(&status[f], st);
        if (mode == PI_CHUNK_SIZE) piece_bytes[p] = (int32_t)produced;
        else {
            adler3[3 * p] = pair[0];
            adler3[3 * p + 1] = pair[1];
            adler3[3 * p + 2] = pair[2];
        }
    }
}

__global__ __launch_bounds__(PNGD_THREADS) void png_unfilter_kernel(const uint8_t* __restrict__ filtered, int H, int W, int bpp, long row_bytes,
                                                                    const int32_t* __restrict__ frame_first, const uint32_t* __restrict__ adler3,
                                                                    const uint32_t* __restrict__ expect, int32_t* status, uint8_t* rgb) {
    __shared__ int verdict;
    const int lane = threadIdx.x;
    const long f = blockIdx.x;
    const uint8_t* src = filtered + f * row_bytes * H;
    uint8_t* out = rgb + f * (long)H * W * 3;
    if (lane == 0) {
        int st = status[f];
        if (!st) {
            const int first = frame_first[f], pieces = frame_first[f + 1] - first;
            if (first < 0 || pieces < 0) st = PI_BAD_RANGE;
            else if (pi_adler_of(adler3 + 3L * first, pieces) != expect[f]) st = PI_BAD_ADLER;
            if (st) status[f] = st;
        }
        verdict = st;
    }
    __syncthreads();
    if (verdict) {
        for (long i = lane; i < (long)H * W * 3; i += PNGD_THREADS) out[i] = 0;
        return;
    }
    bool bad = false;
    for (int y0 = 0; y0 < H; y0 += PNGD_THREADS) {
        if (y0) __syncthreads();                                                // the rows of the pass before are stored
        const int y = y0 + lane;
        const bool row = y < H;
        const uint8_t* in = src + (long)(row ? y : 0) * row_bytes;
        int type = row ? in[0] : 0;
        if (type > 4) {
            bad = true;
            type = 0;
        }
        const uint8_t* above = out + (long)(y0 - 1) * W * 3;                   // read by lane 0 where y0 > 0
        int l0 = 0, l1 = 0, l2 = 0, m0 = 0, m1 = 0, m2 = 0;                     // this row's pixel x - 1 and pixel x - 2
        int a0 = 0, a1 = 0, a2 = 0;                                             // lane 0: the row above at x - 1
        for (int s = 0; s < W + PNGD_THREADS - 1; ++s) {
            const int x = s - lane;
            int b0 = __shfl_up(l0, 1, 64), b1 = __shfl_up(l1, 1, 64), b2 = __shfl_up(l2, 1, 64);
            int c0 = __shfl_up(m0, 1, 64), c1 = __shfl_up(m1, 1, 64), c2 = __shfl_up(m2, 1, 64);
            const bool on = row && x >= 0 && x < W;
            if (lane == 0) {
                c0 = a0, c1 = a1, c2 = a2;
                b0 = b1 = b2 = 0;
                if (on && y0 > 0) {
                    b0 = above[3L * x];
                    b1 = above[3L * x + 1];
                    b2 = above[3L * x + 2];
                }
                a0 = b0, a1 = b1, a2 = b2;
            }
            if (on) {
                const uint8_t* px = in + 1 + (long)x * bpp;
                const int v0 = pi_unfilter_byte(type, px[0], l0, b0, c0), v1 = pi_unfilter_byte(type, px[1], l1, b1, c1), v2 = pi_unfilter_byte(type, px[2], l2, b2, c2);
                uint8_t* o = out + ((long)y * W + x) * 3;
                o[0] = (uint8_t)v0;
                o[1] = (uint8_t)v1;
                o[2] = (uint8_t)v2;
                m0 = l0, m1 = l1, m2 = l2;
                l0 = v0, l1 = v1, l2 = v2;
            }
        }
    }
    if (bad) atomicOr(&status[f], PI_BAD_FILTER);
}

}  // namespace

extern "C" long tg_png_decode_geometry(int H, int W, int bpp, int what) {
    long row, frame;
    if (!pngd_geom(H, W, bpp, row, frame)) return 0;
    switch (what) {
        case 0: return row;
        case 1: return frame;
        case 2: return PNGD_THREADS;
        case 3: return PI_RING;
        default: return 0;
    }
}

extern "C" int tg_png_inflate(const void* data, long data_bytes, const void* piece_begin, const void* piece_end, const void* piece_frame, const void* piece_last,
                              int pieces, int mode, const void* piece_at, void* filtered, int F, int H, int W, int bpp, void* piece_bytes, void* adler3, void* status,
                              hipStream_t stream) {
    TG_REQUIRE(data && piece_begin && piece_end && piece_frame && piece_last && filtered && status, TG_ERR_ARG, "tg_png_inflate: null pointer");
    TG_REQUIRE(mode >= PI_STREAM && mode <= PI_CHUNK_WRITE, TG_ERR_ARG, "tg_png_inflate: mode must be 0 (stream), 1 (chunk sizes) or 2 (chunk write), got %d", mode);
    TG_REQUIRE(mode == PI_CHUNK_SIZE ? piece_bytes != nullptr : adler3 != nullptr, TG_ERR_ARG,
               "tg_png_inflate: null pointer (mode 1 stores piece_bytes, modes 0 and 2 store adler3)");
    TG_REQUIRE(mode != PI_CHUNK_WRITE || piece_at, TG_ERR_ARG, "tg_png_inflate: null pointer (mode 2 reads piece_at)");
    long row, frame;
    TG_REQUIRE(F >= 1 && pieces >= F && data_bytes >= 1 && pngd_geom(H, W, bpp, row, frame), TG_ERR_SHAPE,
               "tg_png_inflate: bad shape F=%d pieces=%d (at least F) data_bytes=%ld H=%d W=%d bpp=%d (3 or 4; H (1 + bpp W) and 3 H W below 2^31)", F, pieces, data_bytes,
               H, W, bpp);
    TG_REQUIRE((((uintptr_t)piece_begin | (uintptr_t)piece_end | (uintptr_t)piece_at) & 7) == 0 &&
                   (((uintptr_t)piece_frame | (uintptr_t)piece_last | (uintptr_t)piece_bytes | (uintptr_t)adler3 | (uintptr_t)status) & 3) == 0,
               TG_ERR_ALIGN, "tg_png_inflate: piece_begin, piece_end and piece_at must be 8-byte aligned, the int32 arrays 4-byte");
    TG_DYN_LDS(png_inflate_kernel, 80 * 1024);
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)pieces), dim3(PNGD_THREADS), (size_t)PI_RING, stream, (const uint8_t*)data, data_bytes, (const long long*)piece_begin,
                       (const long long*)piece_end, (const int32_t*)piece_frame, (const int32_t*)piece_last, mode, (const long long*)piece_at, (uint8_t*)filtered, frame, F,
                       (int32_t*)piece_bytes, (uint32_t*)adler3, (int32_t*)status);
    TG_LAUNCH_CHECK("tg_png_inflate");
    return TG_OK;
}

extern "C" int tg_png_unfilter(const void* filtered, int F, int H, int W, int bpp, const void* frame_first, const void* adler3, const void* expect, void* status,
                               void* rgb, hipStream_t stream) {
    TG_REQUIRE(filtered && frame_first && adler3 && expect && status && rgb, TG_ERR_ARG, "tg_png_unfilter: null pointer");
    long row, frame;
    TG_REQUIRE(F >= 1 && pngd_geom(H, W, bpp, row, frame), TG_ERR_SHAPE, "tg_png_unfilter: bad shape F=%d H=%d W=%d bpp=%d (3 or 4; H (1 + bpp W) and 3 H W below 2^31)",
               F, H, W, bpp);
    TG_REQUIRE((((uintptr_t)frame_first | (uintptr_t)adler3 | (uintptr_t)expect | (uintptr_t)status) & 3) == 0, TG_ERR_ALIGN,
               "tg_png_unfilter: frame_first, adler3, expect and status must be 4-byte aligned");
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)F), dim3(PNGD_THREADS), 0, stream, (const uint8_t*)filtered, H, W, bpp, row, (const int32_t*)frame_first,
                       (const uint32_t*)adler3, (const uint32_t*)expect, (int32_t*)status, (uint8_t*)rgb);
    TG_LAUNCH_CHECK("tg_png_unfilter");
    return TG_OK;
}
