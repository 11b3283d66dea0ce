// The two pixel ends of a run: decoded uint8 frames -> the [-1, 1] bf16 tensor vae_encode_image wants, and decoded bf16 frames -> display bytes.
//   tg_video_resample: separable antialiased resample + crop + zero pad + map to [-1, 1] of uint8 [F][H][W][3] frames, one launch for all frames.  The arithmetic of
//                  longvgen/data/long_video.py:61-76 (`video / 255.`, resize, `* 2 - 1`) with the resize of longvgen/data/utils.py:13-140 taken as
//                  F.interpolate(..., align_corners=False, antialias=True) (torchvision 0.19 `resize` on a float tensor; its source is absent here: a stated assumption,
//                  DESIGN.md).  The host supplies the filter as tables (tokensgen_amd/video_io.py: aa_weights / resample_plan): per output row a first source row, a tap
//                  count and fp32 weights, the same per output column; the crop is a slice of those tables and the pad is a first index that may be negative: a tap
//                  outside [0, H) x [0, W) contributes 0 (the reference's fill of -1 is 0 after its `(x + 1) / 2`).
//                  A workgroup owns a 16 x 64 output tile of one frame (all 3 channels).  The source rows the tile's taps touch are walked in chunks of 16: the
//                  horizontal pass leaves a chunk in LDS as fp32 [16][3][64] (pixel = float(u8) / 255.0f as the reference's division rounds it, fp32 fma in tap order),
//                  the vertical pass adds the chunk's rows to register accumulators, again in tap order, so the summation order depends on the tables alone: not on the
//                  chunking, the tile or the frame count.  out = bf16_rne(2 acc - 1), no clamp (bicubic overshoot past +-1 is the reference's behaviour).
//                  A thread reads its taps' source bytes twelve at a time (four pixels, one unaligned 12-byte load: W * 3 is in general no multiple of 4) through the
//                  vector cache, where neighbouring columns' taps overlap; only the last bytes of the buffer are read one by one.
//   tg_video_to_uint8: the display mapping in one pass, restated from diffusers 0.31, source absent (VaeImageProcessor.denormalize on a bf16 tensor, carried out in the
//                  tensor's dtype, then export_to_video's truncation or numpy_to_pil's rounding): r = clamp(bf16_rne(float(v) * 0.5f + 0.5f), 0, 1) (the single rounding
//                  equals torch's two bf16 operations: v * 0.5 is exact), byte = float(r) * 255.0f truncated (rounding 0) or rounded half to even (rounding 1); NaN -> 0.
//                  Source bf16 with element strides for batch, channel and frame over contiguous H x W planes ([B, 3, T, H, W] of vae.decode, [B, F, 3, H, W] of a source
//                  video); destination [B][T][H][W][3] uint8, or the same r as fp32 [B][T][H][W][3] / bf16 [B][T][3][H][W] (the "np" / "pt" outputs of
//                  VideoProcessor.postprocess_video; these two keep a NaN, as torch's clamp does).  Four pixels per thread (8-byte loads, 12-byte stores) when the strides,
//                  the plane size and the pointers allow; one pixel per thread otherwise.
#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int VR_TH = 16;          // output rows per tile
constexpr int VR_TW = 64;          // output columns per tile
constexpr int VR_R = 16;           // source rows per LDS chunk
constexpr int VR_MAX_TAPS = 64;

// float(u8) / 255.0f, correctly rounded, as the division's own Newton step without its scaling and fix-up: q0 = v * (1 / 255), r = v - 255 q0 (exact in fp32),
// q = q0 + r * (1 / 255).  Equal to the IEEE quotient on all 256 inputs (tests/test_video_io_cpu.py proves it in rational arithmetic, the identity case of
// tests/test_video_io_gpu.py holds the kernel to torch's division on every byte value); a quarter of the division's instructions in a loop that is instruction-bound.
__device__ __forceinline__ float u8_unit(uint8_t b) {
    const float v = (float)b, rcp = 1.0f / 255.0f, q0 = v * rcp;
    return fmaf(fmaf(-q0, 255.0f, v), rcp, q0);
}

__global__ __launch_bounds__(256) void video_resample_kernel(const uint8_t* __restrict__ src, int nframes, int H, int W, bf16_t* __restrict__ dst, int oh, int ow,
                                                             const int32_t* __restrict__ y0, const int32_t* __restrict__ ny, const float* __restrict__ wy, int taps_y,
                                                             const int32_t* __restrict__ x0, const int32_t* __restrict__ nx, const float* __restrict__ wx, int taps_x,
                                                             int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float hbuf[VR_R][3][VR_TW];      // 12 KiB
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, f = b / tiles_y;
    const int oy0 = ty * VR_TH, ox0 = tx * VR_TW;
    const uint8_t* frame = src + (long)f * H * W * 3;
    const uint8_t* src_end = src + (long)nframes * H * W * 3;

    // source rows any output row of the tile touches, clipped to the image (the same in every thread)
    int ys = H, ye = 0;
    for (int r = 0; r < VR_TH && oy0 + r < oh; ++r) {
        const int a = y0[oy0 + r], n = min(ny[oy0 + r], taps_y);
        ys = min(ys, a);
        ye = max(ye, a + n);
    }
    ys = max(ys, 0);
    ye = min(ye, H);

    // horizontal pass: column hx of the tile, rows hr0, hr0 + 4, ... of the chunk
    const int hx = tid & (VR_TW - 1), hr0 = tid >> 6;
    const bool hok = ox0 + hx < ow;
    int hx0 = 0, hk0 = 0, hk1 = 0;
    const float* hw = wx;
    if (hok) {
        hx0 = x0[ox0 + hx];
        hk0 = max(0, -hx0);                                    // taps left of the image contribute 0 ...
        hk1 = min(min(nx[ox0 + hx], taps_x), W - hx0);         // ... and so do taps right of it
        hw = wx + (long)(ox0 + hx) * taps_x;
    }
    // vertical pass: columns 2 vx, 2 vx + 1 of the tile, output rows vr and vr + 8
    const int vx = (tid & 31) * 2, vr = tid >> 5;
    float acc[2][3][2];
    int vy0[2], vn[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int oy = oy0 + vr + 8 * j;
        vy0[j] = 0;
        vn[j] = 0;
        if (oy < oh) {
            vy0[j] = y0[oy];
            vn[j] = min(ny[oy], taps_y);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c][0] = acc[j][c][1] = 0.f;
    }

    for (int cy = ys; cy < ye; cy += VR_R) {
        // the tap loop is the outer one: one weight load serves the thread's four rows, whose byte loads are independent.  Per output the order is still ascending k.
        float s[VR_R / 4][3];
        const uint8_t* p[VR_R / 4];
        bool rok[VR_R / 4];
#pragma unroll
        for (int i = 0; i < VR_R / 4; ++i) {
            const int sy = cy + hr0 + 4 * i;
            rok[i] = hok && sy < ye;                           // sy >= ys >= 0 and sy < ye <= H: inside the image
            p[i] = frame + ((long)(rok[i] ? sy : 0) * W + hx0) * 3;
            s[i][0] = s[i][1] = s[i][2] = 0.f;
        }
        for (int k = hk0; k < hk1; k += 4) {                   // four taps = 12 source bytes = three dwords per step; 0 <= hx0 + k < W for the taps used
            float w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = k + j < hk1 ? hw[k + j] : 0.f;
#pragma unroll
            for (int i = 0; i < VR_R / 4; ++i) {
                if (!rok[i]) continue;
                const uint8_t* q = p[i] + 3 * k;
                uint32_t d[3] = {0u, 0u, 0u};
                if (q + 12 <= src_end) {                       // bytes past the last tap but inside the buffer are read and not used
                    __builtin_memcpy(d, q, 12);
                } else {                                       // the last bytes of the last frame
                    for (int bb = 0; bb < 12 && q + bb < src_end; ++bb) d[bb >> 2] |= (uint32_t)q[bb] << (8 * (bb & 3));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k + j < hk1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            s[i][c] = fmaf(w[j], u8_unit((uint8_t)(d[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3)))), s[i][c]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < VR_R / 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) hbuf[hr0 + 4 * i][c][hx] = s[i][c];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // taps of this output row whose source row lies in [cy, min(cy + VR_R, ye)): ascending k over the chunks == ascending k overall
            const int k0 = max(0, cy - vy0[j]), k1 = min(vn[j], min(cy + VR_R, ye) - vy0[j]);
            const float* w = wy + (long)(oy0 + vr + 8 * j) * taps_y;
            for (int k = k0; k < k1; ++k) {
                const float wk = w[k];
                const int row = vy0[j] + k - cy;               // 0 <= row < VR_R
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float2 h = *(const float2*)&hbuf[row][c][vx];
                    acc[j][c][0] = fmaf(wk, h.x, acc[j][c][0]);
                    acc[j][c][1] = fmaf(wk, h.y, acc[j][c][1]);
                }
            }
        }
        __syncthreads();
    }

    const int ox = ox0 + vx;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int oy = oy0 + vr + 8 * j;
        if (oy >= oh || ox >= ow) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t pk = pack_bf16x2(fmaf(2.f, acc[j][c][0], -1.f), fmaf(2.f, acc[j][c][1], -1.f));
            bf16_t* o = dst + (((long)f * 3 + c) * oh + oy) * ow + ox;
            if ((ow & 1) == 0) {                               // ox is even: a 4-byte aligned pair inside the row
                *(uint32_t*)o = pk;
            } else {
                o[0] = (bf16_t)(pk & 0xffffu);
                if (ox + 1 < ow) o[1] = (bf16_t)(pk >> 16);
            }
        }
    }
}

// ---------------------------------------------------------------- tg_video_to_uint8 ----------------------------------------------------------------
// r of the header comment as fp32, and whether the source was a NaN
__device__ __forceinline__ float display_unit(float v) {
    float r = round_bf16(fmaf(v, 0.5f, 0.5f));                 // v * 0.5f is exact: one rounding, as bf16(bf16(v * 0.5) + 0.5)
    r = r > 0.f ? r : 0.f;                                     // NaN -> 0 here; the float outputs put it back
    return r < 1.f ? r : 1.f;
}

__device__ __forceinline__ uint32_t display_byte(float v, int rounding) {
    const float x = display_unit(v) * 255.0f;                  // exact: 8 x 8 significant bits
    return (uint32_t)(rounding ? rintf(x) : x);                // rintf: half to even in the default rounding mode
}

template <int KIND, bool VEC>                                  // KIND 0: uint8 [B][T][HW][3], 1: fp32 [B][T][HW][3], 2: bf16 [B][T][3][HW]
__global__ __launch_bounds__(256) void video_display_kernel(const bf16_t* __restrict__ src, long sb, long sc, long st, int T, long HW, long total, void* __restrict__ dst,
                                                            int rounding) {
    constexpr int PX = VEC ? 4 : 1;
    const long per_plane = HW / PX;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
        const long plane = g / per_plane, p = (g - plane * per_plane) * PX;      // plane = b * T + t
        const long bi = plane / T, t = plane - bi * T;
        const bf16_t* s = src + bi * sb + t * st + p;
        float v[3][PX];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC) {
                const uint2 raw = *(const uint2*)(s + c * sc);
                v[c][0] = bf16lo_to_f32(raw.x); v[c][1] = bf16hi_to_f32(raw.x); v[c][2] = bf16lo_to_f32(raw.y); v[c][3] = bf16hi_to_f32(raw.y);
            } else {
                v[c][0] = bf16_to_f32(s[c * sc]);
            }
        }
        if constexpr (KIND == 0) {
            uint8_t* o = (uint8_t*)dst + (plane * HW + p) * 3;
            if constexpr (VEC) {
                uint32_t by[12];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) by[3 * i + c] = display_byte(v[c][i], rounding);
#pragma unroll
                for (int w = 0; w < 3; ++w) ((uint32_t*)o)[w] = by[4 * w] | (by[4 * w + 1] << 8) | (by[4 * w + 2] << 16) | (by[4 * w + 3] << 24);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (uint8_t)display_byte(v[c][0], rounding);
            }
        } else if constexpr (KIND == 1) {
            float* o = (float*)dst + (plane * HW + p) * 3;
#pragma unroll
            for (int i = 0; i < PX; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[3 * i + c] = v[c][i] != v[c][i] ? v[c][i] : display_unit(v[c][i]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                bf16_t* o = (bf16_t*)dst + (plane * 3 + c) * HW + p;
                float r[PX];
#pragma unroll
                for (int i = 0; i < PX; ++i) r[i] = v[c][i] != v[c][i] ? v[c][i] : display_unit(v[c][i]);
                if constexpr (VEC) {
                    *(uint2*)o = make_uint2(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]));
                } else {
                    o[0] = f32_to_bf16(r[0]);
                }
            }
        }
    }
}

template <int KIND>
void launch_display(bool vec, unsigned grid, hipStream_t stream, const bf16_t* src, long sb, long sc, long st, int T, long HW, long total, void* dst, int rounding) {
    if (vec)
        hipLaunchKernelGGL((video_display_kernel<KIND, true>), dim3(grid), dim3(256), 0, stream, src, sb, sc, st, T, HW, total, dst, rounding);
    else
        hipLaunchKernelGGL((video_display_kernel<KIND, false>), dim3(grid), dim3(256), 0, stream, src, sb, sc, st, T, HW, total, dst, rounding);
}

}  // namespace

extern "C" int tg_video_resample(const void* src, int F, int H, int W, void* dst, int oh, int ow, const int32_t* y0, const int32_t* ny, const float* wy, int taps_y,
                                 const int32_t* x0, const int32_t* nx, const float* wx, int taps_x, hipStream_t stream) {
    TG_REQUIRE(src && dst && y0 && ny && wy && x0 && nx && wx, TG_ERR_ARG, "tg_video_resample: null pointer");
    TG_REQUIRE(F >= 1 && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && taps_y >= 1 && taps_x >= 1, TG_ERR_SHAPE,
               "tg_video_resample: bad shape F=%d H=%d W=%d oh=%d ow=%d taps_y=%d taps_x=%d", F, H, W, oh, ow, taps_y, taps_x);
    TG_REQUIRE(taps_y <= VR_MAX_TAPS && taps_x <= VR_MAX_TAPS, TG_ERR_SHAPE, "tg_video_resample: at most %d taps per axis (taps_y=%d taps_x=%d): about 15x downscaling",
               VR_MAX_TAPS, taps_y, taps_x);
    const long tiles_x = (ow + VR_TW - 1) / VR_TW, tiles_y = (oh + VR_TH - 1) / VR_TH;
    TG_REQUIRE(tiles_x * tiles_y * F < (1L << 31), TG_ERR_SHAPE, "tg_video_resample: too many tiles");
    TG_REQUIRE((((uintptr_t)dst) & 3) == 0 && (((uintptr_t)y0 | (uintptr_t)ny | (uintptr_t)wy | (uintptr_t)x0 | (uintptr_t)nx | (uintptr_t)wx) & 3) == 0, TG_ERR_ALIGN,
               "tg_video_resample: dst and the tables must be 4-byte aligned");
    hipLaunchKernelGGL(video_resample_kernel, dim3((unsigned)(tiles_x * tiles_y * F)), dim3(256), 0, stream, (const uint8_t*)src, F, H, W, (bf16_t*)dst, oh, ow, y0, ny, wy,
                       taps_y, x0, nx, wx, taps_x, (int)tiles_x, (int)tiles_y);
    TG_LAUNCH_CHECK("tg_video_resample");
    return TG_OK;
}

extern "C" int tg_video_to_uint8(const void* src, long stride_b, long stride_c, long stride_t, int B, int T, int H, int W, void* dst, int dst_kind, int rounding,
                                 hipStream_t stream) {
    TG_REQUIRE(src && dst, TG_ERR_ARG, "tg_video_to_uint8: null pointer");
    TG_REQUIRE(B >= 1 && T >= 1 && H >= 1 && W >= 1, TG_ERR_SHAPE, "tg_video_to_uint8: bad shape B=%d T=%d H=%d W=%d", B, T, H, W);
    TG_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_t >= 0, TG_ERR_SHAPE, "tg_video_to_uint8: negative stride");
    TG_REQUIRE(dst_kind >= 0 && dst_kind <= 2 && (rounding == 0 || rounding == 1), TG_ERR_ARG, "tg_video_to_uint8: dst_kind in 0..2 and rounding in 0..1 (got %d, %d)",
               dst_kind, rounding);
    const long HW = (long)H * W;
    const unsigned dst_align = dst_kind == 0 ? 3u : dst_kind == 1 ? 3u : 7u;
    TG_REQUIRE((((uintptr_t)src) & 1) == 0 && (((uintptr_t)dst) & (dst_kind == 2 ? 1u : dst_kind == 1 ? 3u : 0u)) == 0, TG_ERR_ALIGN, "tg_video_to_uint8: misaligned pointer");
    const bool vec = HW % 4 == 0 && stride_b % 4 == 0 && stride_c % 4 == 0 && stride_t % 4 == 0 && (((uintptr_t)src) & 7) == 0 && (((uintptr_t)dst) & dst_align) == 0;
    const long total = (long)B * T * (vec ? HW / 4 : HW);
    const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);      // grid-stride above that
    const bf16_t* s = (const bf16_t*)src;
    switch (dst_kind) {
        case 0: launch_display<0>(vec, grid, stream, s, stride_b, stride_c, stride_t, T, HW, total, dst, rounding); break;
        case 1: launch_display<1>(vec, grid, stream, s, stride_b, stride_c, stride_t, T, HW, total, dst, rounding); break;
        default: launch_display<2>(vec, grid, stream, s, stride_b, stride_c, stride_t, T, HW, total, dst, rounding); break;
    }
    TG_LAUNCH_CHECK("tg_video_to_uint8");
    return TG_OK;
}
