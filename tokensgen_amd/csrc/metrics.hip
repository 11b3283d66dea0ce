// How close two videos are, in the pixels: per image plane the sum of squared differences (PSNR) and the sum of the SSIM map, one launch for all planes.
//   tg_image_metrics: the arithmetic of longvgen/metrics/psnr_ssim.py:50-79 (calculate_psnr_pt), :159-195 (calculate_ssim_pt) and :266-296 (_ssim_pth), with
//                  rgb2ycbcr_pt(y_only=True) of longvgen/utils/color_util.py:186-208, all in float64 on the 0..255 scale: a uint8 value as it is, an fp32 / bf16 value in
//                  [0, 1] times 255.0 (exact in float64: the reference's `img.to(float64) * 255.`).  The window is the 11-tap gaussian, sigma 1.5, normalised in float64
//                  (what cv2.getGaussianKernel(11, 1.5) is taken to return: its source is absent, a stated assumption), applied separably and "valid".
//                  A workgroup owns a 16 x 32 tile of window positions of one plane.  It stages the 26 x 42 pixels under the tile, of both inputs, in LDS as float64
//                  (luma mode reduces the three channels to Y in this load), and adds up (a - b)^2 over the pixels the tile OWNS: its first 16 rows and 32 columns, all
//                  of them in the last tile row / column, so that every pixel of the plane has one owner.  The horizontal pass leaves the five moments (a, b, a^2, b^2,
//                  ab filtered along the row) of the 26 x 32 positions in LDS, four neighbouring columns per thread from 14 staged pixels; the vertical pass runs in
//                  registers, two rows of one column per thread from 12 rows of moments, and ends in the SSIM map value.  Both passes add their 11 terms in tap order
//                  with fused multiply-adds.  The tile's two sums (fixed order: lanes by butterfly, then the four waves) go to a workspace of the caller's; a second
//                  launch on the same stream adds a plane's tiles in tile order.  No atomics: a plane's two numbers depend on its own pixels alone, not on how many
//                  planes the call has or where the plane stands among them.
//                  Pixels are addressed by element strides (outer image index, inner image index, channel, row, pixel), so the interleaved uint8 [.., H, W, 3] of a
//                  decoder (pixel stride 3, channel stride 1: rows of W * 3 bytes are in general not 4-byte aligned, so a pixel is loaded by itself), planar
//                  [n, C, H, W], a [B, 3, T, H, W] view and a cropped rectangle (a base offset and a smaller h, w) are one code path and cost no copy.
//                  LDS: 2 x 26 x 43 + 5 x 26 x 32 doubles = 50 KiB, three workgroups per CU.
#include <math.h>

#include "common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int IM_TH = 16;                      // window positions per tile: rows
constexpr int IM_TW = 32;                      // ... and columns
constexpr int IM_TAPS = 11;
constexpr int IM_IH = IM_TH + IM_TAPS - 1;     // 26 staged rows
constexpr int IM_IW = IM_TW + IM_TAPS - 1;     // 42 staged columns
constexpr int IM_PITCH = IM_IW + 1;            // odd pitch: the horizontal pass reads one row per eight lanes

struct ImSrc { const void* p; long so, si, sc, sr, sp; };      // element strides: outer image index, inner image index, channel, row, pixel
struct ImWin { double w[IM_TAPS]; };

ImWin gaussian_window() {
    ImWin g;
    double s = 0.0;
    for (int i = 0; i < IM_TAPS; ++i) {
        const double d = i - (IM_TAPS - 1) / 2;
        g.w[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        s += g.w[i];
    }
    for (int i = 0; i < IM_TAPS; ++i) g.w[i] /= s;
    return g;
}

template <int DT>                              // 0 uint8, 1 fp32, 2 bf16: the value on the 0..255 scale
__device__ __forceinline__ double im_load(const void* p, long off) {
    if constexpr (DT == 0) return (double)((const uint8_t*)p)[off];
    else if constexpr (DT == 1) return (double)((const float*)p)[off] * 255.0;
    else return (double)bf16_to_f32(((const bf16_t*)p)[off]) * 255.0;
}

// BT.601 luma on the 0..255 scale, each operation rounded by itself in this order (no fused multiply-add): the same bits as the elementwise float64 expression
__device__ __forceinline__ double im_luma(double r, double g, double b) {
#pragma clang fp contract(off)
    return (65.481 * r + 128.553 * g + 24.966 * b) / 255.0 + 16.0;
}

// the SSIM map value from the five moments (a, b, a^2, b^2, ab under the window), every operation rounded by itself: two identical images give numerators and
// denominators with the same bits, so exactly 1
__device__ __forceinline__ double im_ssim(const double (&m)[5]) {
#pragma clang fp contract(off)
    constexpr double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
    const double mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
    const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
    return ((2.0 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * ((2.0 * s12 + c2) / (s1 + s2 + c2));
}

template <int DT, bool Y>
__device__ __forceinline__ double im_pixel(const ImSrc& s, long off) {
    if constexpr (Y) return im_luma(im_load<DT>(s.p, off), im_load<DT>(s.p, off + s.sc), im_load<DT>(s.p, off + 2 * s.sc));
    else return im_load<DT>(s.p, off);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int DT, bool Y>
__global__ __launch_bounds__(256) void image_metrics_kernel(ImSrc A, ImSrc B, int n_inner, int C, int h, int w, int tiles_x, int tiles_y, ImWin win,
                                                            double* __restrict__ ws) {
    __shared__ double sa[IM_IH][IM_PITCH], sb[IM_IH][IM_PITCH];      // 2 x 8 944 B
    __shared__ double mo[5][IM_IH][IM_TW];                           // 33 280 B
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y, plane = blk / tiles_y;
    const int image = Y ? plane : plane / C, ch = Y ? 0 : plane - image * C;
    const long io = image / n_inner, ii = image - io * n_inner;
    const int y0 = ty * IM_TH, x0 = tx * IM_TW;
    const int rows = min(IM_IH, h - y0), cols = min(IM_IW, w - x0);                  // staged pixels inside the plane: at least 11 x 11
    const int own_r = ty == tiles_y - 1 ? rows : IM_TH, own_c = tx == tiles_x - 1 ? cols : IM_TW;
    const long base_a = io * A.so + ii * A.si + ch * A.sc, base_b = io * B.so + ii * B.si + ch * B.sc;

    double sse = 0.0;
    for (int idx = tid; idx < IM_IH * IM_IW; idx += 256) {
        const int r = idx / IM_IW, c = idx - r * IM_IW;
        double va = 0.0, vb = 0.0;
        if (r < rows && c < cols) {                                                  // 0 <= y0 + r < h and 0 <= x0 + c < w
            va = im_pixel<DT, Y>(A, base_a + (long)(y0 + r) * A.sr + (long)(x0 + c) * A.sp);
            vb = im_pixel<DT, Y>(B, base_b + (long)(y0 + r) * B.sr + (long)(x0 + c) * B.sp);
            if (r < own_r && c < own_c) {
                const double d = va - vb;
                sse = fma(d, d, sse);
            }
        }
        sa[r][c] = va;
        sb[r][c] = vb;
    }
    __syncthreads();

    // horizontal pass: row hr, positions hc .. hc + 3.  Pixel k of the 14 is tap k - j of position j: ascending k is ascending tap order for every position.
    if (tid < IM_IH * (IM_TW / 4)) {
        const int hr = tid >> 3, hc = (tid & 7) * 4;
        double m[4][5];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[j][q] = 0.0;
#pragma unroll
        for (int k = 0; k < IM_TAPS + 3; ++k) {
            const double a = sa[hr][hc + k], b = sb[hr][hc + k];                     // hc + k <= 28 + 13 < IM_IW
            const double v[5] = {a, b, a * a, b * b, a * b};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k - j >= 0 && k - j < IM_TAPS) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[j][q] = fma(win.w[k - j], v[q], m[j][q]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) mo[q][hr][hc + j] = m[j][q];
    }
    __syncthreads();

    // vertical pass: column vc, positions vr and vr + 1, from moment rows vr .. vr + 11 (<= 14 + 11 < IM_IH)
    const int vc = tid & (IM_TW - 1), vr = (tid >> 5) * 2;
    double m[2][5];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) m[j][q] = 0.0;
#pragma unroll
    for (int k = 0; k < IM_TAPS + 1; ++k) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = mo[q][vr + k][vc];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (k - j >= 0 && k - j < IM_TAPS) {
#pragma unroll
                for (int q = 0; q < 5; ++q) m[j][q] = fma(win.w[k - j], v[q], m[j][q]);
            }
        }
    }
    const int ho = h - (IM_TAPS - 1), wo = w - (IM_TAPS - 1);
    double ssim = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double v = im_ssim(m[j]);
        if (y0 + vr + j < ho && x0 + vc < wo) ssim += v;                             // positions past the plane were filtered over zeros and are dropped here
    }

    sse = wave_sum_f64(sse);
    ssim = wave_sum_f64(ssim);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = sse;
        red[1][tid >> 6] = ssim;
    }
    __syncthreads();
    if (tid == 0) {
        double* o = ws + ((long)plane * tiles_y * tiles_x + (long)ty * tiles_x + tx) * 2;
        o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// one wave per plane: lane l adds tiles l, l + 64, ... in that order, then the lanes by butterfly
__global__ __launch_bounds__(64) void image_metrics_finalize_kernel(const double* __restrict__ ws, long tiles, double* __restrict__ out) {
    const long plane = blockIdx.x;
    const double* p = ws + plane * tiles * 2;
    double sse = 0.0, ssim = 0.0;
    for (long t = threadIdx.x; t < tiles; t += 64) {
        sse += p[2 * t];
        ssim += p[2 * t + 1];
    }
    sse = wave_sum_f64(sse);
    ssim = wave_sum_f64(ssim);
    if (threadIdx.x == 0) {
        out[2 * plane] = sse;
        out[2 * plane + 1] = ssim;
    }
}

template <int DT>
void launch_metrics(bool y, unsigned grid, hipStream_t stream, const ImSrc& A, const ImSrc& B, int n_inner, int C, int h, int w, int tiles_x, int tiles_y,
                    const ImWin& win, double* ws) {
    if (y)
        hipLaunchKernelGGL((image_metrics_kernel<DT, true>), dim3(grid), dim3(256), 0, stream, A, B, n_inner, C, h, w, tiles_x, tiles_y, win, ws);
    else
        hipLaunchKernelGGL((image_metrics_kernel<DT, false>), dim3(grid), dim3(256), 0, stream, A, B, n_inner, C, h, w, tiles_x, tiles_y, win, ws);
}

long tiles_of(int n, int tile) { return (n - (IM_TAPS - 1) + tile - 1) / tile; }

}  // namespace

extern "C" long tg_image_metrics_tile(int axis) { return axis == 0 ? IM_TH : axis == 1 ? IM_TW : 0; }

extern "C" long tg_image_metrics_ws_doubles(long planes, int h, int w) {
    if (planes < 1 || h < IM_TAPS || w < IM_TAPS) return 0;
    return planes * tiles_of(h, IM_TH) * tiles_of(w, IM_TW) * 2;
}

extern "C" int tg_image_metrics_window(double* taps) {
    TG_REQUIRE(taps, TG_ERR_ARG, "tg_image_metrics_window: null pointer");
    const ImWin g = gaussian_window();
    for (int i = 0; i < IM_TAPS; ++i) taps[i] = g.w[i];
    return TG_OK;
}

extern "C" int tg_image_metrics(const void* a, long a_so, long a_si, long a_sc, long a_sr, long a_sp, const void* b, long b_so, long b_si, long b_sc, long b_sr,
                                long b_sp, int dtype, int n_outer, int n_inner, int C, int h, int w, int y_only, double* ws, double* out, hipStream_t stream) {
    TG_REQUIRE(a && b && ws && out, TG_ERR_ARG, "tg_image_metrics: null pointer");
    TG_REQUIRE(dtype >= 0 && dtype <= 2 && (y_only == 0 || y_only == 1), TG_ERR_ARG, "tg_image_metrics: dtype in 0..2 and y_only in 0..1 (got %d, %d)", dtype, y_only);
    TG_REQUIRE(n_outer >= 1 && n_inner >= 1 && (C == 1 || C == 3) && (!y_only || C == 3), TG_ERR_SHAPE,
               "tg_image_metrics: bad shape n_outer=%d n_inner=%d C=%d (1 or 3; 3 with y_only)", n_outer, n_inner, C);
    TG_REQUIRE(h >= IM_TAPS && w >= IM_TAPS, TG_ERR_SHAPE, "tg_image_metrics: a %d x %d plane is smaller than the %d x %d window", h, w, IM_TAPS, IM_TAPS);
    TG_REQUIRE(a_so >= 0 && a_si >= 0 && a_sc >= 0 && a_sr >= 0 && a_sp >= 0 && b_so >= 0 && b_si >= 0 && b_sc >= 0 && b_sr >= 0 && b_sp >= 0, TG_ERR_SHAPE,
               "tg_image_metrics: negative stride");
    const unsigned elem = dtype == 0 ? 0u : dtype == 1 ? 3u : 1u;
    TG_REQUIRE((((uintptr_t)a | (uintptr_t)b) & elem) == 0 && (((uintptr_t)ws | (uintptr_t)out) & 7) == 0, TG_ERR_ALIGN,
               "tg_image_metrics: the inputs must be aligned to their element, ws and out to 8 bytes");
    const long planes = (long)n_outer * n_inner * (y_only ? 1 : C);
    const long tiles_x = tiles_of(w, IM_TW), tiles_y = tiles_of(h, IM_TH);
    TG_REQUIRE(planes * tiles_x * tiles_y < (1L << 31), TG_ERR_SHAPE, "tg_image_metrics: too many tiles");
    const ImSrc A{a, a_so, a_si, a_sc, a_sr, a_sp}, B{b, b_so, b_si, b_sc, b_sr, b_sp};
    const ImWin win = gaussian_window();
    const unsigned grid = (unsigned)(planes * tiles_x * tiles_y);
    switch (dtype) {
        case 0: launch_metrics<0>(y_only, grid, stream, A, B, n_inner, C, h, w, (int)tiles_x, (int)tiles_y, win, ws); break;
        case 1: launch_metrics<1>(y_only, grid, stream, A, B, n_inner, C, h, w, (int)tiles_x, (int)tiles_y, win, ws); break;
        default: launch_metrics<2>(y_only, grid, stream, A, B, n_inner, C, h, w, (int)tiles_x, (int)tiles_y, win, ws); break;
    }
    TG_LAUNCH_CHECK("tg_image_metrics");
    hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)planes), dim3(64), 0, stream, ws, tiles_x * tiles_y, out);
    TG_LAUNCH_CHECK("tg_image_metrics (sum of the tiles)");
    return TG_OK;
}
