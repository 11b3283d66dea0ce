// Baseline JPEG of the byte output: quantised DCT coefficients, the size of every restart segment, and the byte stream.  Integer arithmetic only; the
// definition is the comment of include/tokensgen_hip.h, restated by tests/jpeg_ref.py.
//   tg_jpeg_coeffs:        a workgroup owns a strip of 64 pixels x one MCU row of one frame (four 16 x 16 MCUs at 4:2:0, eight 8 x 8 MCUs at 4:4:4: 24 blocks either
//                  way).  The strip's bytes come in by aligned 4-byte loads into LDS (a row starts at any byte: 3 W is no multiple of 4; a dword that is not wholly
//                  inside the input is read byte by byte), rows and columns past the frame repeat the last one.  Colour conversion and the 2 x 2 chroma mean leave
//                  int16 samples minus 128 in LDS.  Then eight threads per block: thread (block, y) does row y of the first matrix product, thread (block, u) column u
//                  of the second and the quantisation; every private array is indexed by unrolled constants.  The coefficients go out in zigzag order as int16, a
//                  strip's 24 blocks as one run of 16-byte stores.
//   tg_jpeg_segment_bytes: one lane per restart segment runs the entropy coder without storing: the byte count needs the stuffed FF bytes, so it needs the bytes.  The
//   tg_jpeg_write          lane walks its blocks' coefficients from memory, eight per 16-byte load (a vector of zeros is one run of eight), and keeps the DC predictors
//                  in three scalars; the Huffman tables (code << 8 | length) sit in LDS.  The write pass is the same function with a sink that stores single bytes up
//                  to the first 4-byte boundary of the output, whole dwords from there and single bytes at the end: neighbouring segments never share a byte, so
//                  there are no atomics.  Every store is checked against the end of the buffer.  A second launch writes the 629 header bytes of every frame.
#include <initializer_list>

#include "common.h"
#include "jpeg_common.h"
#include "tokensgen_hip.h"

namespace {

constexpr int JPEG_HEADER_BYTES = 629;
constexpr int JC_BLOCKS = 24;                   // blocks of a workgroup of the coefficient kernel
constexpr int JC_RAW_DWORDS = 49;               // 64 pixels x 3 bytes from any byte phase: at most 3 + 192 bytes

// Annex K.1: the luminance and chrominance quantisation tables, natural order
constexpr uint8_t QBASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40,  57,  69,  56, 14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: the four Huffman tables as BITS (codes per length 1 .. 16) and HUFFVAL
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// the canonical codes of Annex C as code << 8 | length, indexed by symbol; [table][0 .. 15] the DC categories, [table][16 + symbol] the AC (run, size) symbols
constexpr int HUFF_WORDS = 2 * (16 + 256);
struct HuffCodes { uint32_t w[HUFF_WORDS]; };
constexpr HuffCodes make_huff() {
    HuffCodes h{};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < DC_BITS[t][len - 1]; ++i) h.w[t * 272 + DC_VALS[k++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < AC_BITS[t][len - 1]; ++i) h.w[t * 272 + 16 + AC_VALS[t][k++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    return h;
}
constexpr HuffCodes HUFF = make_huff();

struct QTabs { uint8_t q[2][64]; };             // natural order
struct JpegHeader { uint8_t b[640]; };

void quant_tables(int quality, QTabs& t) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 64; ++k) {
            const int v = (QBASE[i][k] * s + 50) / 100;
            t.q[i][k] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

void build_header(int H, int W, int subsampling, int restart, const QTabs& qt, JpegHeader& h) {
    uint8_t* p = h.b;
    auto put = [&](std::initializer_list<int> l) { for (int v : l) *p++ = (uint8_t)v; };
    put({0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int i = 0; i < 2; ++i) {
        put({0xff, 0xdb, 0, 67, i});
        for (int k = 0; k < 64; ++k) *p++ = qt.q[i][ZIGZAG[k]];
    }
    put({0xff, 0xc0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, subsampling == 420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xc4, 0, 19 + 12, t});
        for (int i = 0; i < 16; ++i) *p++ = DC_BITS[t][i];
        for (int i = 0; i < 12; ++i) *p++ = DC_VALS[i];
        put({0xff, 0xc4, 0, 19 + 162, 0x10 | t});
        for (int i = 0; i < 16; ++i) *p++ = AC_BITS[t][i];
        for (int i = 0; i < 162; ++i) *p++ = AC_VALS[t][i];
    }
    put({0xff, 0xdd, 0, 4, restart >> 8, restart & 255});
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    while (p < h.b + sizeof(h.b)) *p++ = 0;     // p was h.b + JPEG_HEADER_BYTES
}

// libjpeg's fixed-point full-range conversion, samples minus 128
__device__ __forceinline__ void ycc(int r, int g, int b, int& y, int& cb, int& cr) {
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

template <bool S420>
__global__ __launch_bounds__(256) void jpeg_coeffs_kernel(const uint8_t* __restrict__ src, long total_bytes, int H, int W, int mcu_rows, int mcu_cols, int strips, QTabs qt,
                                                          int16_t* __restrict__ coef) {
    constexpr int ROWS = S420 ? 16 : 8, NM = S420 ? 4 : 8, BPM = S420 ? 6 : 3;
    __shared__ uint32_t raw[ROWS][JC_RAW_DWORDS + 1];
    __shared__ __align__(16) int16_t smp[3][ROWS][64];
    __shared__ int32_t tb[JC_BLOCKS][64];
    __shared__ __align__(16) int16_t zz[JC_BLOCKS][64];
    __shared__ uint8_t qs[2][64];
    const int tid = threadIdx.x;
    long blk = blockIdx.x;
    const int strip = (int)(blk % strips);
    blk /= strips;
    const int my = (int)(blk % mcu_rows);
    const long f = blk / mcu_rows;
    const int x0 = strip * 64, y0 = my * ROWS;                                  // x0 < W and y0 < H: the strip and the MCU row exist
    const int npx = W - x0 < 64 ? W - x0 : 64;
    const uint8_t* frame = src + f * 3L * H * W;
    const uint8_t* src_end = src + total_bytes;
    if (tid < 128) qs[tid >> 6][tid & 63] = qt.q[tid >> 6][tid & 63];
    for (int i = tid; i < ROWS * JC_RAW_DWORDS; i += 256) {
        const int r = i / JC_RAW_DWORDS, d = i - r * JC_RAW_DWORDS;
        const int py = y0 + r < H ? y0 + r : H - 1;
        const uint8_t* s = frame + ((long)py * W + x0) * 3;                     // the row's first byte; its npx pixels lie inside the frame
        const uint8_t* q = s - ((uintptr_t)s & 3) + 4 * d;                      // aligned dword d of the row
        uint32_t v = 0;
        if (q < s + 3 * npx) {
            if (q >= src && q + 4 <= src_end) {
                v = *(const uint32_t*)q;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (q + k >= src && q + k < src_end) v |= (uint32_t)q[k] << (8 * k);
            }
        }
        raw[r][d] = v;
    }
    __syncthreads();
    if constexpr (S420) {
        const int qx = tid & 31, qy = tid >> 5;                                 // one 2 x 2 quad per thread
        int sb = 0, sr = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * qy + dy;
            const int py = y0 + y < H ? y0 + y : H - 1;
            const int phase = (int)(((uintptr_t)frame + ((long)py * W + x0) * 3) & 3);
            const uint8_t* row = (const uint8_t*)raw[y] + phase;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * qx + dx, cx = x < npx ? x : npx - 1;
                int yy, cb, cr;
                ycc(row[3 * cx], row[3 * cx + 1], row[3 * cx + 2], yy, cb, cr);
                smp[0][y][x] = (int16_t)(yy - 128);
                sb += cb;
                sr += cr;
            }
        }
        smp[1][qy][qx] = (int16_t)(((sb + 2) >> 2) - 128);
        smp[2][qy][qx] = (int16_t)(((sr + 2) >> 2) - 128);
    } else {
        const int x = tid & 63, cx = x < npx ? x : npx - 1;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int y = (tid >> 6) + 4 * k;
            const int py = y0 + y < H ? y0 + y : H - 1;
            const int phase = (int)(((uintptr_t)frame + ((long)py * W + x0) * 3) & 3);
            const uint8_t* row = (const uint8_t*)raw[y] + phase;
            int yy, cb, cr;
            ycc(row[3 * cx], row[3 * cx + 1], row[3 * cx + 2], yy, cb, cr);
            smp[0][y][x] = (int16_t)(yy - 128);
            smp[1][y][x] = (int16_t)(cb - 128);
            smp[2][y][x] = (int16_t)(cr - 128);
        }
    }
    __syncthreads();
    const int b = tid >> 3, i8 = tid & 7;                                       // block of the strip, row (first product) or column (second product)
    int plane = 0;
    if (b < JC_BLOCKS) {
        const int m = b / BPM, k = b - m * BPM;
        int bx, by = 0;
        if constexpr (S420) {
            plane = k < 4 ? 0 : k - 3;
            bx = k < 4 ? m * 16 + (k & 1) * 8 : m * 8;
            by = k < 4 ? (k >> 1) * 8 : 0;
        } else {
            plane = k;
            bx = m * 8;
        }
        const uint4 pv = *(const uint4*)&smp[plane][by + i8][bx];              // bx is a multiple of 8: 16 bytes, aligned
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
        int p[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = (int16_t)(pw[x >> 1] >> (16 * (x & 1)));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int s = 512;
#pragma unroll
            for (int x = 0; x < 8; ++x) s += DCT_A[u][x] * p[x];
            tb[b][i8 * 8 + u] = s >> 10;
        }
    }
    __syncthreads();
    if (b < JC_BLOCKS) {
        int t[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) t[y] = tb[b][y * 8 + i8];
        const uint8_t* q = qs[plane != 0];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int s = 32768;
#pragma unroll
            for (int y = 0; y < 8; ++y) s += DCT_A[v][y] * t[y];
            const int c = s >> 16, n = v * 8 + i8, Q = q[n];
            int a = ((c < 0 ? -c : c) + (Q >> 1)) / Q;
            if (n != 0 && a > 1023) a = 1023;
            zz[b][UNZIG.at[n]] = (int16_t)(c < 0 ? -a : a);
        }
    }
    __syncthreads();
    const int nv = mcu_cols - strip * NM < NM ? mcu_cols - strip * NM : NM;     // MCUs of the strip that exist
    uint4* out = (uint4*)(coef + ((f * mcu_rows + my) * mcu_cols + (long)strip * NM) * (BPM * 64));
    if (tid < nv * BPM * 8) out[tid] = ((const uint4*)&zz[0][0])[tid];          // nv BPM <= 24: at most 192 vectors
}

// the 8-bit bytes of one segment: counted, and with WRITE stored
template <bool WRITE>
struct ByteSink {
    uint8_t* p;                                 // where the next byte goes
    uint8_t* end;                               // no store at or past this address
    uint32_t w;
    int nb;
    long count;
    __device__ __forceinline__ void emit(uint32_t byte) {
        ++count;
        if constexpr (WRITE) {
            if (nb == 0 && ((uintptr_t)p & 3) != 0) {
                if (p < end) *p = (uint8_t)byte;
                ++p;
            } else {
                w |= byte << (8 * nb);
                ++nb;
                ++p;
                if (nb == 4) {
                    if (p <= end) *(uint32_t*)(p - 4) = w;                      // p - 4 is 4-byte aligned
                    w = 0;
                    nb = 0;
                }
            }
        }
    }
    __device__ __forceinline__ void finish() {
        if constexpr (WRITE) {
            for (int i = 0; i < nb; ++i)
                if (p - nb + i < end) p[i - nb] = (uint8_t)(w >> (8 * i));
            nb = 0;
        }
    }
};

template <bool WRITE>
struct BitWriter {
    ByteSink<WRITE> out;
    uint64_t acc;
    int n;                                      // bits of acc not yet emitted, < 8 between calls
    __device__ __forceinline__ void put(uint32_t code, int len) {              // len <= 27
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) {
            const uint32_t byte = (uint32_t)(acc >> (n - 8)) & 255u;
            out.emit(byte);
            if (byte == 255u) out.emit(0);
            n -= 8;
        }
    }
    __device__ __forceinline__ void put_symbol(uint32_t entry, int value, int size) {      // a Huffman code and the `size` low bits of value (of value - 1 below zero)
        const uint32_t bits = (uint32_t)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
        put(((entry >> 8) << size) | bits, (int)(entry & 255u) + size);
    }
};

__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(v < 0 ? -v : v); }

// MCUs [m0, m1) of one frame (coef: the frame's coefficients), then the padding and FF `marker`.  Returns the number of bytes.
template <bool WRITE>
__device__ long encode_segment(const int16_t* __restrict__ coef, long m0, long m1, int bpm, const uint32_t* huff, uint32_t marker, uint8_t* dst, uint8_t* end) {
    BitWriter<WRITE> bw;
    bw.out.p = dst;
    bw.out.end = end;
    bw.out.w = 0;
    bw.out.nb = 0;
    bw.out.count = 0;
    bw.acc = 0;
    bw.n = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const uint4* q = (const uint4*)(coef + m0 * bpm * 64);
    for (long m = m0; m < m1; ++m) {
        for (int k = 0; k < bpm; ++k, q += 8) {
            const int comp = k < bpm - 2 ? 0 : k - (bpm - 3);                   // 4:2:0: Y Y Y Y Cb Cr, 4:4:4: Y Cb Cr
            const uint32_t* hdc = huff + (comp != 0) * 272;
            const uint32_t* hac = hdc + 16;
            int run = 0;
            for (int g = 0; g < 8; ++g) {
                const uint4 v = q[g];
                if (g > 0 && (v.x | v.y | v.z | v.w) == 0) {
                    run += 8;
                    continue;
                }
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
                    if (g == 0 && j == 0) {
                        const int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
                        const int diff = c - pred, size = bit_size(diff);
                        bw.put_symbol(hdc[size], diff, size);
                        pred0 = comp == 0 ? c : pred0;
                        pred1 = comp == 1 ? c : pred1;
                        pred2 = comp == 2 ? c : pred2;
                    } else if (c == 0) {
                        ++run;
                    } else {
                        for (; run > 15; run -= 16) bw.put_symbol(hac[0xf0], 0, 0);
                        const int size = bit_size(c);
                        bw.put_symbol(hac[(run << 4) | size], c, size);
                        run = 0;
                    }
                }
            }
            if (run > 0) bw.put_symbol(hac[0], 0, 0);
        }
    }
    if (bw.n) bw.put((1u << (8 - bw.n)) - 1u, 8 - bw.n);
    bw.out.emit(0xff);
    bw.out.emit(marker);
    bw.out.finish();
    return bw.out.count;
}

// one lane per restart segment.  WRITE: seg_off[f][s] is the segment's first byte in data; otherwise seg_bytes[f][s] receives its length.
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, long segments, long n_seg, long n_mcu, int bpm, int restart,
                                                          int32_t* __restrict__ seg_bytes, const long long* __restrict__ seg_off, uint8_t* data, long data_bytes) {
    __shared__ uint32_t huff[HUFF_WORDS];
    for (int i = threadIdx.x; i < HUFF_WORDS; i += 64) huff[i] = HUFF.w[i];
    __syncthreads();
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= segments) return;
    const long f = id / n_seg, s = id - f * n_seg;
    const long m0 = s * restart, m1 = m0 + restart < n_mcu ? m0 + restart : n_mcu;
    const uint32_t marker = s == n_seg - 1 ? 0xd9u : 0xd0u + (uint32_t)(s & 7);
    const int16_t* fc = coef + f * n_mcu * bpm * 64;
    if constexpr (WRITE) {
        const long long off = seg_off[id];
        if (off < 0 || off > data_bytes) return;
        encode_segment<true>(fc, m0, m1, bpm, huff, marker, data + off, data + data_bytes);
    } else {
        seg_bytes[id] = (int32_t)encode_segment<false>(fc, m0, m1, bpm, huff, marker, nullptr, nullptr);
    }
}

__global__ __launch_bounds__(256) void jpeg_header_kernel(JpegHeader h, const long long* __restrict__ frame_off, uint8_t* __restrict__ data, long data_bytes) {
    const long long off = frame_off[blockIdx.x];
    for (int i = threadIdx.x; i < JPEG_HEADER_BYTES; i += 256)
        if (off >= 0 && off + i < data_bytes) data[off + i] = h.b[i];
}

long segments_of(const Geometry& g, int restart) { return (g.n_mcu + restart - 1) / restart; }

}  // namespace

extern "C" long tg_jpeg_header_bytes(void) { return JPEG_HEADER_BYTES; }

extern "C" long tg_jpeg_geometry(int H, int W, int subsampling, int restart_interval, int what) {
    Geometry g;
    if (!geometry(H, W, subsampling, g) || restart_interval < 1 || restart_interval > 65535) return 0;
    switch (what) {
        case 0: return g.rows;
        case 1: return g.cols;
        case 2: return g.bpm;
        case 3: return segments_of(g, restart_interval);
        case 4: return g.n_mcu * g.bpm * 64;
        default: return 0;
    }
}

extern "C" int tg_jpeg_coeffs(const void* frames, int F, int H, int W, int subsampling, int quality, void* coef, hipStream_t stream) {
    TG_REQUIRE(frames && coef, TG_ERR_ARG, "tg_jpeg_coeffs: null pointer");
    TG_REQUIRE(quality >= 1 && quality <= 100, TG_ERR_ARG, "tg_jpeg_coeffs: quality must be in 1..100 (got %d)", quality);
    Geometry g;
    TG_REQUIRE(F >= 1 && geometry(H, W, subsampling, g), TG_ERR_SHAPE, "tg_jpeg_coeffs: bad shape F=%d H=%d W=%d (1..65535) subsampling=%d (420 or 444)", F, H, W, subsampling);
    TG_REQUIRE(tg_aligned16(coef), TG_ERR_ALIGN, "tg_jpeg_coeffs: coef must be 16-byte aligned");
    const long strips = (g.cols * g.mcu + 63) / 64, grid = (long)F * g.rows * strips;
    TG_REQUIRE(grid < (1L << 31), TG_ERR_SHAPE, "tg_jpeg_coeffs: too many strips");
    QTabs qt;
    quant_tables(quality, qt);
    const long total = 3L * F * H * W;
    if (subsampling == 420)
        hipLaunchKernelGGL(jpeg_coeffs_kernel<true>, dim3((unsigned)grid), dim3(256), 0, stream, (const uint8_t*)frames, total, H, W, g.rows, g.cols, (int)strips, qt,
                           (int16_t*)coef);
    else
        hipLaunchKernelGGL(jpeg_coeffs_kernel<false>, dim3((unsigned)grid), dim3(256), 0, stream, (const uint8_t*)frames, total, H, W, g.rows, g.cols, (int)strips, qt,
                           (int16_t*)coef);
    TG_LAUNCH_CHECK("tg_jpeg_coeffs");
    return TG_OK;
}

extern "C" int tg_jpeg_segment_bytes(const void* coef, int F, int H, int W, int subsampling, int restart_interval, void* seg_bytes, hipStream_t stream) {
    TG_REQUIRE(coef && seg_bytes, TG_ERR_ARG, "tg_jpeg_segment_bytes: null pointer");
    TG_REQUIRE(restart_interval >= 1 && restart_interval <= 65535, TG_ERR_ARG, "tg_jpeg_segment_bytes: restart_interval must be in 1..65535 (got %d)", restart_interval);
    Geometry g;
    TG_REQUIRE(F >= 1 && geometry(H, W, subsampling, g), TG_ERR_SHAPE, "tg_jpeg_segment_bytes: bad shape F=%d H=%d W=%d (1..65535) subsampling=%d (420 or 444)", F, H, W,
               subsampling);
    TG_REQUIRE(tg_aligned16(coef) && ((uintptr_t)seg_bytes & 3) == 0, TG_ERR_ALIGN, "tg_jpeg_segment_bytes: coef must be 16-byte aligned, seg_bytes 4-byte");
    const long n_seg = segments_of(g, restart_interval), segments = n_seg * F;
    TG_REQUIRE((segments + 63) / 64 < (1L << 31), TG_ERR_SHAPE, "tg_jpeg_segment_bytes: too many segments");
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)((segments + 63) / 64)), dim3(64), 0, stream, (const int16_t*)coef, segments, n_seg, g.n_mcu, g.bpm,
                       restart_interval, (int32_t*)seg_bytes, (const long long*)nullptr, (uint8_t*)nullptr, 0L);
    TG_LAUNCH_CHECK("tg_jpeg_segment_bytes");
    return TG_OK;
}

extern "C" int tg_jpeg_write(const void* coef, int F, int H, int W, int subsampling, int quality, int restart_interval, const void* seg_offsets,
                             const void* frame_offsets, void* data, long data_bytes, hipStream_t stream) {
    TG_REQUIRE(coef && seg_offsets && frame_offsets && data, TG_ERR_ARG, "tg_jpeg_write: null pointer");
    TG_REQUIRE(quality >= 1 && quality <= 100, TG_ERR_ARG, "tg_jpeg_write: quality must be in 1..100 (got %d)", quality);
    TG_REQUIRE(restart_interval >= 1 && restart_interval <= 65535, TG_ERR_ARG, "tg_jpeg_write: restart_interval must be in 1..65535 (got %d)", restart_interval);
    Geometry g;
    TG_REQUIRE(F >= 1 && geometry(H, W, subsampling, g), TG_ERR_SHAPE, "tg_jpeg_write: bad shape F=%d H=%d W=%d (1..65535) subsampling=%d (420 or 444)", F, H, W, subsampling);
    TG_REQUIRE(data_bytes >= (long)F * (JPEG_HEADER_BYTES + 2), TG_ERR_SHAPE, "tg_jpeg_write: %ld bytes cannot hold %d frames", data_bytes, F);
    TG_REQUIRE(tg_aligned16(coef) && (((uintptr_t)seg_offsets | (uintptr_t)frame_offsets) & 7) == 0, TG_ERR_ALIGN,
               "tg_jpeg_write: coef must be 16-byte aligned, the offsets 8-byte");
    const long n_seg = segments_of(g, restart_interval), segments = n_seg * F;
    TG_REQUIRE((segments + 63) / 64 < (1L << 31), TG_ERR_SHAPE, "tg_jpeg_write: too many segments");
    QTabs qt;
    quant_tables(quality, qt);
    JpegHeader h;
    build_header(H, W, subsampling, restart_interval, qt, h);
    hipLaunchKernelGGL(jpeg_header_kernel, dim3((unsigned)F), dim3(256), 0, stream, h, (const long long*)frame_offsets, (uint8_t*)data, data_bytes);
    TG_LAUNCH_CHECK("tg_jpeg_write (headers)");
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)((segments + 63) / 64)), dim3(64), 0, stream, (const int16_t*)coef, segments, n_seg, g.n_mcu, g.bpm,
                       restart_interval, (int32_t*)nullptr, (const long long*)seg_offsets, (uint8_t*)data, data_bytes);
    TG_LAUNCH_CHECK("tg_jpeg_write");
    return TG_OK;
}
