// Lossless PNG of the byte output: filtered rows, a plan per band of rows, and the files.  Integer arithmetic only; the definition is the comment of
// include/tokensgen_hip.h, restated by tests/png_ref.py; what a run becomes, the code lengths, the block header and the checksum arithmetic are csrc/png_deflate.h,
// which tests/csrc/png_deflate_host.cpp compiles for the host.
//   tg_png_filter:    a workgroup owns one row.  Adaptive: every lane forms the five filtered values of its bytes and adds min(v, 256 - v) per type, the five sums are
//                  reduced, the smallest wins (the lowest type of equals); a second sweep stores the type and the row under it.  Filters read raw neighbours only.
//                  The workspace keeps a band's rows together and starts every band at a multiple of 16 bytes.
//   tg_png_band_plan: a workgroup owns one band (at most 65535 bytes), staged in LDS by 16-byte loads.  Lane t owns slice t of the band and the runs that START in it:
//                  a lane finds its first run start, a suffix minimum over the lanes tells where a run that leaves a slice ends, so every maximal run is seen whole by
//                  exactly one lane and its tokens are a closed form of its length (pd_run_split).  Histogram by LDS atomics, the symbols ranked in parallel, the tree
//                  and the block header by lane 0, the token bits from the histogram.  Σ d and Σ (n - i) d in 64 bits give the band's Adler pair.  Stores the plan
//                  record and the bytes of the band's IDAT chunk.
//   tg_png_write:     a workgroup owns one band and builds its whole chunk body ('IDAT', payload) in LDS: lane 0 the header's bits, every lane its runs' bits at the
//                  offset that a prefix sum of the slices' bit counts gives (whole words by LDS atomic OR: two lanes may share a word, never a bit), or the stored
//                  block.  The chunk's CRC-32 is the XOR of the slices' CRCs, each multiplied by x^(8 bytes after it) (pd_crc_mulmod).  The last band folds the frame's
//                  Adler pairs and appends the final block and the checksum; band 0 also writes signature and IHDR, the last band IEND.  Bands never share a byte of
//                  the output, there is no global atomic, and every store is checked against the end of the buffer.
#include "common.h"
#include "png_deflate.h"
#include "tokensgen_hip.h"

namespace {

constexpr int PNG_THREADS = 256;
constexpr int PNG_FILE_HEADER = 33;             // signature 8, IHDR 25
constexpr int PNG_FILE_TRAILER = 12;            // IEND
constexpr int PNG_CHUNK_FRAME = 12;             // length, type, CRC
constexpr int PNG_ZLIB_HEADER = 2;              // 78 01, in front of the first band
constexpr int PNG_ZLIB_TRAILER = 6;             // the final block 03 00 and Adler-32, after the last band
constexpr int PNG_MAX_W = 21844;
constexpr int PNG_DEFAULT_ROWS = 16;
constexpr int PNG_ADAPTIVE = 5;

struct PngPlan {                                // one per band, TG_PNG_PLAN_BYTES
    uint8_t ll[288];
    uint8_t cl[20];
    uint32_t stored, deflate_bytes, adler_a, adler_b, n, header_bits, token_bits, reserved[4];
};
static_assert(sizeof(PngPlan) == 352, "PngPlan is a plain 352-byte record");

struct PngGeom {
    int rows, bands;                            // rows of a band, bands of a frame
    long row, stride;                           // bytes of a filtered row; bytes between two bands of the workspace (a multiple of 16)
};

bool png_geom(int H, int W, int rows_per_block, PngGeom& g) {
    if (H < 1 || H > 65535 || W < 1 || W > PNG_MAX_W || rows_per_block < 0) return false;
    g.row = 1 + 3L * W;
    g.rows = rows_per_block ? rows_per_block : (int)(PD_MAX_BAND / g.row < PNG_DEFAULT_ROWS ? PD_MAX_BAND / g.row : PNG_DEFAULT_ROWS);
    if (g.rows * g.row > PD_MAX_BAND) return false;
    g.bands = (H + g.rows - 1) / g.rows;
    g.stride = (g.rows * g.row + 15) / 16 * 16;
    return true;
}

long png_chunk_lds(const PngGeom& g) {          // the chunk body of a full band in its largest form (stored), and two words of slack for the last flush
    return (4 + PNG_ZLIB_HEADER + 5 + g.rows * g.row + PNG_ZLIB_TRAILER + 15) / 16 * 16 + 16;
}

struct PngFileHeader { uint8_t b[36]; };

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

__device__ __forceinline__ int filter_byte(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255;
}

__device__ __forceinline__ int filter_cost(int v) { return v < 256 - v ? v : 256 - v; }

__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(const uint8_t* __restrict__ src, int H, int W, int filter, int rows, int bands, long row_bytes,
                                                                 long stride, uint8_t* __restrict__ filtered) {
    __shared__ int sums[5];
    __shared__ int chosen;
    const int tid = threadIdx.x, y = (int)(blockIdx.x % (unsigned)H);
    const long f = blockIdx.x / (unsigned)H;
    const int n = 3 * W;
    const uint8_t* cur = src + (f * H + y) * n;
    const uint8_t* up = y > 0 ? cur - n : cur;                                  // read only where y > 0
    int type = filter;
    if (filter == PNG_ADAPTIVE) {
        if (tid < 5) sums[tid] = 0;
        __syncthreads();
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
        for (int i = tid; i < n; i += PNG_THREADS) {
            const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= 3) ? up[i - 3] : 0;
            s0 += filter_cost(x);
            s1 += filter_cost((x - a) & 255);
            s2 += filter_cost((x - b) & 255);
            s3 += filter_cost((x - ((a + b) >> 1)) & 255);
            s4 += filter_cost((x - paeth(a, b, c)) & 255);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s0 += __shfl_xor(s0, off, 64);
            s1 += __shfl_xor(s1, off, 64);
            s2 += __shfl_xor(s2, off, 64);
            s3 += __shfl_xor(s3, off, 64);
            s4 += __shfl_xor(s4, off, 64);
        }
        if ((tid & 63) == 0) {
            atomicAdd(&sums[0], s0);
            atomicAdd(&sums[1], s1);
            atomicAdd(&sums[2], s2);
            atomicAdd(&sums[3], s3);
            atomicAdd(&sums[4], s4);
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            for (int t = 1; t < 5; ++t)
                if (sums[t] < sums[best]) best = t;                             // strictly smaller: equals stay with the lowest type
            chosen = best;
        }
        __syncthreads();
        type = chosen;
    }
    uint8_t* dst = filtered + (f * bands + y / rows) * stride + (long)(y % rows) * row_bytes;
    if (tid == 0) dst[0] = (uint8_t)type;
    for (int i = tid; i < n; i += PNG_THREADS) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= 3) ? up[i - 3] : 0;
        dst[1 + i] = (uint8_t)filter_byte(type, x, a, b, c);
    }
}

// ---- what the plan and the write kernel share: the band in LDS, a lane's slice, the runs that start in it --------------------------------------------------------------

__device__ __forceinline__ void stage_band(const uint8_t* __restrict__ band, int n, uint8_t* raw) {
    const uint4* s = (const uint4*)band;                                        // the band starts at a multiple of 16 and its stride is one: whole vectors are inside
    uint4* d = (uint4*)raw;
    for (int i = threadIdx.x; i < (n + 15) / 16; i += PNG_THREADS) d[i] = s[i];
}

// inclusive suffix minimum over the 256 lanes (s: 256 words), then what lies after the lane: the first run start behind slice t, n where there is none
__device__ __forceinline__ int next_start_after(int first, int n, int* s) {
    const int t = threadIdx.x;
    s[t] = first;
    __syncthreads();
    for (int off = 1; off < PNG_THREADS; off <<= 1) {
        const int u = t + off < PNG_THREADS ? s[t + off] : n;
        __syncthreads();
        if (u < s[t]) s[t] = u;
        __syncthreads();
    }
    const int r = t + 1 < PNG_THREADS ? s[t + 1] : n;
    __syncthreads();
    return r;
}

// exclusive prefix sum over the 256 lanes; total: the sum of all
__device__ __forceinline__ uint32_t prefix_sum(uint32_t v, uint32_t* s, uint32_t& total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < PNG_THREADS; off <<= 1) {
        const uint32_t u = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += u;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    total = s[PNG_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// the first run start in [s, e), n where the slice has none
__device__ __forceinline__ int first_start(const uint8_t* raw, int s, int e, int n) {
    for (int i = s; i < e; ++i)
        if (i == 0 || raw[i] != raw[i - 1]) return i;
    return n;
}

// f(value, length) for every run that starts in [first, e); a run that reaches the end of the slice ends at `after`
template <class F>
__device__ __forceinline__ void for_own_runs(const uint8_t* raw, int first, int e, int after, F&& f) {
    for (int i = first; i < e;) {
        const int v = raw[i];
        int j = i + 1;
        while (j < e && raw[j] == v) ++j;
        if (j == e) j = after;
        f(v, j - i);
        i = j;
    }
}

__device__ __forceinline__ uint32_t symbol_extra_bits(int s) {                  // of a literal/length symbol in the token stream: extra bits and the distance code's bit
    return s <= PD_EOB ? 0u : s < 265 || s == 285 ? 1u : 1u + (uint32_t)(s - 261) / 4u;
}

__global__ __launch_bounds__(PNG_THREADS) void png_plan_kernel(const uint8_t* __restrict__ filtered, int H, int rows, int bands, long row_bytes, long stride,
                                                               PngPlan* __restrict__ plans, int32_t* __restrict__ band_bytes) {
    extern __shared__ __align__(16) uint8_t raw[];
    __shared__ uint32_t hist[PD_LL_SYMBOLS];
    __shared__ uint16_t order[PD_LL_SYMBOLS];
    __shared__ PdTree tree;
    __shared__ PngPlan plan;
    __shared__ int scan[PNG_THREADS];
    __shared__ unsigned long long sum_d, sum_w;
    __shared__ uint32_t n_symbols, token_bits;
    const int tid = threadIdx.x;
    const long id = blockIdx.x;
    const int band = (int)(id % bands);
    const int y0 = band * rows, nrows = H - y0 < rows ? H - y0 : rows, n = (int)(nrows * row_bytes);
    stage_band(filtered + id * stride, n, raw);
    for (int s = tid; s < PD_LL_SYMBOLS; s += PNG_THREADS) hist[s] = s == PD_EOB ? 1u : 0u;
    if (tid == 0) {
        sum_d = 0;
        sum_w = 0;
        n_symbols = 0;
        token_bits = 0;
    }
    __syncthreads();
    const int C = (n + PNG_THREADS - 1) / PNG_THREADS, s0 = tid * C < n ? tid * C : n, e0 = s0 + C < n ? s0 + C : n;
    unsigned long long sd = 0, sw = 0;
    for (int i = s0; i < e0; ++i) {
        sd += raw[i];
        sw += (unsigned long long)(n - i) * raw[i];
    }
    atomicAdd(&sum_d, sd);
    atomicAdd(&sum_w, sw);
    const int first = first_start(raw, s0, e0, n);
    const int after = next_start_after(first, n, scan);
    for_own_runs(raw, first, e0, after, [&](int v, int L) { pd_run_count(v, L, [&](int s, int c) { atomicAdd(&hist[s], (uint32_t)c); }); });
    __syncthreads();
    // rank the symbols that occur by (count, symbol): a count is below 2^17, the key below 2^26
    for (int s = tid; s < PD_LL_SYMBOLS; s += PNG_THREADS) {
        if (hist[s] == 0) continue;
        const uint32_t key = hist[s] << 9 | (uint32_t)s;
        int rank = 0;
        for (int u = 0; u < PD_LL_SYMBOLS; ++u) rank += hist[u] != 0 && (hist[u] << 9 | (uint32_t)u) < key;
        order[rank] = (uint16_t)s;
        atomicAdd(&n_symbols, 1u);
    }
    __syncthreads();
    if (tid == 0) {
        pd_lengths_sorted(hist, order, (int)n_symbols, PD_LL_SYMBOLS, 15, plan.ll, &tree);
        plan.ll[286] = plan.ll[287] = 0;
        pd_cl_lengths(plan.ll, plan.cl, &tree);
        plan.cl[19] = 0;
        plan.header_bits = pd_header_bits(plan.ll, plan.cl);
    }
    __syncthreads();
    uint32_t bits = 0;
    for (int s = tid; s < PD_LL_SYMBOLS; s += PNG_THREADS)
        if (s != PD_EOB) bits += hist[s] * (plan.ll[s] + symbol_extra_bits(s));
    atomicAdd(&token_bits, bits);
    __syncthreads();
    if (tid == 0) {
        const uint32_t dynamic = pd_dynamic_bytes(plan.header_bits, token_bits, plan.ll);
        plan.stored = dynamic >= pd_stored_bytes(n);
        plan.deflate_bytes = plan.stored ? pd_stored_bytes(n) : dynamic;
        pd_adler_pair(sum_d, sum_w, (uint32_t)n, plan.adler_a, plan.adler_b);
        plan.n = (uint32_t)n;
        plan.token_bits = token_bits;
        for (int k = 0; k < 4; ++k) plan.reserved[k] = 0;
        band_bytes[id] = (int32_t)(PNG_CHUNK_FRAME + plan.deflate_bytes + (band == 0 ? PNG_ZLIB_HEADER : 0) + (band == bands - 1 ? PNG_ZLIB_TRAILER : 0));
    }
    __syncthreads();
    const uint32_t* src = (const uint32_t*)&plan;
    uint32_t* dst = (uint32_t*)(plans + id);
    for (int i = tid; i < (int)(sizeof(PngPlan) / 4); i += PNG_THREADS) dst[i] = src[i];
}

// bits into LDS words, least significant first, from any bit position: whole words by atomic OR (the words were zero; a neighbour lane may own the other bits of one)
struct LdsBits {
    uint32_t* words;
    uint32_t w;                                 // the word the low bits of acc belong to
    uint64_t acc;
    int n;                                      // bits of acc in use, < 32 between calls
    __device__ __forceinline__ void start(uint32_t* base, uint32_t bit) {
        words = base;
        w = bit >> 5;
        acc = 0;
        n = (int)(bit & 31u);
    }
    __device__ __forceinline__ void put(uint32_t value, int bits) {            // bits <= 32, value < 2^bits
        acc |= (uint64_t)value << n;
        n += bits;
        if (n >= 32) {
            atomicOr(&words[w++], (uint32_t)acc);
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (acc) atomicOr(&words[w], (uint32_t)acc);
        acc = 0;
    }
};

__device__ __forceinline__ void store_checked(uint8_t* data, long data_bytes, long at, uint32_t byte) {
    if (at >= 0 && at < data_bytes) data[at] = (uint8_t)byte;
}

__global__ __launch_bounds__(PNG_THREADS) void png_write_kernel(const uint8_t* __restrict__ filtered, const PngPlan* __restrict__ plans, int H, int rows, int bands,
                                                                long row_bytes, long stride, long raw_lds, long chunk_lds, PngFileHeader head,
                                                                const long long* __restrict__ band_off, uint8_t* data, long data_bytes) {
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ uint8_t ll[288];
    __shared__ uint8_t cl[20];
    __shared__ uint16_t code[PD_LL_SYMBOLS];
    __shared__ int next_code[16];
    __shared__ uint32_t scan[PNG_THREADS];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t crc_acc, ok;
    uint8_t* raw = lds;
    uint8_t* body = lds + raw_lds;                                              // the chunk's type and payload
    uint32_t* words = (uint32_t*)body;
    const int tid = threadIdx.x;
    const long id = blockIdx.x;
    const int band = (int)(id % bands);
    const long f = id / bands;
    const long long off = band_off[id];
    if (off < 0 || off > data_bytes) return;                                    // the whole workgroup
    const int y0 = band * rows, nrows = H - y0 < rows ? H - y0 : rows, n = (int)(nrows * row_bytes);
    const PngPlan* plan = plans + id;
    const uint32_t stored = plan->stored, deflate_bytes = plan->deflate_bytes;
    const int lead = 4 + (band == 0 ? PNG_ZLIB_HEADER : 0);                     // where the deflate bytes start in the body
    const uint32_t payload = deflate_bytes + (band == 0 ? PNG_ZLIB_HEADER : 0) + (band == bands - 1 ? PNG_ZLIB_TRAILER : 0);
    if (deflate_bytes > pd_stored_bytes(n) || (stored && deflate_bytes != pd_stored_bytes(n))) return;         // not a plan of this band: the body would not fit
    stage_band(filtered + id * stride, n, raw);
    for (int i = tid; i < (int)(chunk_lds / 4); i += PNG_THREADS) words[i] = 0;
    for (int i = tid; i < 288; i += PNG_THREADS) ll[i] = i < PD_LL_SYMBOLS ? plan->ll[i] & 15 : 0;
    if (tid < 20) cl[tid] = tid < PD_CL_SYMBOLS ? plan->cl[tid] & 7 : 0;
    crc_table[tid] = pd_crc_table_entry((uint32_t)tid);
    if (tid == 0) {
        crc_acc = 0;
        ok = 1;
    }
    __syncthreads();
    if (tid == 0) {
        words[0] = 0x54414449u;                                                 // 'IDAT'
        if (band == 0) words[1] = 0x0178u;                                      // 78 01
    }
    if (stored) {
        if (tid == 0) {
            body[lead] = 0;
            body[lead + 1] = (uint8_t)n;
            body[lead + 2] = (uint8_t)(n >> 8);
            body[lead + 3] = (uint8_t)~n;
            body[lead + 4] = (uint8_t)(~n >> 8);
        }
        for (int i = tid; i < n; i += PNG_THREADS) body[lead + 5 + i] = raw[i];
    } else {
        // the canonical codes: lane 0 the first code of every length, then every symbol its rank among the symbols of its length
        if (tid == 0) {
            int bl[16];
            for (int b = 0; b < 16; ++b) bl[b] = 0;
            for (int s = 0; s < PD_LL_SYMBOLS; ++s) ++bl[ll[s]];
            bl[0] = 0;
            int c = 0;
            next_code[0] = 0;
            for (int b = 1; b < 16; ++b) {
                c = (c + bl[b - 1]) << 1;
                next_code[b] = c;
            }
        }
        __syncthreads();
        for (int s = tid; s < PD_LL_SYMBOLS; s += PNG_THREADS) {
            const int l = ll[s];
            int rank = 0;
            for (int u = 0; u < s; ++u) rank += ll[u] == l;
            code[s] = l ? (uint16_t)(__brev((uint32_t)(next_code[l] + rank)) >> (32 - l)) : (uint16_t)0;
        }
        const int C = (n + PNG_THREADS - 1) / PNG_THREADS, s0 = tid * C < n ? tid * C : n, e0 = s0 + C < n ? s0 + C : n;
        const int first = first_start(raw, s0, e0, n);
        const int after = next_start_after(first, n, (int*)scan);
        uint32_t bits = 0, token_bits;
        for_own_runs(raw, first, e0, after, [&](int v, int L) { bits += pd_run_bits(v, L, ll); });
        const uint32_t before = prefix_sum(bits, scan, token_bits);
        const uint32_t header_bits = pd_header_bits(ll, cl);
        // the lengths of the record must give the bytes of the record: the bits below then stay inside the body
        if (tid == 0 && pd_dynamic_bytes(header_bits, token_bits, ll) != deflate_bytes) ok = 0;
        __syncthreads();
        if (!ok) return;
        LdsBits sink;
        if (tid == 0) {
            sink.start(words, 8u * lead);
            pd_header_emit(ll, cl, sink);
            sink.finish();
            sink.start(words, 8u * lead + header_bits + token_bits);
            sink.put(code[PD_EOB], ll[PD_EOB]);                                 // then the empty stored block: three zero bits, zeros to the byte, 00 00 FF FF
            sink.finish();
            sink.start(words, 8u * (lead + deflate_bytes - 4));
            sink.put(0xffff0000u, 32);
            sink.finish();
        }
        sink.start(words, 8u * lead + header_bits + before);
        for_own_runs(raw, first, e0, after, [&](int v, int L) { pd_run_emit(v, L, ll, code, sink); });
        sink.finish();
    }
    __syncthreads();
    if (band == bands - 1 && tid == 0) {                                        // the final block and the frame's Adler-32
        uint32_t A = 1, B = 0;
        const PngPlan* p = plans + f * bands;
        for (int k = 0; k < bands; ++k) pd_adler_combine(A, B, p[k].adler_a, p[k].adler_b, p[k].n);
        uint8_t* t = body + lead + deflate_bytes;
        t[0] = 3;
        t[1] = 0;
        t[2] = (uint8_t)(B >> 8);
        t[3] = (uint8_t)B;
        t[4] = (uint8_t)(A >> 8);
        t[5] = (uint8_t)A;
    }
    __syncthreads();
    // CRC-32 of type and payload
    const int total = 4 + (int)payload;
    {
        const int C = (total + PNG_THREADS - 1) / PNG_THREADS, s0 = tid * C < total ? tid * C : total, e0 = s0 + C < total ? s0 + C : total;
        uint32_t crc = 0xffffffffu;
        for (int i = s0; i < e0; ++i) crc = crc_table[(crc ^ body[i]) & 255u] ^ (crc >> 8);
        crc = e0 > s0 ? ~crc : 0u;
        if (crc) atomicXor(&crc_acc, pd_crc_mulmod(pd_crc_shift((uint32_t)(total - e0)), crc));
    }
    __syncthreads();
    const uint32_t crc = crc_acc;
    const long at = (long)off;
    if (tid < 4) {
        store_checked(data, data_bytes, at + tid, (payload >> (24 - 8 * tid)) & 255u);
        store_checked(data, data_bytes, at + 4 + total + tid, (crc >> (24 - 8 * tid)) & 255u);
    }
    for (int i = tid; i < total; i += PNG_THREADS) store_checked(data, data_bytes, at + 4 + i, body[i]);
    if (band == 0 && tid < PNG_FILE_HEADER) store_checked(data, data_bytes, at - PNG_FILE_HEADER + tid, head.b[tid]);
    if (band == bands - 1 && tid < PNG_FILE_TRAILER) {
        const uint8_t iend[PNG_FILE_TRAILER] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
        store_checked(data, data_bytes, at + 8 + total + tid, iend[tid]);
    }
}

void file_header(int H, int W, PngFileHeader& h) {
    const uint8_t b[PNG_FILE_HEADER - 4] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R', (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8),
                                            (uint8_t)W, (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8, 2, 0, 0, 0};
    for (int i = 0; i < PNG_FILE_HEADER - 4; ++i) h.b[i] = b[i];
    const uint32_t crc = pd_crc32(0, b + 12, 17);
    for (int i = 0; i < 4; ++i) h.b[PNG_FILE_HEADER - 4 + i] = (uint8_t)(crc >> (24 - 8 * i));
    for (int i = PNG_FILE_HEADER; i < (int)sizeof(h.b); ++i) h.b[i] = 0;
}

}  // namespace

extern "C" long tg_png_geometry(int H, int W, int rows_per_block, int what) {
    PngGeom g;
    if (!png_geom(H, W, rows_per_block, g)) return 0;
    switch (what) {
        case 0: return g.rows;
        case 1: return g.bands;
        case 2: return g.row;
        case 3: return g.bands * g.stride;                                      // bytes of a frame's filtered rows in the workspace
        case 4: return (long)sizeof(PngPlan);
        case 5: return PNG_FILE_HEADER + PNG_FILE_TRAILER + PNG_ZLIB_HEADER + PNG_ZLIB_TRAILER + (long)g.bands * (PNG_CHUNK_FRAME + 5) + H * g.row;     // no file is larger
        case 6: return PNG_FILE_HEADER;
        case 7: return PNG_FILE_TRAILER;
        default: return 0;
    }
}

#define PNG_SHAPE(name)                                                                                                                                          \
    PngGeom g;                                                                                                                                                   \
    TG_REQUIRE(F >= 1 && png_geom(H, W, rows_per_block, g), TG_ERR_SHAPE,                                                                                        \
               name ": bad shape F=%d H=%d (1..65535) W=%d (1..21844) rows_per_block=%d (0: the default; a band of rows_per_block (1 + 3 W) bytes is at most 65535)", F, \
               H, W, rows_per_block);                                                                                                                            \
    const long grid_bands = (long)F * g.bands;                                                                                                                  \
    TG_REQUIRE((long)F * H < (1L << 31) && grid_bands < (1L << 31), TG_ERR_SHAPE, name ": too many rows")

extern "C" int tg_png_filter(const void* frames, int F, int H, int W, int filter, int rows_per_block, void* filtered, hipStream_t stream) {
    TG_REQUIRE(frames && filtered, TG_ERR_ARG, "tg_png_filter: null pointer");
    TG_REQUIRE(filter >= 0 && filter <= PNG_ADAPTIVE, TG_ERR_ARG, "tg_png_filter: filter must be 0..4 (none, sub, up, average, paeth) or 5 (adaptive), got %d", filter);
    PNG_SHAPE("tg_png_filter");
    TG_REQUIRE(tg_aligned16(filtered), TG_ERR_ALIGN, "tg_png_filter: filtered must be 16-byte aligned");
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((long)F * H)), dim3(PNG_THREADS), 0, stream, (const uint8_t*)frames, H, W, filter, g.rows, g.bands, g.row, g.stride,
                       (uint8_t*)filtered);
    TG_LAUNCH_CHECK("tg_png_filter");
    return TG_OK;
}

extern "C" int tg_png_band_plan(const void* filtered, int F, int H, int W, int rows_per_block, void* plans, void* band_bytes, hipStream_t stream) {
    TG_REQUIRE(filtered && plans && band_bytes, TG_ERR_ARG, "tg_png_band_plan: null pointer");
    PNG_SHAPE("tg_png_band_plan");
    TG_REQUIRE(tg_aligned16(filtered) && (((uintptr_t)plans | (uintptr_t)band_bytes) & 3) == 0, TG_ERR_ALIGN,
               "tg_png_band_plan: filtered must be 16-byte aligned, plans and band_bytes 4-byte");
    const long lds = g.stride;
    TG_DYN_LDS(png_plan_kernel, 80 * 1024);
    hipLaunchKernelGGL(png_plan_kernel, dim3((unsigned)grid_bands), dim3(PNG_THREADS), (size_t)lds, stream, (const uint8_t*)filtered, H, g.rows, g.bands, g.row, g.stride,
                       (PngPlan*)plans, (int32_t*)band_bytes);
    TG_LAUNCH_CHECK("tg_png_band_plan");
    return TG_OK;
}

extern "C" int tg_png_write(const void* filtered, const void* plans, int F, int H, int W, int rows_per_block, const void* band_offsets, void* data, long data_bytes,
                            hipStream_t stream) {
    TG_REQUIRE(filtered && plans && band_offsets && data, TG_ERR_ARG, "tg_png_write: null pointer");
    PNG_SHAPE("tg_png_write");
    TG_REQUIRE(data_bytes >= (long)F * (PNG_FILE_HEADER + PNG_FILE_TRAILER), TG_ERR_SHAPE, "tg_png_write: %ld bytes cannot hold %d files", data_bytes, F);
    TG_REQUIRE(tg_aligned16(filtered) && ((uintptr_t)plans & 3) == 0 && ((uintptr_t)band_offsets & 7) == 0, TG_ERR_ALIGN,
               "tg_png_write: filtered must be 16-byte aligned, plans 4-byte, band_offsets 8-byte");
    PngFileHeader head;
    file_header(H, W, head);
    const long chunk_lds = png_chunk_lds(g);
    TG_DYN_LDS(png_write_kernel, 144 * 1024);
    hipLaunchKernelGGL(png_write_kernel, dim3((unsigned)grid_bands), dim3(PNG_THREADS), (size_t)(g.stride + chunk_lds), stream, (const uint8_t*)filtered,
                       (const PngPlan*)plans, H, g.rows, g.bands, g.row, g.stride, g.stride, chunk_lds, head, (const long long*)band_offsets, (uint8_t*)data, data_bytes);
    TG_LAUNCH_CHECK("tg_png_write");
    return TG_OK;
}
