// Host program around tokensgen_amd/csrc/jpeg_entropy_dec.h, the entropy decoder that csrc/jpeg_decode.hip runs one lane per restart segment: the same inline code,
// compiled by g++ with the address and undefined-behaviour sanitizers (tests/test_jpeg_decode_cpu.py builds and runs it).  It shows, before the code runs on a
// GPU, that the bit reader stays inside its segment for valid and for damaged streams alike.
//
//   jpeg_entropy_host JOBS
// JOBS (little endian): u32 number of jobs, then per job: u32 blocks per MCU (3 or 6), u32 MCUs, u32 print (1: the coefficients follow the status line); six tables
// (component c's DC at 2 c, AC at 2 c + 1), each 16 bytes BITS, u32 n, n bytes HUFFVAL; u32 segment bytes, the segment.  The segment is copied into a heap block of
// exactly its size, so a read one byte past it is an error the sanitizer reports.  Output per job: "table T C" for a refused table (C: jd_build_table's code) or
// "status S" and, with print, one line of 64 coefficients per block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy_dec.h"

namespace {

struct Input {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    bool take(void* dst, size_t n) {
        if (n > buf.size() - pos) return false;
        if (n) memcpy(dst, buf.data() + pos, n);
        pos += n;
        return true;
    }
    bool u32(uint32_t& v) {
        uint8_t b[4];
        if (!take(b, 4)) return false;
        v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
        return true;
    }
};

int fail(const char* what) {
    fprintf(stderr, "jpeg_entropy_host: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: jpeg_entropy_host JOBS");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return fail("cannot open the jobs file");
    Input in;
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, fh)) > 0;) in.buf.insert(in.buf.end(), chunk, chunk + n);
    fclose(fh);
    uint32_t jobs;
    if (!in.u32(jobs)) return fail("no job count");
    for (uint32_t j = 0; j < jobs; ++j) {
        uint32_t bpm, mcus, print;
        if (!in.u32(bpm) || !in.u32(mcus) || !in.u32(print) || (bpm != 3 && bpm != 6) || mcus < 1 || mcus > (1u << 20)) return fail("bad job header");
        JdHuffTable tabs[JD_TABLES_PER_SET];
        int refused = -1, code = 0;
        for (int t = 0; t < JD_TABLES_PER_SET; ++t) {
            uint8_t bits[16];
            uint32_t n;
            if (!in.take(bits, 16) || !in.u32(n) || n > 4096) return fail("bad table");
            std::vector<uint8_t> vals(n ? n : 1);
            if (!in.take(vals.data(), n)) return fail("bad table values");
            const int r = jd_build_table(bits, vals.data(), (int)n, &tabs[t]);
            if (r && refused < 0) {
                refused = t;
                code = r;
            }
        }
        uint32_t bytes;
        if (!in.u32(bytes)) return fail("no segment length");
        uint8_t* seg = (uint8_t*)malloc(bytes ? bytes : 1);                        // exactly the segment: the sanitizer sees the first byte past it
        if (!seg || !in.take(seg, bytes)) return fail("bad segment");
        if (refused >= 0) {
            printf("table %d %d\n", refused, code);
            free(seg);
            continue;
        }
        const size_t n_coef = (size_t)mcus * bpm * 64;
        int16_t* coef = (int16_t*)aligned_alloc(16, n_coef * sizeof(int16_t));
        if (!coef) return fail("no memory");
        memset(coef, 0x5a, n_coef * sizeof(int16_t));                              // the decoder writes every coefficient: none of this survives
        const int status = jd_decode_segment(seg, seg + bytes, tabs, (int)bpm, (long)mcus, coef);
        printf("status %d\n", status);
        if (print)
            for (size_t b = 0; b < n_coef / 64; ++b) {
                for (int i = 0; i < 64; ++i) printf(i ? " %d" : "%d", coef[b * 64 + i]);
                printf("\n");
            }
        for (size_t i = 0; i < n_coef; ++i)
            if (coef[i] == 0x5a5a) {                                               // 23130: no decoded value of these tests; after an error the rest is zero
                free(coef);
                free(seg);
                return fail("a coefficient was left unwritten");
            }
        free(coef);
        free(seg);
    }
    return 0;
}
