// Host program around tokensgen_amd/csrc/png_deflate.h, the deflate pieces that csrc/png.hip runs per band: the same inline code, compiled by g++ with the address
// and undefined-behaviour sanitizers (tests/test_png_cpu.py builds and runs it and compares every line with tests/png_ref.py).
//
//   png_deflate_host JOBS
// JOBS (little endian): u32 number of jobs, then per job u32 n (1 .. 65535) and the n bytes of one band.  The band is copied into a heap block of exactly its size and
// the output goes into a heap block of exactly the size that the plan announces, so a read or a store one byte past either is an error the sanitizer reports.
// Output per job, one line each:
//   tokens   L<v> for a literal, M<n> for a match, in order
//   ll       the 286 literal/length code lengths
//   cl       the 19 code lengths of the code-length alphabet
//   plan     header bits, token bits, bytes of the dynamic form, 1 if the stored form is chosen
//   bytes    the band's deflate bytes in hex
//   sums     the CRC-32 and the Adler-32 of the band, each put together from three parts by pd_crc_shift / pd_crc_mulmod and pd_adler_combine
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_deflate.h"

namespace {

int fail(const char* what) {
    fprintf(stderr, "png_deflate_host: %s\n", what);
    return 2;
}

void adler_part(const uint8_t* p, uint32_t n, uint32_t& A, uint32_t& B) {
    uint64_t sum = 0, weighted = 0;
    for (uint32_t i = 0; i < n; ++i) {
        sum += p[i];
        weighted += (uint64_t)(n - i) * p[i];
    }
    pd_adler_pair(sum, weighted, n, A, B);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: png_deflate_host JOBS");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return fail("cannot open the jobs file");
    std::vector<uint8_t> buf;
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, fh)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
    fclose(fh);
    size_t pos = 0;
    auto u32 = [&](uint32_t& v) {
        if (buf.size() - pos < 4) return false;
        v = (uint32_t)buf[pos] | (uint32_t)buf[pos + 1] << 8 | (uint32_t)buf[pos + 2] << 16 | (uint32_t)buf[pos + 3] << 24;
        pos += 4;
        return true;
    };
    uint32_t jobs;
    if (!u32(jobs)) return fail("no job count");
    PdTree* tree = (PdTree*)malloc(sizeof(PdTree));
    PdBandPlan* plan = (PdBandPlan*)malloc(sizeof(PdBandPlan));
    if (!tree || !plan) return fail("no memory");
    for (uint32_t j = 0; j < jobs; ++j) {
        uint32_t n;
        if (!u32(n) || n < 1 || n > (uint32_t)PD_MAX_BAND || buf.size() - pos < n) return fail("bad job");
        uint8_t* d = (uint8_t*)malloc(n);
        if (!d) return fail("no memory");
        memcpy(d, buf.data() + pos, n);
        pos += n;
        printf("tokens");
        pd_for_runs(d, (int)n, [&](int v, int L) {
            int lits, n258, rem;
            pd_run_split(L, lits, n258, rem);
            printf(" L%d", v);
            for (int i = 0; i < n258; ++i) printf(" M258");
            if (rem) printf(" M%d", rem);
            for (int i = 1; i < lits; ++i) printf(" L%d", v);
        });
        pd_band_plan(d, (int)n, plan, tree);
        printf("\nll");
        for (int s = 0; s < PD_LL_SYMBOLS; ++s) printf(" %d", plan->ll[s]);
        printf("\ncl");
        for (int s = 0; s < PD_CL_SYMBOLS; ++s) printf(" %d", plan->cl[s]);
        printf("\nplan %u %u %u %u\n", plan->header_bits, plan->token_bits, plan->dynamic_bytes, plan->stored);
        const long want = plan->stored ? (long)pd_stored_bytes((int)n) : (long)plan->dynamic_bytes;
        uint8_t* out = (uint8_t*)malloc((size_t)want);
        if (!out) return fail("no memory");
        const long got = pd_band_write(d, (int)n, plan, out, want);
        if (got != want) return fail("the band's bytes are not what its plan announced");
        printf("bytes ");
        for (long i = 0; i < got; ++i) printf("%02x", out[i]);
        const uint32_t n1 = n / 3, n2 = (n - n1) / 2, n3 = n - n1 - n2;
        uint32_t crc = pd_crc32(0, d, n1);
        crc = pd_crc_mulmod(pd_crc_shift(n2), crc) ^ pd_crc32(0, d + n1, n2);
        crc = pd_crc_mulmod(pd_crc_shift(n3), crc) ^ pd_crc32(0, d + n1 + n2, n3);
        uint32_t A = 1, B = 0, A2, B2;
        adler_part(d, n1, A2, B2);
        pd_adler_combine(A, B, A2, B2, n1);
        adler_part(d + n1, n2, A2, B2);
        pd_adler_combine(A, B, A2, B2, n2);
        adler_part(d + n1 + n2, n3, A2, B2);
        pd_adler_combine(A, B, A2, B2, n3);
        printf("\nsums %u %u\n", crc, B << 16 | A);
        free(out);
        free(d);
    }
    free(plan);
    free(tree);
    return 0;
}
