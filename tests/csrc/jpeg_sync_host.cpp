// Host program around tokensgen_amd/csrc/jpeg_entropy_sync.h, the self-synchronising entropy decoder that csrc/jpeg_decode_sync.hip runs one lane per subsequence:
// the same inline code, compiled by g++ with the address and undefined-behaviour sanitizers (tests/test_jpeg_sync_cpu.py builds and runs it).  The lanes of a
// workgroup are emulated round by round, as a barrier would order them: in a round every lane first reads its neighbour's exit of the round before, then decodes.
//
//   jpeg_sync_host JOBS
// JOBS (little endian): u32 number of jobs, then per job: u32 blocks per MCU (3 or 6), u32 MCUs, u32 print (1: the coefficients follow), u32 sub_bytes, u32 lanes;
// six tables (component c's DC at 2 c, AC at 2 c + 1), each 16 bytes BITS, u32 n, n bytes HUFFVAL; u32 segment bytes, the segment.  The segment is copied into a heap
// block of exactly its size, and the coefficients into one of exactly the segment's blocks, so a read or a store one byte outside is an error the sanitizer reports.
// Output per job: "clean C rounds R chunks N multi M serial S same E": the verdict, the most rounds a chunk took, the chunks, those with more than one subsequence
// whose rounds were within 1 .. lanes of the chunk (all of them, or the program fails), jd_decode_segment's status and whether the two coefficient arrays are equal;
// with print, one line of 64 coefficients per block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy_sync.h"

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
    fprintf(stderr, "jpeg_sync_host: %s\n", what);
    return 2;
}

struct Verdict { int clean, rounds, chunks, multi; };

// one segment as one workgroup of `lanes` lanes decodes it; false: something a kernel must never do
bool decode_sync(const uint8_t* seg, uint32_t bytes, const JdHuffTable* tabs, int bpm, long n_mcus, int sub_bytes, int lanes, int16_t* coef, Verdict& v) {
    const long n_blocks = n_mcus * bpm;
    for (long i = 0; i < n_blocks * 64; ++i) coef[i] = 0;
    const uint32_t chunk_bytes = (uint32_t)lanes * (uint32_t)sub_bytes;
    const uint32_t n_chunks = (bytes + chunk_bytes - 1) / chunk_bytes;
    const int max_steps = js_max_steps(sub_bytes);
    JsState carry = js_state(0, 0, 0);
    long base = 0;
    v = Verdict{0, 0, (int)n_chunks, 0};
    bool invalid_entry = false;
    std::vector<JsState> entry(lanes), exit(lanes), next(lanes), guess(lanes);
    std::vector<int32_t> started(lanes);
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t c0 = c * chunk_bytes, left = bytes - c0;
        const int n_act = left >= chunk_bytes ? lanes : (int)((left + (uint32_t)sub_bytes - 1) / (uint32_t)sub_bytes);
        auto sub_end = [&](int i) {
            const uint32_t e = c0 + (uint32_t)(i + 1) * (uint32_t)sub_bytes;
            return e < bytes ? e : bytes;
        };
        for (int i = 0; i < n_act; ++i) {
            guess[i] = js_guess(seg, bytes, c0 + (uint32_t)i * (uint32_t)sub_bytes);
            entry[i] = i == 0 ? carry : guess[i];
            exit[i] = js_run<false>(seg, bytes, sub_end(i), max_steps, tabs, bpm, js_effective(entry[i], guess[i]), &started[i], nullptr, 0, 0);
        }
        int rounds = 1;
        for (int r = 1; r < n_act; ++r) {
            for (int i = 1; i < n_act; ++i) next[i] = exit[i - 1];                 // before the barrier
            bool changed = false;
            for (int i = 1; i < n_act; ++i)
                if (!js_same(next[i], entry[i])) {
                    entry[i] = next[i];
                    exit[i] = js_run<false>(seg, bytes, sub_end(i), max_steps, tabs, bpm, js_effective(entry[i], guess[i]), &started[i], nullptr, 0, 0);
                    changed = true;
                }
            if (!changed) break;
            ++rounds;
        }
        for (int i = 1; i < n_act; ++i)
            if (!js_same(entry[i], exit[i - 1])) return false;                     // not a fixed point
        if (n_act > 1) {
            if (rounds < 1 || rounds > n_act) return false;
            ++v.multi;
        }
        v.rounds = rounds > v.rounds ? rounds : v.rounds;
        long before = base;
        for (int i = 0; i < n_act; ++i) {
            int32_t again;
            invalid_entry |= js_how(entry[i]) == JS_INVALID;
            const JsState out = js_run<true>(seg, bytes, sub_end(i), max_steps, tabs, bpm, js_effective(entry[i], guess[i]), &again, coef, before, n_blocks);
            if (!js_same(out, exit[i]) || again != started[i]) return false;      // the write pass is the count pass
            before += started[i];
        }
        carry = exit[n_act - 1];
        base = before;
    }
    int32_t p0 = 0, p1 = 0, p2 = 0;
    js_dc_prefix<true>(coef, bpm, 0, n_mcus, p0, p1, p2);
    v.clean = js_segment_clean(invalid_entry, carry, base, n_blocks) ? 1 : 0;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: jpeg_sync_host JOBS");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return fail("cannot open the jobs file");
    Input in;
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, fh)) > 0;) in.buf.insert(in.buf.end(), chunk, chunk + n);
    fclose(fh);
    uint32_t jobs;
    if (!in.u32(jobs)) return fail("no job count");
    for (uint32_t j = 0; j < jobs; ++j) {
        uint32_t bpm, mcus, print, sub_bytes, lanes;
        if (!in.u32(bpm) || !in.u32(mcus) || !in.u32(print) || !in.u32(sub_bytes) || !in.u32(lanes) || (bpm != 3 && bpm != 6) || mcus < 1 || mcus > (1u << 20) ||
            sub_bytes < 16 || sub_bytes > 256 || (sub_bytes & (sub_bytes - 1)) || lanes < 1 || lanes > 1024)
            return fail("bad job header");
        JdHuffTable tabs[JD_TABLES_PER_SET];
        for (int t = 0; t < JD_TABLES_PER_SET; ++t) {
            uint8_t bits[16];
            uint32_t n;
            if (!in.take(bits, 16) || !in.u32(n) || n > 4096) return fail("bad table");
            std::vector<uint8_t> vals(n ? n : 1);
            if (!in.take(vals.data(), n)) return fail("bad table values");
            if (jd_build_table(bits, vals.data(), (int)n, &tabs[t])) return fail("a refused table");
        }
        uint32_t bytes;
        if (!in.u32(bytes) || bytes > JS_MAX_SEGMENT_BYTES) return fail("no segment length");
        uint8_t* seg = (uint8_t*)malloc(bytes ? bytes : 1);                        // exactly the segment: the sanitizer sees the first byte past it
        if (!seg || !in.take(seg, bytes)) return fail("bad segment");
        const size_t n_coef = (size_t)mcus * bpm * 64;
        int16_t* coef = (int16_t*)aligned_alloc(16, n_coef * sizeof(int16_t));     // exactly the segment's blocks
        int16_t* serial = (int16_t*)aligned_alloc(16, n_coef * sizeof(int16_t));
        if (!coef || !serial) return fail("no memory");
        memset(coef, 0x5a, n_coef * sizeof(int16_t));
        Verdict v;
        if (!decode_sync(seg, bytes, tabs, (int)bpm, (long)mcus, (int)sub_bytes, (int)lanes, coef, v)) return fail("no fixed point, rounds out of bounds or a write pass that differs");
        const int status = jd_decode_segment(seg, seg + bytes, tabs, (int)bpm, (long)mcus, serial);
        printf("clean %d rounds %d chunks %d multi %d serial %d same %d\n", v.clean, v.rounds, v.chunks, v.multi, status,
               memcmp(coef, serial, n_coef * sizeof(int16_t)) == 0 ? 1 : 0);
        if (print)
            for (size_t b = 0; b < n_coef / 64; ++b) {
                for (int i = 0; i < 64; ++i) printf(i ? " %d" : "%d", coef[b * 64 + i]);
                printf("\n");
            }
        free(coef);
        free(serial);
        free(seg);
    }
    return 0;
}
