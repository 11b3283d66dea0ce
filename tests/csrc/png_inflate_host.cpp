// Host program around tokensgen_amd/csrc/png_inflate.h, the decoder that csrc/png_decode.hip runs per piece: the same inline code with one lane, compiled by g++
// with the address and undefined-behaviour sanitizers (tests/test_png_decode_cpu.py builds and runs it over clean and damaged streams and compares every line with
// tests/png_dec_ref.py).  This is where the decoder's safety on hostile bytes is shown: no damaged stream goes to the GPU that has not passed here.
//
//   png_inflate_host JOBS
// JOBS (little endian): u32 number of jobs, then per job u32 kind (0: the stream route, 1: the chunk route), H, W, bpp, the stream's Adler-32, the number of pieces,
// and per piece u32 n and the n bytes of raw deflate data.  Every piece is copied into a heap block of exactly its size, and the filtered bytes and the pixels go
// into heap blocks of exactly theirs, so a read or a store one byte outside is an error the sanitizer reports.
// Output per job, one line each:
//   inflate   the status after the pieces, and the bytes produced by every piece
//   filtered  the frame's filtered bytes in hex, or - where the status is not 0
//   final     the status after the Adler comparison and the filters
//   rgb       the pixels in hex, or - where the status stopped the decode before the filters
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_inflate.h"

namespace {

int fail(const char* what) {
    fprintf(stderr, "png_inflate_host: %s\n", what);
    return 2;
}

void hex(const char* word, const uint8_t* p, long n) {
    printf("%s ", word);
    for (long i = 0; i < n; ++i) printf("%02x", p[i]);
    if (n == 0) printf("-");
    printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: png_inflate_host JOBS");
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return fail("cannot open the jobs file");
    std::vector<uint8_t> buf;
    uint8_t block[65536];
    for (size_t n; (n = fread(block, 1, sizeof block, fh)) > 0;) buf.insert(buf.end(), block, block + n);
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
    PiTables* tables = (PiTables*)malloc(sizeof(PiTables));
    uint8_t* ring = (uint8_t*)malloc(PI_RING);
    if (!tables || !ring) return fail("no memory");
    for (uint32_t j = 0; j < jobs; ++j) {
        uint32_t kind, H, W, bpp, expect, pieces;
        if (!u32(kind) || !u32(H) || !u32(W) || !u32(bpp) || !u32(expect) || !u32(pieces) || kind > 1 || pieces < 1 || (bpp != 3 && bpp != 4) || H < 1 || W < 1)
            return fail("bad job");
        const long cap = (long)H * (1 + (long)bpp * W);
        std::vector<uint8_t*> data(pieces);
        std::vector<uint32_t> bytes(pieces);
        for (uint32_t k = 0; k < pieces; ++k) {
            if (!u32(bytes[k]) || buf.size() - pos < bytes[k]) return fail("bad piece");
            data[k] = (uint8_t*)malloc(bytes[k] ? bytes[k] : 1);
            if (!data[k]) return fail("no memory");
            memcpy(data[k], buf.data() + pos, bytes[k]);
            pos += bytes[k];
        }
        uint8_t* filtered = (uint8_t*)calloc((size_t)cap, 1);
        uint8_t* rgb = (uint8_t*)calloc((size_t)H * W * 3, 1);
        std::vector<uint32_t> adler3(3 * (size_t)pieces);
        std::vector<long> produced(pieces);
        if (!filtered || !rgb) return fail("no memory");
        int status = 0;
        if (kind == 0) {
            if (pieces != 1) return fail("the stream route has one piece");
            status = pi_inflate<PiSerial>(data[0], 0, bytes[0], PI_STREAM, true, tables, ring, filtered, 0, cap, &produced[0], &adler3[0]);
        } else {
            long at = 0;
            std::vector<long> start(pieces);
            for (uint32_t k = 0; k < pieces; ++k) {                             // the size pass touches neither the ring nor the output
                status |= pi_inflate<PiSerial>(data[k], 0, bytes[k], PI_CHUNK_SIZE, k + 1 == pieces, tables, nullptr, nullptr, 0, cap, &produced[k], nullptr);
                start[k] = at;
                at += produced[k];
            }
            for (uint32_t k = 0; k < pieces; ++k)
                status |= pi_inflate<PiSerial>(data[k], 0, bytes[k], PI_CHUNK_WRITE, k + 1 == pieces, tables, ring, filtered, start[k], cap, &produced[k], &adler3[3 * k]);
        }
        printf("inflate %d", status);
        for (uint32_t k = 0; k < pieces; ++k) printf(" %ld", produced[k]);
        printf("\n");
        hex("filtered", filtered, status ? 0 : cap);
        bool filters = false;
        if (!status) {
            if (pi_adler_of(adler3.data(), (int)pieces) != expect) status = PI_BAD_ADLER;
            else {
                status = pi_unfilter_frame(filtered, (int)H, (int)W, (int)bpp, rgb);
                filters = true;
            }
        }
        printf("final %d\n", status);
        hex("rgb", rgb, filters ? (long)H * W * 3 : 0);
        free(rgb);
        free(filtered);
        for (uint8_t* p : data) free(p);
    }
    free(ring);
    free(tables);
    return 0;
}
