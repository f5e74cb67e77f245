// The host twin of the JPEG decode (csrc/jpeg_core.h) over seeded damage, for a run under AddressSanitizer and UBSan:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I chessboard-vision_amd/csrc \
//         tools/jpeg_fuzz_host.cpp -o jpeg_fuzz_host && ./jpeg_fuzz_host 600 good0.jpg good1.jpg ...
//
// Every good stream is decoded as it is, then N times with a damage drawn from a fixed generator: bytes overwritten, bits
// flipped, a span removed or doubled, the stream cut short, the header hit as well as the entropy data.  Every buffer is
// allocated at its exact size, so a read or write outside it stops the program; a header the parser refuses is a pass.
// Needs no GPU and no HIP.  tests/test_jpeg_host.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "jpeg_core.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

// returns 1 when the stream decoded (whatever its status), 0 when the header was refused
static int decode_once(const std::vector<uint8_t>& in, int* status)
{
    // an exact-size copy: the decode may not read one byte past the stream
    uint8_t* d = (uint8_t*)malloc(in.size() ? in.size() : 1);
    memcpy(d, in.data(), in.size());
    JpegDesc D;
    JpegTables T;
    char msg[200];
    int ok = 0;
    if (jpeg_parse_header(d, in.size(), &D, &T, msg, sizeof(msg)) == JP_OK && (uint64_t)D.w * D.h <= (1u << 22)) {
        std::vector<int16_t> coef(D.plane_total);
        std::vector<uint8_t> planes(D.plane_total);
        std::vector<uint8_t> bgr((size_t)D.w * D.h * 3);
        jpeg_decode_host(d, D, T, coef.data(), planes.data(), bgr.data(), (size_t)D.w * 3, status);
        ok = 1;
    }
    free(d);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s COUNT good.jpg...\n", argv[0]);
        return 2;
    }
    const int count = atoi(argv[1]);
    long total = 0, decoded = 0, flagged = 0;
    for (int a = 2; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> good;
        uint8_t buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) good.insert(good.end(), buf, buf + n);
        fclose(f);
        int st = -1;
        if (!decode_once(good, &st) || st != 0) {
            fprintf(stderr, "%s: the undamaged stream does not decode cleanly (status %d)\n", argv[a], st);
            return 1;
        }
        JpegDesc D;
        JpegTables T;
        char msg[200];
        jpeg_parse_header(good.data(), good.size(), &D, &T, msg, sizeof(msg));
        for (int i = 0; i < count; i++) {
            std::vector<uint8_t> d = good;
            // three in four damages hit the entropy data only, the rest the whole stream
            const size_t lo = (rnd() & 3) ? D.ent_off : 0;
            const size_t span = d.size() - lo;
            const int kind = (int)(rnd() % 6);
            const size_t at = lo + rnd() % span;
            if (kind == 0) d.resize(at);                                                     // cut short
            else if (kind == 1) d[at] ^= (uint8_t)(1u << (rnd() & 7));                       // one bit
            else if (kind == 2) for (int k = 0; k < 1 + (int)(rnd() % 8) && at + k < d.size(); k++) d[at + k] = (uint8_t)rnd(); // a few bytes
            else if (kind == 3) d[at] = 0xFF;                                                // a stray marker prefix
            else if (kind == 4) {                                                            // a span removed
                size_t len = rnd() % 64;
                if (len > d.size() - at) len = d.size() - at;
                d.erase(d.begin() + at, d.begin() + at + len);
            } else {                                                                         // a span doubled
                const size_t len = d.size() - at < 32 ? d.size() - at : 32;
                const std::vector<uint8_t> copy(d.begin() + at, d.begin() + at + len);
                d.insert(d.begin() + at, copy.begin(), copy.end());
            }
            if (kind == 2 && (rnd() & 1) && at + 1 < d.size()) { // ... or a restart marker where none belongs
                d[at] = 0xFF;
                d[at + 1] = (uint8_t)(0xD0 + (rnd() & 7));
            }
            st = 0;
            total++;
            if (decode_once(d, &st)) {
                decoded++;
                if (st) flagged++;
            }
        }
    }
    printf("%ld damaged streams, %ld decoded, %ld of them with a status\n", total, decoded, flagged);
    return 0;
}
