// The piece path over restart intervals (csrc/jpeg_core.h, jpeg_decode_pieces_host with segments; include/cbv.h,
// CBV_JPEG_ENTROPY_SEGMENTS) against the serial twin over seeded damage, for a run under AddressSanitizer and UBSan:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I chessboard-vision_amd/csrc \
//         tools/jpeg_segments_fuzz_host.cpp -o jpeg_segments_fuzz_host && \
//         ./jpeg_segments_fuzz_host 600 dri0.jpg dri1.jpg ... [--fixed damaged0.jpg damaged1.jpg ...]
//
// The damages are tools/jpeg_fuzz_host.cpp's, from the same generator, and the streams keep their DRI segment: markers
// go missing, appear where none belongs and change their numbers, intervals are cut, emptied and doubled.  Every stream the
// parser accepts is decoded by interval and by segments with pieces of 4, 16 and 128 bytes: coefficients, planes, BGR and
// status must be equal, pieces = the sum of the intervals' piece counts, 1 <= rounds <= the longest interval's pieces and
// intervals <= settled in round 0 <= pieces.  Every buffer is allocated at its exact size, so a read or write outside it
// stops the program.  The streams behind --fixed are decoded as they are, once each, with the same comparison at the same
// three sizes and whatever their status: the fixed damaged streams of the tests pass through here before any of them is
// given to the GPU.  Needs no GPU and no HIP.  tests/test_jpeg_segments_host.py builds and runs it.
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

static long g_mismatch = 0, g_rounds = 0, g_pieces = 0, g_with_dri = 0;

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
        std::vector<int16_t> coef(D.plane_total), coef2(D.plane_total);
        std::vector<uint8_t> planes(D.plane_total), planes2(D.plane_total);
        std::vector<uint8_t> bgr((size_t)D.w * D.h * 3), bgr2((size_t)D.w * D.h * 3);
        jpeg_decode_host(d, D, T, coef.data(), planes.data(), bgr.data(), (size_t)D.w * 3, status);
        // what the figures must be: the intervals' bytes as the markers found bound them
        std::vector<uint32_t> mpos;
        int ignored = 0;
        jpeg_find_restarts_host(d, D, &mpos, &ignored);
        if (D.dri) g_with_dri++;
        static const uint32_t sizes[3] = {4, 16, 128};
        for (uint32_t S : sizes) {
            uint32_t want = 0, longest = 1;
            for (int iv = 0; iv < D.nint; iv++) {
                uint32_t a, b;
                jpeg_interval_bytes(D, mpos.data(), (int)mpos.size(), iv, &a, &b);
                const uint32_t n = jpeg_piece_count(b - a, S);
                want += n;
                longest = n > longest ? n : longest;
            }
            int st2 = -1;
            JpegPieceStats ps;
            jpeg_decode_host(d, D, T, coef2.data(), planes2.data(), bgr2.data(), (size_t)D.w * 3, &st2, S, &ps, true);
            bool same = st2 == *status && coef == coef2 && planes == planes2 && bgr == bgr2;
            same = same && ps.pieces == want && ps.rounds >= 1 && ps.rounds <= longest && ps.settled >= (uint32_t)D.nint && ps.settled <= ps.pieces;
            g_rounds += ps.rounds;
            g_pieces += ps.pieces;
            if (!same) {
                if (g_mismatch < 5)
                    fprintf(stderr, "segments with pieces of %u bytes differ from the serial decode: status %d / %d, %u pieces (%u), %u rounds (<= %u), %u settled\n",
                            S, st2, *status, ps.pieces, want, ps.rounds, longest, ps.settled);
                g_mismatch++;
            }
        }
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
    long total = 0, decoded = 0, flagged = 0, fixed = 0, fixed_flagged = 0;
    bool as_they_are = false;
    for (int a = 2; a < argc; a++) {
        if (!strcmp(argv[a], "--fixed")) {
            as_they_are = true;
            continue;
        }
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
        if (as_they_are) {
            if (!decode_once(good, &st)) {
                fprintf(stderr, "%s: the header is refused\n", argv[a]);
                return 1;
            }
            fixed++;
            if (st) fixed_flagged++;
            continue;
        }
        if (!decode_once(good, &st) || st != 0) {
            fprintf(stderr, "%s: the undamaged stream does not decode (status %d)\n", argv[a], st);
            return 1;
        }
        JpegDesc D;
        JpegTables T;
        char msg[200];
        jpeg_parse_header(good.data(), good.size(), &D, &T, msg, sizeof(msg));
        if (!D.dri) {
            fprintf(stderr, "%s: a stream without DRI\n", argv[a]);
            return 2;
        }
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
    printf("%ld damaged streams, %ld decoded, %ld of them with a status, %ld fixed streams, %ld of them with a status, %ld decodes differ; "
           "%ld rounds over %ld pieces; %ld decodes had DRI\n",
           total, decoded, flagged, fixed, fixed_flagged, g_mismatch, g_rounds, g_pieces, g_with_dri);
    return g_mismatch ? 1 : 0;
}
