// Prints the frame plan (chessboard-vision_amd/csrc/frame_plan.h) of every cell of DESIGN.md's "Where the frames live":
// four configuration kinds x every input format class and planes mode, for one size and one set of Motion-JPEG settings.
// Host code only: tests/test_frame_plan_host.py builds it with the host compiler under AddressSanitizer and UBSan.
//
//     frame_plan_host W H SLOT_BYTES ENTROPY PIECE_BYTES DEPTH [CS]  one line per cell (CS: the colour space of the YUV cells, 0 .. 3)
//     frame_plan_host --piece-size MODE PIECE_BYTES [...]          what jpeg_piece_size makes of each pair
//     frame_plan_host --bayer-deep W H                             the cells of the Bayer ids with a sample encoding (CBV_BAYER_*), four kinds each
//     frame_plan_host --bayer-neutral BITS                         the neutral table of a developed mosaic, and the encodings BITS goes with
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "frame_plan.h"

int main(int argc, char** argv)
{
    char msg[160];
    if (argc >= 4 && !strcmp(argv[1], "--piece-size")) {
        for (int i = 2; i + 1 < argc; i += 2) {
            uint32_t S = 0;
            int segments = 0;
            const int mode = atoi(argv[i]);
            const uint32_t bytes = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
            const int rc = jpeg_piece_size(mode, bytes, &S, &segments, msg, sizeof(msg));
            if (rc) printf("%d %u refused %d %s\n", mode, bytes, rc, msg);
            else printf("%d %u S=%u seg=%d\n", mode, bytes, S, segments);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--bayer-deep")) { // the cells of the twelve Bayer ids with a sample encoding, four kinds each
        FrameSettings s;
        s.w = atoi(argv[2]);
        s.h = atoi(argv[3]);
        s.max_frames = 4;
        const int layouts[] = {CBV_FMT_BAYER_RGGB, CBV_FMT_BAYER_BGGR, CBV_FMT_BAYER_GRBG, CBV_FMT_BAYER_GBRG};
        const int encs[] = {CBV_BAYER_16, CBV_BAYER_10P, CBV_BAYER_12P};
        for (s.kind = FRAMES_ENHANCE; s.kind <= FRAMES_PROFILE_RAW; s.kind++)
            for (int enc : encs)
                for (int lay : layouts) {
                    s.fmt = lay | enc;
                    FramePlan p;
                    const int rc = frame_plan(s, &p, msg, sizeof(msg));
                    printf("%d %d ", s.kind, s.fmt);
                    if (rc) printf("refused %d %s\n", rc, msg);
                    else
                        printf("bayer=%d enc=%d row=%d frame=%zu source=%d bgr=%d slot=%zu pmode=%d depth=%d\n", (int)raw_fmt_bayer(s.fmt), raw_fmt_enc(s.fmt),
                               bayer_row_bytes(s.fmt, s.w), raw_frame_bytes(s.fmt, s.w, s.h), p.source, (int)p.bgr_ring, p.slot_bytes, p.plane_mode, p.depth);
                }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--bayer-neutral")) { // the neutral table of BITS bits, and which bits go with which encoding
        const int bits = atoi(argv[2]);
        if (bits < 1 || bits > 16) return 2;
        uint8_t* t = (uint8_t*)malloc((size_t)1 << bits);
        bayer_neutral_table(bits, t);
        for (int v = 0; v < (1 << bits); v++) printf("%d%c", t[v], v + 1 == (1 << bits) ? '\n' : ' ');
        free(t);
        for (int enc = 0; enc <= 4; enc++)
            printf("enc=%d known=%d ok=%d default=%d\n", enc, (int)raw_fmt_bayer(CBV_FMT_BAYER_RGGB | enc << 12), (int)bayer_bits_ok(CBV_FMT_BAYER_RGGB | enc << 12, bits),
                   bayer_default_bits(CBV_FMT_BAYER_RGGB | enc << 12));
        return 0;
    }
    if (argc != 7 && argc != 8) {
        fprintf(stderr, "usage: %s W H SLOT_BYTES ENTROPY PIECE_BYTES DEPTH [CS] | --piece-size MODE PIECE_BYTES [...]\n", argv[0]);
        return 2;
    }
    FrameSettings s;
    s.w = atoi(argv[1]);
    s.h = atoi(argv[2]);
    s.max_frames = 4;
    s.jpeg_slot_bytes = (size_t)strtoull(argv[3], nullptr, 10);
    s.entropy = atoi(argv[4]);
    s.piece_bytes = (uint32_t)strtoul(argv[5], nullptr, 10);
    s.depth = atoi(argv[6]);
    const int fmts[] = {CBV_FMT_BGR, CBV_FMT_NV12, CBV_FMT_YUYV, CBV_FMT_BAYER_RGGB, CBV_FMT_MJPEG};
    for (s.kind = FRAMES_ENHANCE; s.kind <= FRAMES_PROFILE_RAW; s.kind++)
        for (int fmt : fmts)
            for (s.planes = CBV_JPEG_PLANES_OFF; s.planes <= CBV_JPEG_PLANES_444; s.planes++) {
                if (fmt != CBV_FMT_MJPEG && s.planes != CBV_JPEG_PLANES_OFF && s.planes != CBV_JPEG_PLANES_444) continue; // (there the mode is only stored)
                s.fmt = fmt;
                s.cs = argc == 8 && raw_fmt_yuv(fmt) ? atoi(argv[7]) : 0;
                FramePlan p;
                const int rc = frame_plan(s, &p, msg, sizeof(msg));
                printf("%d %d %d ", s.kind, s.fmt, s.planes);
                if (rc) printf("refused %d %s\n", rc, msg);
                else
                    printf("source=%d bgr=%d slot=%zu pmode=%d pslot=%zu S=%u seg=%d depth=%d own=%d elems=%zu maxint=%zu cap=%u pwords=%zu swords=%zu\n", p.source,
                           (int)p.bgr_ring, p.slot_bytes, p.plane_mode, p.plane_slot, p.piece_bytes, p.segments, p.depth, (int)p.own_planes, p.frame_elems, p.max_int,
                           p.piece_cap, p.piece_words, p.seg_words);
            }
    return 0;
}
