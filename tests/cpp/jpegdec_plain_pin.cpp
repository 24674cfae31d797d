// jpegdec_plain_pin: the path of csrc/jpeg_dec_plan.h that spreads a file WITHOUT a restart interval over several workgroups -- plain_subseq_bits, plain_chunks,
// plain_chunk_begin and decode_planned_host with plain_wgs = W -- built with g++ alone, with -fsanitize=address,undefined (tests/test_jpegdec_plain_cpu.py,
// tests/jpegdec_plain_cases.py), over the fixtures and the mutated files.
//   jpegdec_plain_pin <in> <out>
// in:  int32 n; per case int32 {size, S, W, max_sub} + the file
// out: per case int32 {status, w, h, subsequences, S used, chunks, chunk rounds, seam rounds, seam changed, seam chunks, has_pixels} + w * h pixels when
//      has_pixels.  The picture is decoded into a buffer of stride w + 3 filled with 0xA5, with a guard row behind it: a byte written outside the picture is exit
//      code 5.  The partition is checked here, for the case's own (subsequences, W) and for a sweep of both: chunks cover [0, n_sub) without gap or overlap, none
//      is empty, none is above max_sub once S obeys plain_subseq_bits (exit code 6)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_dec_plan.h"

using namespace omni::jd;

static int check_partition(uint32_t n_sub, uint32_t W, uint32_t max_sub) {
    const uint32_t C = plain_chunks(n_sub, W);
    if (C < 1 || C > (W ? W : 1u) || (n_sub && C > n_sub)) return 1;
    if (plain_chunk_begin(0, n_sub, C) != 0 || plain_chunk_begin(C, n_sub, C) != n_sub) return 1;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t lo = plain_chunk_begin(c, n_sub, C), hi = plain_chunk_begin(c + 1, n_sub, C);
        if (n_sub && (lo >= hi || hi > n_sub)) return 1;                                    // empty, or out of order
        if (hi - lo > max_sub) return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    // the partition and the S rule on their own: every total up to a few thousand bits and some large ones, W 1..64, small and real workgroups
    for (uint32_t max_sub : {1u, 7u, 8u, 4096u})
        for (uint32_t W = 1; W <= JD_MAX_PLAIN_WGS; ++W)
            for (uint32_t bits = 0; bits < 70000000u; bits = bits < 3000u ? bits + 1 : bits * 2 + 12345u) {
                const uint32_t S = plain_subseq_bits(bits, 128u, W, max_sub), n_sub = (bits + S - 1) / S;
                if (S < 128u || (S & (S - 1)) || (uint64_t)n_sub > (uint64_t)W * max_sub) return 6;
                if (S > 128u && (bits + S / 2 - 1) / (S / 2) <= W * max_sub) return 6;      // doubled once too often
                if (check_partition(n_sub, W, max_sub)) return 6;
            }
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 3;
    for (int i = 0; i < n; ++i) {
        int32_t a[4];
        if (fread(a, 4, 4, in) != 4 || a[0] < 0 || a[2] < 1 || a[3] < 1) return 3;
        std::vector<uint8_t> file((size_t)a[0]);
        if (a[0] && fread(file.data(), 1, file.size(), in) != file.size()) return 3;
        const uint32_t S = (uint32_t)a[1], W = (uint32_t)a[2], max_sub = (uint32_t)a[3];
        Desc d;
        const int cls = parse(file.data(), (int64_t)file.size(), &d);
        int w = d.w, h = d.h;
        const int stride = w + 3;
        std::vector<uint8_t> buf((size_t)stride * (h + 1) + 8, 0xA5);
        PlannedStats ps;
        int st = cls;
        const bool pixels = cls != OMNI_JPEGDEC_UNSUPPORTED && w > 0 && h > 0;
        if (pixels) {
            st = decode_planned_host(file.data(), (int64_t)file.size(), S, 0u, W, max_sub, buf.data(), stride, w, h, &w, &h, &ps);
            if (st < 0) return 4;
            for (int y = 0; y <= h; ++y)
                for (int x = y < h ? w : 0; x < stride; ++x)
                    if (buf[(size_t)y * stride + x] != 0xA5) return 5;
            if (cls == OMNI_JPEGDEC_OK && (check_partition(ps.n_sub, W, max_sub) || ps.n_chunks != plain_chunks(ps.n_sub, W))) return 6;
        }
        const int32_t r[11] = {st, w, h, (int32_t)ps.n_sub, (int32_t)ps.subseq_bits, (int32_t)ps.n_chunks, (int32_t)ps.chunk_rounds, (int32_t)ps.seam_rounds,
                               (int32_t)ps.seam_changed, (int32_t)ps.seam_chunks, pixels ? 1 : 0};
        fwrite(r, 4, 11, out);
        if (pixels)
            for (int y = 0; y < h; ++y) fwrite(buf.data() + (size_t)y * stride, 1, (size_t)w, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
