// jpegdec_plan_pin: csrc/jpeg_dec_plan.h built with g++ alone (tests/test_jpegdec_plan_cpu.py, tests/jpegdec_cases.py) -- also with -fsanitize=address,undefined
// for the mutated files.
//   jpegdec_plan_pin <in> <out>
// in:  int32 n; per case int32 {size, S, max_sub} + the file.  S = 0: jpeg_decode_host; else decode_planned_host with both switches off (one chunk), S bits per subsequence
//      and at most max_sub subsequences (0: no limit)
// out: per case int32 {status, w, h, subsequences, S used, rounds, wrong first-pass exits, has_pixels} + w * h pixels when has_pixels.  The picture is decoded into
//      a buffer of stride w + 3 filled with 0xA5, with a guard row behind it: a byte written outside the picture is exit code 5
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_dec_plan.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 3;
    for (int i = 0; i < n; ++i) {
        int32_t a[3];
        if (fread(a, 4, 3, in) != 3 || a[0] < 0) return 3;
        std::vector<uint8_t> file((size_t)a[0]);
        if (a[0] && fread(file.data(), 1, file.size(), in) != file.size()) return 3;
        int w = 0, h = 0;
        const int cls = omni::jd::jpeg_decode_host(file.data(), (int64_t)file.size(), nullptr, 0, 0, 0, &w, &h);
        const int stride = w + 3;
        std::vector<uint8_t> buf((size_t)stride * (h + 1) + 8, 0xA5);
        omni::jd::PlannedStats ps;
        uint32_t wrong = 0;
        int st = cls;
        const bool pixels = cls != OMNI_JPEGDEC_UNSUPPORTED && w > 0 && h > 0;
        if (pixels) {
            const uint32_t max_sub = a[2] ? (uint32_t)a[2] : 0xffffffffu;
            st = a[1] == 0 ? omni::jd::jpeg_decode_host(file.data(), (int64_t)file.size(), buf.data(), stride, w, h, &w, &h)
                           : omni::jd::decode_planned_host(file.data(), (int64_t)file.size(), (uint32_t)a[1], 0u, 0u, max_sub, buf.data(), stride, w, h, &w, &h, &ps);
            if (st < 0) return 4;
            if (a[1]) wrong = omni::jd::wrong_after_first(file.data(), (int64_t)file.size(), (uint32_t)a[1], max_sub);
            for (int y = 0; y <= h; ++y)
                for (int x = y < h ? w : 0; x < stride; ++x)
                    if (buf[(size_t)y * stride + x] != 0xA5) return 5;
        }
        const int32_t r[8] = {st, w, h, (int32_t)ps.n_sub, (int32_t)ps.subseq_bits, (int32_t)ps.chunk_rounds, (int32_t)wrong, pixels ? 1 : 0};
        fwrite(r, 4, 8, out);
        if (pixels)
            for (int y = 0; y < h; ++y) fwrite(buf.data() + (size_t)y * stride, 1, (size_t)w, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
