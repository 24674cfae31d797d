// jpegdec_restart_pin: the restart-interval path of csrc/jpeg_dec_plan.h -- plan_chunks and decode_planned_host with restart_wgs = W -- built with g++ alone, with
// -fsanitize=address,undefined (tests/test_jpegdec_restart_cpu.py, tests/jpegdec_restart_cases.py), over the fixtures and the mutated files.
//   jpegdec_restart_pin <in> <out>
// in:  int32 n; per case int32 {size, S, W, max_sub} + the file
// out: per case int32 {status, w, h, subsequences, S used, chunks, rounds, the planner's verdict (-1: no restart-only file), has_pixels} + w * h pixels when
//      has_pixels.  The picture is decoded into a buffer of stride w + 3 filled with 0xA5, with a guard row behind it: a byte written outside the picture is exit
//      code 5.  The plan itself is checked here: intervals and chunks tile the scan and the subsequences in order, no chunk above max_sub (exit code 6)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_dec_plan.h"

using namespace omni::jd;

static int check_plan(const Desc& d, const ChunkPlan& P, uint32_t total_bits, uint32_t W, uint32_t max_sub) {
    if (P.status != OMNI_JPEGDEC_OK) return 0;
    if (P.n_chunks < 1 || P.n_chunks > W || P.iv.size() != (size_t)P.n_int + 1 || P.chunk_first.size() != (size_t)P.n_chunks + 1) return 1;
    if (P.chunk_first[0] != 0 || P.chunk_first[P.n_chunks] != P.n_int) return 1;
    uint32_t sub = 0;
    for (uint32_t c = 0; c < P.n_chunks; ++c) {
        if (P.chunk_first[c] >= P.chunk_first[c + 1]) return 1;
        const uint32_t before = sub;
        for (uint32_t k = P.chunk_first[c]; k < P.chunk_first[c + 1]; ++k) {
            const Interval& I = P.iv[k];
            if (I.first_sub != sub || I.bit_begin > I.bit_end || I.bit_end > total_bits || (I.bit_begin & 7) || I.first_block != k * (uint32_t)d.restart * (uint32_t)d.T.bpm) return 1;
            if (k && I.bit_begin != P.iv[k - 1].bit_end) return 1;
            sub += interval_subs(I.bit_end - I.bit_begin, P.subseq_bits);
            for (uint32_t g = I.first_sub; g < sub; ++g)
                if (interval_of(P.iv.data(), P.chunk_first[c], P.chunk_first[c + 1], g) != k) return 1;
        }
        if (sub - before > max_sub) return 1;
    }
    const Interval& E = P.iv[P.n_int];
    return !(sub == P.n_sub && E.first_sub == sub && E.first_block == d.n_blocks && E.bit_begin == total_bits && P.iv[P.n_int - 1].bit_end == total_bits && P.iv[0].bit_begin == 0);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
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
        int plan = -1;
        if (d.restart_only) {                                                               // the planner alone
            std::vector<uint8_t> clean((size_t)d.scan_bytes + JD_SCAN_PAD + 4);
            std::vector<int64_t> rst((size_t)(d.scan_bytes / 2 + 1));
            int64_t n_rst = 0;
            const int64_t nclean = unstuff(file.data() + d.scan_off, d.scan_bytes, clean.data(), rst.data(), (int64_t)rst.size(), &n_rst);
            ChunkPlan P;
            plan_chunks(d, nclean, rst.data(), n_rst, S, W, max_sub, &P);
            if (check_plan(d, P, (uint32_t)(nclean * 8), W, max_sub)) return 6;
            plan = P.status;
        }
        int w = d.w, h = d.h;
        const int stride = w + 3;
        std::vector<uint8_t> buf((size_t)stride * (h + 1) + 8, 0xA5);
        PlannedStats rs;
        int st = cls;
        const bool pixels = cls != OMNI_JPEGDEC_UNSUPPORTED && w > 0 && h > 0;
        if (pixels) {
            st = decode_planned_host(file.data(), (int64_t)file.size(), S, W, 0u, max_sub, buf.data(), stride, w, h, &w, &h, &rs);
            if (st < 0) return 4;
            for (int y = 0; y <= h; ++y)
                for (int x = y < h ? w : 0; x < stride; ++x)
                    if (buf[(size_t)y * stride + x] != 0xA5) return 5;
        }
        const int32_t r[9] = {st, w, h, (int32_t)rs.n_sub, (int32_t)rs.subseq_bits, (int32_t)rs.n_chunks, (int32_t)rs.chunk_rounds, plan, pixels ? 1 : 0};
        fwrite(r, 4, 9, out);
        if (pixels)
            for (int y = 0; y < h; ++y) fwrite(buf.data() + (size_t)y * stride, 1, (size_t)w, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
