// resize_plan_pin: prints what csrc/resize_plan.h plans, for tests/test_resize_cpu.py to compare with the numpy restatement (tests/resize_ref.py).
//   resize_plan_pin plans  < "w h W H" lines  -> per line, binary: int32 mode, int32 xofs[W], int16 ialpha[W][2], int32 yofs[H], int16 ibeta[H][2]
//   resize_plan_pin resize w h W H < h * w source bytes -> H * W bytes: the spec's arithmetic read off the plan's tables, pixel by pixel
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "../../omni-swarm_amd/csrc/resize_plan.h"

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "plans")) {
        int w, h, W, H;
        while (std::scanf("%d %d %d %d", &w, &h, &W, &H) == 4) {
            const omni::ResizePlan p = omni::resize_plan(w, h, W, H);
            const int32_t mode = p.mode;
            std::fwrite(&mode, 4, 1, stdout);
            std::fwrite(p.xofs.data(), 4, p.xofs.size(), stdout);
            std::fwrite(p.ialpha.data(), 2, p.ialpha.size(), stdout);
            std::fwrite(p.yofs.data(), 4, p.yofs.size(), stdout);
            std::fwrite(p.ibeta.data(), 2, p.ibeta.size(), stdout);
        }
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "resize")) {
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), W = std::atoi(argv[4]), H = std::atoi(argv[5]);
        std::vector<uint8_t> src((size_t)w * h), dst((size_t)W * H);
        if (std::fread(src.data(), 1, src.size(), stdin) != src.size()) return 2;
        const omni::ResizePlan p = omni::resize_plan(w, h, W, H);
        auto at = [&](int y, int x) { return (int)src[(size_t)y * w + x]; };
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int v;
                if (p.mode == omni::RESIZE_COPY) v = at(y, x);
                else if (p.mode == omni::RESIZE_AREA2) v = (at(2 * y, 2 * x) + at(2 * y, 2 * x + 1) + at(2 * y + 1, 2 * x) + at(2 * y + 1, 2 * x + 1) + 2) >> 2;
                else {
                    const int x0 = p.xofs[x], x1 = std::min(x0 + 1, w - 1), a0 = p.ialpha[2 * x], a1 = p.ialpha[2 * x + 1];
                    const int y0 = std::min(std::max(p.yofs[y], 0), h - 1), y1 = std::min(std::max(p.yofs[y] + 1, 0), h - 1), b0 = p.ibeta[2 * y], b1 = p.ibeta[2 * y + 1];
                    const int R0 = at(y0, x0) * a0 + at(y0, x1) * a1, R1 = at(y1, x0) * a0 + at(y1, x1) * a1;
                    v = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2;
                }
                dst[(size_t)y * W + x] = (uint8_t)v;
            }
        std::fwrite(dst.data(), 1, dst.size(), stdout);
        return 0;
    }
    return 1;
}
