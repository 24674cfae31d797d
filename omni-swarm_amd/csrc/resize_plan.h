// resize_plan.h -- the plan of one image resize: cv::resize(src, dst, cv::Size(W, H)) with the default INTER_LINEAR on a CV_8UC1 image, which both of the
// reference's engines run in front of their networks (superpoint_tensorrt.cpp:123-125, mobilenetvlad_tensorrt.cpp:6-8), restated from OpenCV 3.4's own
// (non-IPP) resize.  OpenCV is un-vendored: PARITY UNPINNED.  Plain host C++ (no HIP): resize.hip uploads the four tables as they
// are and tests/cpp/resize_plan_pin.cpp prints them; nothing else computes a coefficient.
//
// Source w x h, destination W x H:
//   RESIZE_COPY    w == W and h == H.
//   RESIZE_AREA2   w == 2W and h == 2H (OpenCV switches INTER_LINEAR to INTER_AREA there): dst = (the 2 x 2 block's sum + 2) >> 2.
//   RESIZE_LINEAR  otherwise.  Per axis scale = 1.0 / ((double)n_dst / n_src); destination index d reads f = (float)((d + 0.5) * scale - 0.5),
//                  s = floor(f), f -= s (float), c0 = rint((1.f - f) * 2048.f), c1 = rint(f * 2048.f) (half to even) as short.
//                  x axis: s < 0 -> s = 0, (c0, c1) = (2048, 0); s >= w - 1 -> s = w - 1, (2048, 0); the second tap is min(s + 1, w - 1).
//                  y axis: s and the coefficients stay as computed; the two rows are clamp(s, 0, h - 1) and clamp(s + 1, 0, h - 1).
//                  R[y][dx] = src[y][sx] * a0 + src[y][sx + 1] * a1 (int);  dst = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2.
//                  Everything fits 32 bits and the result is always in 0..255.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace omni {

enum ResizeMode { RESIZE_COPY = 0, RESIZE_AREA2 = 1, RESIZE_LINEAR = 2 };
enum { RESIZE_COEF_BITS = 11, RESIZE_COEF_ONE = 1 << RESIZE_COEF_BITS };

struct ResizePlan {
    int mode = RESIZE_COPY;
    int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
    std::vector<int32_t> xofs;       // [W]   first tap's column, clamped into the row
    std::vector<int16_t> ialpha;     // [W][2]
    std::vector<int32_t> yofs;       // [H]   first tap's row as computed: -1 .. h - 1 (clamped where it is read)
    std::vector<int16_t> ibeta;      // [H][2]
};

// one axis: n_src -> n_dst; clamp_x: the x axis' rule (offsets clamped, the border taps' coefficients replaced)
inline void resize_axis(int n_src, int n_dst, bool clamp_x, std::vector<int32_t>& ofs, std::vector<int16_t>& coef) {
    ofs.resize((size_t)n_dst);
    coef.resize((size_t)2 * n_dst);
    const double scale = 1.0 / ((double)n_dst / n_src);
    for (int d = 0; d < n_dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (clamp_x && s < 0) { s = 0; f = 0.f; }
        if (clamp_x && s >= n_src - 1) { s = n_src - 1; f = 0.f; }
        ofs[(size_t)d] = s;
        coef[(size_t)2 * d] = (int16_t)std::nearbyint((1.f - f) * (float)RESIZE_COEF_ONE);      // (round half to even: the default rounding mode)
        coef[(size_t)2 * d + 1] = (int16_t)std::nearbyint(f * (float)RESIZE_COEF_ONE);
    }
}

// The tables are made for every mode (the copy and area-2x kernels do not read them): one shape for the device object and the pin program.
inline ResizePlan resize_plan(int w, int h, int W, int H) {
    ResizePlan p;
    p.src_w = w; p.src_h = h; p.dst_w = W; p.dst_h = H;
    p.mode = (w == W && h == H) ? RESIZE_COPY : (w == 2 * W && h == 2 * H) ? RESIZE_AREA2 : RESIZE_LINEAR;
    resize_axis(w, W, true, p.xofs, p.ialpha);
    resize_axis(h, H, false, p.yofs, p.ibeta);
    return p;
}

}  // namespace omni
