// Pins omni-swarm_amd/csrc/depth_plan.h (the arithmetic of the GPU depth-landmark stage, csrc/depth_landmarks.hip) to the host functions it restates:
// omni::fill_image_descriptor's lifted floats and omni::fill_depth_landmarks (host/loop_geometry.hpp) with omni::CameraModel::lift (host/camera_model.hpp).
// Built with plain g++, ASan + UBSan (tests/depth_cases.py); the C-ABI and GPU tests use the `host` mode's output as the expectation.
//
//   depth_plan_pin plan   the header (dp::depth_landmarks_host) on the case's arrays
//   depth_plan_pin host   the two host functions, image by image, on the same arrays: an image whose have flag is 0 gets fill_image_descriptor alone (what
//                         KeyframePipeline::finish() leaves when a key frame came without a depth image); a raw key-point count outside [0, max_num] is
//                         clamped before the call (the message of a unit never holds more than max_num key points)
//
// stdin, repeated until EOF (binary, native endianness): int32 n_images, max_num, depth_stride (elements), 0; omni_depth_model; omni_camera_model;
//   poses7 [n_images][7] f64; kps_xy [n_images][max_num][2] f32; n_kps [n_images] i32; have [n_images] u8; depth [n_images][depth_height][depth_stride] u16
// stdout per case: norm2d [n_images][max_num][2] f32; landmarks_3d [n_images][max_num][3] f32; flag [n_images][max_num] u8; count_3d [n_images] i32
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/depth_plan.h"
#include "../../omni-swarm_amd/host/camera_model.hpp"
#include "../../omni-swarm_amd/host/loop_geometry.hpp"

using namespace omni;

struct Case {
    int n_images = 0, max_num = 0, stride = 0;
    omni_depth_model m;
    omni_camera_model cm;
    std::vector<double> poses;
    std::vector<float> kps;
    std::vector<int> n_kps;
    std::vector<uint8_t> have;
    std::vector<uint16_t> depth;
};

template <typename T> static bool get(std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, stdin) == n; }
template <typename T> static void put(const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), stdout); }

static int read_case(Case& c) {                  // 1: a case, 0: clean end of input, -1: truncated
    int hdr[4];
    const size_t got = fread(hdr, sizeof(int), 4, stdin);
    if (got == 0) return 0;
    if (got != 4) return -1;
    c.n_images = hdr[0]; c.max_num = hdr[1]; c.stride = hdr[2];
    if (c.n_images < 1 || c.max_num < 1) return -1;
    if (fread(&c.m, sizeof(c.m), 1, stdin) != 1 || fread(&c.cm, sizeof(c.cm), 1, stdin) != 1) return -1;
    if (dp::check_model(c.m) || cam::check(c.cm) || dp::check_sizes(c.m, c.n_images, c.max_num, c.stride)) return -1;
    const size_t N = (size_t)c.n_images, M = (size_t)c.max_num;
    return get(c.poses, N * 7) && get(c.kps, N * M * 2) && get(c.n_kps, N) && get(c.have, N) && get(c.depth, N * c.m.depth_height * c.stride) ? 1 : -1;
}

static PoseMsg msg7(const double* v) {
    PoseMsg m;
    for (int i = 0; i < 3; ++i) m.position[i] = v[i];
    for (int i = 0; i < 4; ++i) m.quat_wxyz[i] = v[3 + i];
    return m;
}

int main(int argc, char** argv) {
    if (argc != 2 || (strcmp(argv[1], "plan") && strcmp(argv[1], "host"))) { fprintf(stderr, "usage: depth_plan_pin plan|host < cases\n"); return 2; }
    const bool plan = !strcmp(argv[1], "plan");
    Case c;
    int rc;
    while ((rc = read_case(c)) == 1) {
        const size_t N = (size_t)c.n_images, M = (size_t)c.max_num;
        std::vector<float> norm(N * M * 2, 0.f), l3d(N * M * 3, 0.f);
        std::vector<uint8_t> flag(N * M, 0);
        std::vector<int> count(N, 0);
        if (plan) {
            dp::depth_landmarks_host(c.m, c.cm, c.poses.data(), c.n_images, c.max_num, c.kps.data(), c.n_kps.data(), c.depth.data(), c.stride, c.have.data(), norm.data(),
                                     l3d.data(), flag.data(), count.data());
        } else {
            CameraModel camera;
            camera.model = c.cm; camera.fx = c.m.fx; camera.fy = c.m.fy; camera.cx = c.m.cx; camera.cy = c.m.cy;
            const std::function<geom::Vec2(const Point2f&)> lift = [&camera](const Point2f& p) { return camera.lift(p); };
            for (size_t i = 0; i < N; ++i) {
                const int n = c.n_kps[i] < 0 ? 0 : (c.n_kps[i] > c.max_num ? c.max_num : c.n_kps[i]);
                ImageDescriptor im;
                fill_image_descriptor(im, c.kps.data() + i * M * 2, n, nullptr, 0, nullptr, 0, lift);
                stamp_image_descriptor(im, 0.0, 0, msg7(c.m.extrinsic), msg7(c.poses.data() + 7 * i), 0);
                if (c.have[i])
                    count[i] = fill_depth_landmarks(im, c.depth.data() + i * c.m.depth_height * c.stride, c.stride, c.m.depth_width, c.m.depth_height, c.m.depth_near, c.m.depth_far,
                                                    c.m.accept_min_3d_pts, lift);
                for (size_t k = 0; k < im.landmarks_2d.size(); ++k) {
                    const size_t at = i * M + k;
                    norm[at * 2] = im.landmarks_2d_norm[k].x; norm[at * 2 + 1] = im.landmarks_2d_norm[k].y;
                    l3d[at * 3] = im.landmarks_3d[k].x; l3d[at * 3 + 1] = im.landmarks_3d[k].y; l3d[at * 3 + 2] = im.landmarks_3d[k].z;
                    flag[at] = im.landmarks_flag[k];
                }
            }
        }
        put(norm); put(l3d); put(flag); put(count);
    }
    if (rc < 0) { fprintf(stderr, "depth_plan_pin: truncated or inconsistent case\n"); return 1; }
    return 0;
}
