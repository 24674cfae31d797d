// Pins omni-swarm_amd/csrc/camera_plan.h (the lens model of every lift: camodocal's PINHOLE with distortion and MEI) and what is built on it: the landmark
// stage with a camera (csrc/landmark_plan.h's overloads, what csrc/landmarks.hip runs), the host path (omni::CameraModel::lift through
// fill_image_descriptor + fill_stereo_landmarks), the camodocal file reader and KeyframePipeline::Config's checks.  A stand-alone program: plain g++, calls
// nothing of the GPU library; tests/test_camera_plan_cpu.py also builds it with -fsanitize=address,undefined.  The GPU tests use `plan` as the reference the
// kernel must equal bit for bit.
//
//   camera_plan_pin lift      cam::lift            per record: int32 n, 0; omni_camera_model; fx fy cx cy f64; xy [n][2] f32   -> [n][2] f64
//   camera_plan_pin lmlift    the EARLIER lm::lift(stereo model, x, y) on the same records (the camera is read and ignored)     -> [n][2] f64
//   camera_plan_pin project   cam::project         per record: int32 n, 0; omni_camera_model; fx fy cx cy f64; xyz [n][3] f64  -> [n][2] f64
//   camera_plan_pin plan      lm::landmarks_host with the camera      per case: landmark_plan_pin's case with an omni_camera_model behind the omni_stereo_model;
//   camera_plan_pin host      the host functions with CameraModel::lift         the output is landmark_plan_pin's
//   camera_plan_pin depth     fill_image_descriptor + fill_depth_landmarks with CameraModel::lift (PINHOLE_DEPTH's host path).  Per record: int32 n, width, height,
//                             accept_min_3d_pts; omni_camera_model; fx fy cx cy depth_near depth_far f64; pose_drone7, extrinsic7 f64; kps [n][2] f32; depth
//                             [height][width] u16 -> norm2d [n][2] f32, landmarks_3d [n][3] f32, flag [n] u8, int32 count
//   camera_plan_pin yaml W H  the camodocal text on stdin -> SwarmLoopParams::read_camera_config -> to_pipeline_config for W x H networks: one line
//                             "type k1 k2 p1 p2 xi | fx fy cx cy (file) | image_width image_height | fx fy cx cy (Config)", or "ERROR <message>"
//   camera_plan_pin config    KeyframePipeline::Config's camera checks: prints OK, or FAIL lines
#include <cstdio>
#include <cstring>
#include <iostream>
#include <iterator>
#include <vector>

#include "../../omni-swarm_amd/csrc/landmark_plan.h"
#include "../../omni-swarm_amd/host/camera_model.hpp"
#include "../../omni-swarm_amd/host/keyframe_pipeline.hpp"
#include "../../omni-swarm_amd/host/loop_geometry.hpp"
#include "../../omni-swarm_amd/host/swarm_loop_params.hpp"

using namespace omni;

template <typename T> static bool get(std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, stdin) == n; }
template <typename T> static void put(const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), stdout); }

// ---- lift / lmlift / project ---------------------------------------------------------------------------------------------------------------------------------
static int run_points(const char* mode) {
    const bool proj = !strcmp(mode, "project"), legacy = !strcmp(mode, "lmlift");
    for (;;) {
        int hdr[2];
        const size_t got = fread(hdr, sizeof(int), 2, stdin);
        if (got == 0) return 0;
        omni_camera_model cm;
        double k[4];
        if (got != 2 || hdr[0] < 0 || fread(&cm, sizeof(cm), 1, stdin) != 1 || fread(k, sizeof(double), 4, stdin) != 4) return 1;
        const size_t n = (size_t)hdr[0];
        std::vector<double> out(2 * n);
        if (proj) {
            std::vector<double> X;
            if (!get(X, 3 * n)) return 1;
            for (size_t i = 0; i < n; ++i) cam::project(cm, k[0], k[1], k[2], k[3], X.data() + 3 * i, out.data() + 2 * i);
        } else {
            std::vector<float> xy;
            if (!get(xy, 2 * n)) return 1;
            omni_stereo_model m{};
            m.fx = k[0]; m.fy = k[1]; m.cx = k[2]; m.cy = k[3];
            for (size_t i = 0; i < n; ++i) {
                if (legacy) lm::lift(m, xy[2 * i], xy[2 * i + 1], out.data() + 2 * i);
                else cam::lift(cm, k[0], k[1], k[2], k[3], xy[2 * i], xy[2 * i + 1], out.data() + 2 * i);
            }
        }
        put(out);
    }
}

// ---- plan / host -------------------------------------------------------------------------------------------------------------------------------------------
struct Case {
    int n_pairs = 0, max_num = 0, n_keyframes = 0;
    omni_stereo_model m;
    omni_camera_model cm;
    std::vector<double> poses;
    std::vector<float> kps;
    std::vector<int> n_kps, mu, md, nm;
};

static int read_case(Case& c) {                  // 1: a case, 0: clean end of input, -1: truncated
    int hdr[4];
    const size_t got = fread(hdr, sizeof(int), 4, stdin);
    if (got == 0) return 0;
    if (got != 4) return -1;
    c.n_pairs = hdr[0]; c.max_num = hdr[1]; c.n_keyframes = hdr[2];
    if (c.n_pairs < 1 || c.max_num < 1 || c.n_keyframes < 1) return -1;
    if (fread(&c.m, sizeof(c.m), 1, stdin) != 1 || fread(&c.cm, sizeof(c.cm), 1, stdin) != 1) return -1;
    if (c.m.dirs_per_keyframe < 1 || c.m.dirs_per_keyframe > OMNI_STEREO_MAX_DIRS || c.n_keyframes * c.m.dirs_per_keyframe != c.n_pairs) return -1;
    const size_t P = (size_t)c.n_pairs, M = (size_t)c.max_num;
    return get(c.poses, (size_t)c.n_keyframes * 7) && get(c.kps, 2 * P * M * 2) && get(c.n_kps, 2 * P) && get(c.mu, P * M) && get(c.md, P * M) && get(c.nm, P) ? 1 : -1;
}

static PoseMsg msg7(const double* v) {
    PoseMsg m;
    for (int i = 0; i < 3; ++i) m.position[i] = v[i];
    for (int i = 0; i < 4; ++i) m.quat_wxyz[i] = v[3 + i];
    return m;
}

// the smallest two eigenvalues of one match's D^T D, by the host's own functions: 1 when they are equal
static int host_tie(const geom::Pose& pu, const geom::Pose& pd, geom::Vec2 p0, geom::Vec2 p1) {
    const geom::Mat3 R0t = pu.att.R().T(), R1t = pd.att.R().T();
    const geom::Vec3 c0 = -1.0 * (R0t * pu.pos), c1 = -1.0 * (R1t * pd.pos);
    double P0[3][4], P1[3][4], D[4][4], A[4][4], W[4], V[4][4];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { P0[i][j] = R0t.m[i][j]; P1[i][j] = R1t.m[i][j]; }
    P0[0][3] = c0.x; P0[1][3] = c0.y; P0[2][3] = c0.z; P1[0][3] = c1.x; P1[1][3] = c1.y; P1[2][3] = c1.z;
    for (int j = 0; j < 4; ++j) {
        D[0][j] = p0.x * P0[2][j] - P0[0][j]; D[1][j] = p0.y * P0[2][j] - P0[1][j];
        D[2][j] = p1.x * P1[2][j] - P1[0][j]; D[3][j] = p1.y * P1[2][j] - P1[1][j];
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { A[i][j] = 0; for (int k = 0; k < 4; ++k) A[i][j] += D[k][i] * D[k][j]; }
    geom::jacobi_eigen<4>(A, W, V);
    return W[3] == W[2];
}

static int run_cases(bool plan) {
    Case c;
    int rc;
    while ((rc = read_case(c)) == 1) {
        const size_t P = (size_t)c.n_pairs, M = (size_t)c.max_num;
        std::vector<float> norm(2 * P * M * 2, 0.f), l3d(2 * P * M * 3, 0.f);
        std::vector<uint8_t> flag(2 * P * M, 0);
        std::vector<int> count(P, 0), ties(1, 0);
        if (plan) {
            ties[0] = lm::landmarks_host(c.m, c.cm, c.poses.data(), c.n_pairs, c.max_num, c.kps.data(), c.n_kps.data(), c.mu.data(), c.md.data(), c.nm.data(), norm.data(),
                                         l3d.data(), flag.data(), count.data());
        } else {
            const omni_stereo_model& m = c.m;
            CameraModel camera;
            camera.model = c.cm; camera.fx = m.fx; camera.fy = m.fy; camera.cx = m.cx; camera.cy = m.cy;
            const std::function<geom::Vec2(const Point2f&)> lift = [&camera](const Point2f& p) { return camera.lift(p); };
            for (size_t p = 0; p < P; ++p) {
                const size_t img[2] = {p, P + p};
                const int dir = (int)p % m.dirs_per_keyframe;
                const PoseMsg drone = msg7(c.poses.data() + 7 * (p / m.dirs_per_keyframe));
                ImageDescriptor im[2];
                for (int s = 0; s < 2; ++s) {
                    fill_image_descriptor(im[s], c.kps.data() + img[s] * M * 2, c.n_kps[img[s]], nullptr, 0, nullptr, 0, lift);
                    stamp_image_descriptor(im[s], 0.0, 0, msg7(s == 0 ? m.up_extrinsic[dir] : m.down_extrinsic[dir]), drone, 0);
                }
                std::vector<int> iu, id;
                for (int i = 0; i < c.nm[p]; ++i) {
                    const int a = c.mu[p * M + i], b = c.md[p * M + i];
                    if (a < 0 || a >= c.n_kps[img[0]] || b < 0 || b >= c.n_kps[img[1]]) continue;
                    iu.push_back(a); id.push_back(b);
                }
                count[p] = fill_stereo_landmarks(im[0], im[1], iu.data(), id.data(), (int)iu.size(), m.triangle_thres, m.accept_min_3d_pts, &lift);
                if (c.n_kps[img[0]] > m.accept_min_3d_pts) {
                    const geom::Pose pu = to_pose(drone) * to_pose(im[0].camera_extrinsic), pd = to_pose(drone) * to_pose(im[1].camera_extrinsic);
                    for (size_t i = 0; i < iu.size(); ++i) ties[0] += host_tie(pu, pd, lift(im[0].landmarks_2d[(size_t)iu[i]]), lift(im[1].landmarks_2d[(size_t)id[i]]));
                }
                for (int s = 0; s < 2; ++s)
                    for (size_t k = 0; k < im[s].landmarks_2d.size(); ++k) {
                        const size_t at = img[s] * M + k;
                        norm[at * 2] = im[s].landmarks_2d_norm[k].x; norm[at * 2 + 1] = im[s].landmarks_2d_norm[k].y;
                        l3d[at * 3] = im[s].landmarks_3d[k].x; l3d[at * 3 + 1] = im[s].landmarks_3d[k].y; l3d[at * 3 + 2] = im[s].landmarks_3d[k].z;
                        flag[at] = im[s].landmarks_flag[k];
                    }
            }
        }
        put(norm); put(l3d); put(flag); put(count); put(ties);
    }
    if (rc < 0) { fprintf(stderr, "camera_plan_pin: truncated or inconsistent case\n"); return 1; }
    return 0;
}

// ---- depth ---------------------------------------------------------------------------------------------------------------------------------------------
static int run_depth() {
    for (;;) {
        int hdr[4];
        const size_t got = fread(hdr, sizeof(int), 4, stdin);
        if (got == 0) return 0;
        CameraModel camera;
        double k[6], pose[7], ext[7];
        if (got != 4 || hdr[0] < 0 || hdr[1] < 1 || hdr[2] < 1 || fread(&camera.model, sizeof(camera.model), 1, stdin) != 1 || fread(k, sizeof(double), 6, stdin) != 6 ||
            fread(pose, sizeof(double), 7, stdin) != 7 || fread(ext, sizeof(double), 7, stdin) != 7) return 1;
        const size_t n = (size_t)hdr[0];
        std::vector<float> kps;
        std::vector<uint16_t> depth;
        if (!get(kps, 2 * n) || !get(depth, (size_t)hdr[1] * hdr[2])) return 1;
        camera.fx = k[0]; camera.fy = k[1]; camera.cx = k[2]; camera.cy = k[3];
        const std::function<geom::Vec2(const Point2f&)> lift = [&camera](const Point2f& p) { return camera.lift(p); };
        ImageDescriptor im;
        fill_image_descriptor(im, kps.data(), (int)n, nullptr, 0, nullptr, 0, lift);
        stamp_image_descriptor(im, 0.0, 0, msg7(ext), msg7(pose), 0);
        std::vector<int> count(1, fill_depth_landmarks(im, depth.data(), hdr[1], hdr[1], hdr[2], k[4], k[5], hdr[3], lift));
        std::vector<float> norm(2 * n), l3d(3 * n);
        for (size_t i = 0; i < n; ++i) {
            norm[2 * i] = im.landmarks_2d_norm[i].x; norm[2 * i + 1] = im.landmarks_2d_norm[i].y;
            l3d[3 * i] = im.landmarks_3d[i].x; l3d[3 * i + 1] = im.landmarks_3d[i].y; l3d[3 * i + 2] = im.landmarks_3d[i].z;
        }
        put(norm); put(l3d); put(im.landmarks_flag); put(count);
    }
}

// ---- yaml --------------------------------------------------------------------------------------------------------------------------------------------------
static int run_yaml(int width, int height) {
    const std::string text((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
    try {
        SwarmLoopParams p;
        p.width = width; p.height = height;
        p.read_camera_config(text);
        KeyframePipeline::Config c;
        p.to_pipeline_config(c);
        const CameraModel& f = p.camera;
        printf("%d %.17g %.17g %.17g %.17g %.17g | %.17g %.17g %.17g %.17g | %d %d | %.17g %.17g %.17g %.17g\n", c.camera_model.type, c.camera_model.k1, c.camera_model.k2,
               c.camera_model.p1, c.camera_model.p2, c.camera_model.xi, f.fx, f.fy, f.cx, f.cy, f.image_width, f.image_height, c.fx, c.fy, c.cx, c.cy);
    } catch (const std::exception& e) { printf("ERROR %s\n", e.what()); }
    return 0;
}

// ---- config ------------------------------------------------------------------------------------------------------------------------------------------------
static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)
static std::string refusal(const KeyframePipeline::Config& c) {
    try { KeyframePipeline::resolved(c); return ""; } catch (const std::exception& e) { return e.what(); }
}
static int run_config() {
    using Config = KeyframePipeline::Config;
    const omni_camera_model mild = {OMNI_CAMERA_PINHOLE, -0.05, 0.01, 1e-3, -1e-3, 0.0}, mei = {OMNI_CAMERA_MEI, -0.05, 0.01, 1e-3, -1e-3, 1.2};
    { Config c; EXPECT(cam::is_ideal(c.camera_model) && refusal(c).empty()); }                                   // the default is the ideal pinhole
    for (int configuration = 0; configuration < 3; ++configuration) {                                          // a lens is accepted in every configuration ...
        Config c;
        c.camera_configuration = configuration; c.camera_model = mild; EXPECT(refusal(c).empty());
        c.camera_model = mei; EXPECT(refusal(c).empty());
    }
    {                                                                                                          // ... but not in the raw-fisheye mode, and the message says why
        Config c;
        c.camera_configuration = 1; c.width = 600; c.height = 312; c.fisheye_src_width = 1280; c.fisheye_src_height = 1024; c.fisheye_fov_deg = 235.0;
        EXPECT(refusal(c).empty());
        c.camera_model = mild;
        EXPECT(refusal(c).find("ideal pinhole views") != std::string::npos && refusal(c).find("raw-fisheye") != std::string::npos);
        c.camera_model = {OMNI_CAMERA_PINHOLE, 0, 0, 0, 0, 0};
        EXPECT(refusal(c).empty());
    }
    { Config c; c.camera_model = mei; c.camera_model.xi = 0.0; EXPECT(refusal(c).find("xi > 0") != std::string::npos); }
    { Config c; c.camera_model = mei; c.camera_model.xi = -1.0; EXPECT(refusal(c).find("xi > 0") != std::string::npos); }
    { Config c; c.camera_model = mild; c.camera_model.k2 = NAN; EXPECT(refusal(c).find("not finite") != std::string::npos); }
    { Config c; c.camera_model = mild; c.camera_model.p1 = INFINITY; EXPECT(refusal(c).find("not finite") != std::string::npos); }
    { Config c; c.camera_model = mild; c.camera_model.type = 2; EXPECT(refusal(c).find("unknown type") != std::string::npos); }
    EXPECT(cam::check(mild) == nullptr && cam::check(mei) == nullptr && cam::check(cam::ideal()) == nullptr);
    std::printf(failures ? "FAILED %d\n" : "OK\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    const char* mode = argc >= 2 ? argv[1] : "";
    if (argc == 2 && (!strcmp(mode, "lift") || !strcmp(mode, "lmlift") || !strcmp(mode, "project"))) {
        const int rc = run_points(mode);
        if (rc) fprintf(stderr, "camera_plan_pin: truncated record\n");
        return rc;
    }
    if (argc == 2 && (!strcmp(mode, "plan") || !strcmp(mode, "host"))) return run_cases(!strcmp(mode, "plan"));
    if (argc == 2 && !strcmp(mode, "depth")) { const int rc = run_depth(); if (rc) fprintf(stderr, "camera_plan_pin: truncated record\n"); return rc; }
    if (argc == 4 && !strcmp(mode, "yaml")) return run_yaml(atoi(argv[2]), atoi(argv[3]));
    if (argc == 2 && !strcmp(mode, "config")) return run_config();
    fprintf(stderr, "usage: camera_plan_pin lift|lmlift|project|plan|host|depth|config < records, camera_plan_pin yaml W H < text\n");
    return 2;
}
