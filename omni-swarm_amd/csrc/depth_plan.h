// depth_plan.h -- the depth landmarks of one image of a PINHOLE_DEPTH key frame, stated once: what generate_gray_depth_image_descriptor does between the networks
// and the frame message (swarm_loop/src/loop_cam.cpp:260-304 with the lifted floats of extractor_img_desc_deepnet :558-566), as host/loop_geometry.hpp states
// it: fill_image_descriptor's landmarks_2d_norm + fill_depth_landmarks, the latter WITH its one recorded deviation (a key point the 640 x 480 gate lets through
// but which lies outside this depth image gets no landmark).  Plain C++ for g++ AND hipcc: depth_landmarks.hip runs it one key-point slot per lane,
// depth_host.cpp (omni_depth_landmarks_host) and tests/cpp/depth_plan_pin.cpp run it on the host; nothing else restates the arithmetic.  The lens is
// camera_plan.h's, the pose algebra landmark_plan.h's (pose_from7, pose_mul, quat_R, mat_vec, clamp_count).
//
// SAME OPERATIONS IN THE SAME ORDER as the host functions, every product and sum rounded on its own (contraction off), IEEE division: a g++ build of this
// header is bit-identical to them, and the gfx950 build is meant to be.
//
//   per image  landmarks_3d and landmarks_flag zeroed for all max_num slots; norm2d of slot k < clamp_count(n, max_num) is the float-cast cam::lift, zero behind.
//   live       no landmarks at all unless the image has MORE than accept_min_3d_pts key points (:266-270), or when it has no depth frame.
//   slot       1  the reference's literal gate (:280): x < 0 || x > 640 || y < 0 || y > 480 drops the point (inclusive upper bounds);
//              2  px = rint((double)x), py = rint((double)y): half to even, what lrint does in the default rounding mode (cv::Mat::at<ushort>(Point2f));
//              3  px >= depth_w or py >= depth_h: no landmark (the deviation);
//              4  dep = depth[py * stride + px] / 1000.0;
//              5  strictly dep > near && dep < far;
//              6  the lift in double -- the SAME call that gave norm2d its floats: one lift per key point serves both;
//              7  pose_cam.pos + R(pose_cam.att) * {n.x * dep, n.y * dep, dep}, pose_cam = pose_drone * extrinsic; cast to float, flag 1.
//   count_3d   the landmarks set.
#pragma once
#include "landmark_plan.h"

namespace omni {
namespace dp {

// nullptr when the stage can run with the model / on arrays of these sizes, else what is wrong (the refusals of every entry that takes them)
inline const char* check_model(const omni_depth_model& m) {
    if (!(m.fx != 0 && m.fy != 0 && m.fx == m.fx && m.fy == m.fy)) return "depth model: a focal length is zero or NaN";
    if (m.depth_width < 1 || m.depth_height < 1) return "depth model: depth_width / depth_height below 1";
    if (!(m.depth_near == m.depth_near && m.depth_far == m.depth_far)) return "depth model: depth_near or depth_far is NaN";
    return nullptr;
}
inline const char* check_sizes(const omni_depth_model& m, int n_images, int max_num, int stride) {
    if (n_images < 1 || n_images > 65535) return "depth landmarks: n_images outside [1, 65535]";
    if (max_num < 1 || max_num > 1024) return "depth landmarks: max_num outside [1, 1024]";
    if (stride < m.depth_width) return "depth landmarks: a depth stride (elements) below depth_width";
    return nullptr;
}

// what every key point of one image shares: pose_cam = pose_drone * extrinsic as a rotation matrix and a position
struct ImageGeom { double R[3][3]; double pos[3]; };
LM_HD void image_geom(const double* pose_drone7, const double* extrinsic7, ImageGeom& g) {
    const lm::Pose pose_cam = lm::pose_mul(lm::pose_from7(pose_drone7), lm::pose_from7(extrinsic7));
    lm::quat_R(pose_cam.q, g.R);
    g.pos[0] = pose_cam.p[0]; g.pos[1] = pose_cam.p[1]; g.pos[2] = pose_cam.p[2];
}

// does the image get landmarks at all?  n_raw as the network reports it, have: it came with a depth frame
LM_HD bool image_live(const omni_depth_model& m, int max_num, int n_raw, bool have) { return have && lm::clamp_count(n_raw, max_num) > m.accept_min_3d_pts; }

// ONE slot k of [0, max_num) of one image: writes norm [2], l3d [3] and flag of the slot, returns 1 when it got a landmark.  n = clamp_count(n_raw, max_num);
// `depth` is read only for a live image
LM_HD int slot(const omni_depth_model& m, const omni_camera_model& c, const ImageGeom& g, bool live, int n, const float* kps, const uint16_t* depth, int stride, int k, float* norm,
               float* l3d, uint8_t* flag) {
    float nx = 0.f, ny = 0.f, wx = 0.f, wy = 0.f, wz = 0.f;
    int set = 0;
    if (k < n) {
        const float x = kps[2 * k], y = kps[2 * k + 1];
        double q[2];
        cam::lift(c, m.fx, m.fy, m.cx, m.cy, x, y, q);
        nx = (float)q[0]; ny = (float)q[1];
        if (live && !(x < 0 || x > 640 || y < 0 || y > 480)) {
            const double rx = rint((double)x), ry = rint((double)y);
            if (rx >= 0 && rx < m.depth_width && ry >= 0 && ry < m.depth_height) {      // (a NaN coordinate passes the gate and stops here, as the host's lrint does)
                const double dep = depth[(size_t)ry * stride + (size_t)rx] / 1000.0;
                if (dep > m.depth_near && dep < m.depth_far) {
                    const double v[3] = {q[0] * dep, q[1] * dep, dep};
                    double r[3];
                    lm::mat_vec(g.R, v, r);
                    wx = (float)(g.pos[0] + r[0]); wy = (float)(g.pos[1] + r[1]); wz = (float)(g.pos[2] + r[2]);
                    set = 1;
                }
            }
        }
    }
    norm[2 * k] = nx; norm[2 * k + 1] = ny;
    l3d[3 * k] = wx; l3d[3 * k + 1] = wy; l3d[3 * k + 2] = wz;
    flag[k] = (uint8_t)set;
    return set;
}

// host form of the whole stage on the arrays of omni_depth_landmarks_enqueue_dev: what the kernel computes, sequentially.  depth: image i at
// depth + i * stride * depth_height; have == nullptr: every image has a depth frame
inline void depth_landmarks_host(const omni_depth_model& m, const omni_camera_model& c, const double* poses7, int n_images, int max_num, const float* kps_xy, const int* n_kps,
                                 const uint16_t* depth, int stride, const uint8_t* have, float* norm2d, float* l3d, uint8_t* flag, int* count) {
    for (int i = 0; i < n_images; ++i) {
        const size_t at = (size_t)i * max_num;
        const bool live = image_live(m, max_num, n_kps[i], !have || have[i]);
        ImageGeom g;
        image_geom(poses7 + 7 * (size_t)i, m.extrinsic, g);
        const int n = lm::clamp_count(n_kps[i], max_num);
        int cnt = 0;
        for (int k = 0; k < max_num; ++k)
            cnt += slot(m, c, g, live, n, kps_xy + at * 2, depth + (size_t)i * stride * m.depth_height, stride, k, norm2d + at * 2, l3d + at * 3, flag + at);
        count[i] = cnt;
    }
}

}  // namespace dp
}  // namespace omni
