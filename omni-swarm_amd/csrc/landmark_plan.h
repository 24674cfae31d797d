// landmark_plan.h -- the stereo landmarks of one direction of a key frame, stated once: what generate_stereo_image_descriptor does between the up <-> down
// match and the frame message (swarm_loop/src/loop_cam.cpp:397-444 with triangulatePoint :73-106 and the lifting of extractor_img_desc_deepnet :558-566),
// as host/geometry.hpp (triangulate_point, jacobi_eigen<4>, stereo_landmarks) and host/loop_geometry.hpp (fill_image_descriptor's lifted floats,
// fill_stereo_landmarks) state it.  Plain C++ for g++ AND hipcc: landmarks.hip runs these functions one match per lane, tests/cpp/landmark_plan_pin.cpp runs
// them on the host and compares them bit for bit with the host functions above; nothing else restates the arithmetic.
//
// SAME OPERATIONS IN THE SAME ORDER as geometry.hpp, every product and sum rounded on its own (contraction off: hipcc's default would fuse a * b + c), IEEE
// division and square root: a g++ build of this header is bit-identical to the host functions, and the gfx950 build is meant to be.
//
//   lift          camera_plan.h's cam::lift with the model's fx fy cx cy: the ideal pinhole ((double)x - cx) / fx, ((double)y - cy) / fy unless an
//                 omni_camera_model says otherwise (camodocal's PINHOLE with distortion, MEI); the message keeps the floats.  Every function that lifts has
//                 two forms: with the lens model, and the earlier signature, which is the ideal pinhole.
//   poses         pose_up = pose_drone * extrinsic_up, pose_down likewise; input xyz + quaternion wxyz, normalised as to_pose() does.
//   triangulate   design matrix, D^T D, the cyclic Jacobi of jacobi_eigen<4> (sweep limit 60, the same stop and skip rules, the same rotation order),
//                 v / v[3], the residual.  Only the eigenvector of the SMALLEST eigenvalue is read: the arg-min of the diagonal replaces the sort.  Where
//                 the smallest eigenvalue is unique both give the same row; a tie is a two-dimensional null space in which the sorted form's choice is
//                 arbitrary too -- ties are reported (*tie) and are outside what the tests gate on finite input.  The arg-min walks from the last row down,
//                 so among equal entries it lands where the host's stable sort does: a lift that diverged to inf (camera_plan.h) makes the whole diagonal
//                 inf before the first sweep, and both forms then read the untouched last row.
//   accept        nothing at all unless the up image has MORE than accept_min_3d_pts key points; a match is dropped when
//                 `err > triangle_thres || pt_cam.z < 0` (literally: a NaN residual passes, as on the host); the float point and flag 1 go to both
//                 images at the matched indices, zeros elsewhere; the number kept is count_3d.
//
// PRECONDITION: the match list is one-to-one -- a query index appears at most once and a train index at most once (every matcher mode of this library:
// cross-check / mutual nearest neighbour).  The writes of different matches then never meet and their order does not matter.  A match whose index lies
// outside [0, n_kps) of its image is skipped: never written through, never counted (the host loop has no such guard; the matcher never emits one).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/omni_hip.h"
#include "camera_plan.h"

#if defined(__HIPCC__)
#define LM_HD __host__ __device__ inline
#else
#define LM_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define LM_UNROLL _Pragma("unroll")
#else
#define LM_UNROLL
#endif

namespace omni {
namespace lm {

struct Pose { double p[3]; double q[4]; };                 // position, attitude (w, x, y, z)

// PoseMsg-shaped input (xyz + quaternion wxyz) -> pose, the quaternion normalised: to_pose() = geom::Quat::normalized()
LM_HD Pose pose_from7(const double* v) {
    Pose r;
    r.p[0] = v[0]; r.p[1] = v[1]; r.p[2] = v[2];
    const double w = v[3], x = v[4], y = v[5], z = v[6];
    const double n = sqrt(w * w + x * x + y * y + z * z);
    r.q[0] = w / n; r.q[1] = x / n; r.q[2] = y / n; r.q[3] = z / n;
    return r;
}
// geom::Quat::R (Eigen::Quaterniond::toRotationMatrix)
LM_HD void quat_R(const double* q, double m[3][3]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    m[0][0] = 1 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy;
    m[1][0] = txy + twz; m[1][1] = 1 - (txx + tzz); m[1][2] = tyz - twx;
    m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1 - (txx + tyy);
}
LM_HD void mat_vec(const double m[3][3], const double* v, double* o) {
    const double a = m[0][0] * v[0] + m[0][1] * v[1] + m[0][2] * v[2], b = m[1][0] * v[0] + m[1][1] * v[1] + m[1][2] * v[2], c = m[2][0] * v[0] + m[2][1] * v[1] + m[2][2] * v[2];
    o[0] = a; o[1] = b; o[2] = c;
}
// geom::Pose::operator*: {pos + att * o.pos, (att * o.att).normalized()}
LM_HD Pose pose_mul(const Pose& a, const Pose& o) {
    Pose r;
    double R[3][3], t[3];
    quat_R(a.q, R);
    mat_vec(R, o.p, t);
    r.p[0] = a.p[0] + t[0]; r.p[1] = a.p[1] + t[1]; r.p[2] = a.p[2] + t[2];
    const double w = a.q[0], x = a.q[1], y = a.q[2], z = a.q[3], ow = o.q[0], ox = o.q[1], oy = o.q[2], oz = o.q[3];
    const double qw = w * ow - x * ox - y * oy - z * oz, qx = w * ox + x * ow + y * oz - z * oy, qy = w * oy - x * oz + y * ow + z * ox, qz = w * oz + x * oy - y * ox + z * ow;
    const double n = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    r.q[0] = qw / n; r.q[1] = qx / n; r.q[2] = qy / n; r.q[3] = qz / n;
    return r;
}

// what every match of one image pair shares: the two projection matrices of triangulate_point and the up camera's frame for the depth test
struct PairGeom {
    double P0[3][4], P1[3][4];
    double Rinv[3][3];                                      // pose_up.att.inverse().R()
    double pos_up[3];
};
LM_HD void projection(const Pose& pose, double P[3][4]) {   // [R^T | -(R^T t)]
    double R[3][3], Rt[3][3], c[3];
    quat_R(pose.q, R);
    LM_UNROLL for (int i = 0; i < 3; ++i) { LM_UNROLL for (int j = 0; j < 3; ++j) Rt[i][j] = R[j][i]; }
    mat_vec(Rt, pose.p, c);
    LM_UNROLL for (int i = 0; i < 3; ++i) { LM_UNROLL for (int j = 0; j < 3; ++j) P[i][j] = Rt[i][j]; P[i][3] = -1.0 * c[i]; }
}
// pose_drone7 / up7 / down7: xyz + quaternion wxyz as they arrive (un-normalised quaternions allowed)
LM_HD void pair_geom(const double* pose_drone7, const double* up7, const double* down7, PairGeom& g) {
    const Pose drone = pose_from7(pose_drone7);
    const Pose pose_up = pose_mul(drone, pose_from7(up7)), pose_down = pose_mul(drone, pose_from7(down7));
    projection(pose_up, g.P0);
    projection(pose_down, g.P1);
    const double qi[4] = {pose_up.q[0], -pose_up.q[1], -pose_up.q[2], -pose_up.q[3]};
    quat_R(qi, g.Rinv);
    g.pos_up[0] = pose_up.p[0]; g.pos_up[1] = pose_up.p[1]; g.pos_up[2] = pose_up.p[2];
}

// the lift of one pixel, in double: the lens model `c` on the stereo model's intrinsics; without one, the ideal pinhole
LM_HD void lift(const omni_stereo_model& m, const omni_camera_model& c, float x, float y, double* o) { cam::lift(c, m.fx, m.fy, m.cx, m.cy, x, y, o); }
LM_HD void lift(const omni_stereo_model& m, float x, float y, double* o) { lift(m, cam::ideal(), x, y, o); }

// geom::triangulate_point from the pair's projections: the point (world frame) and the residual |design * [X; 1]| / 4.  *tie = 1 when the smallest
// diagonal entry after the Jacobi sweeps is not unique.
LM_HD double triangulate(const PairGeom& g, const double* p0, const double* p1, double* point, int* tie) {
    double D[4][4], A[4][4], V[4][4];
    LM_UNROLL for (int j = 0; j < 4; ++j) {
        D[0][j] = p0[0] * g.P0[2][j] - g.P0[0][j]; D[1][j] = p0[1] * g.P0[2][j] - g.P0[1][j];
        D[2][j] = p1[0] * g.P1[2][j] - g.P1[0][j]; D[3][j] = p1[1] * g.P1[2][j] - g.P1[1][j];
    }
    LM_UNROLL for (int i = 0; i < 4; ++i) {
        LM_UNROLL for (int j = 0; j < 4; ++j) {
            double a = 0;
            LM_UNROLL for (int k = 0; k < 4; ++k) a += D[k][i] * D[k][j];
            A[i][j] = a;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
        LM_UNROLL for (int i = 0; i < 4; ++i) { diag += A[i][i] * A[i][i]; LM_UNROLL for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j]; }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        LM_UNROLL for (int p = 0; p < 3; ++p) {
            LM_UNROLL for (int q = p + 1; q < 4; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), s = t * c;
                LM_UNROLL for (int k = 0; k < 4; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                LM_UNROLL for (int k = 0; k < 4; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                LM_UNROLL for (int k = 0; k < 4; ++k) { const double vpk = V[p][k], vqk = V[q][k]; V[p][k] = c * vpk - s * vqk; V[q][k] = s * vpk + c * vqk; }
            }
        }
    }
    // the row of the smallest eigenvalue (selects, not an indexed read: the rows stay in registers)
    // Walked from the LAST row down with a strict comparison: among equal smallest entries the last one wins, which is where the host's stable descending sort
    // leaves it (and row 3 when every entry is NaN) -- so the all-inf diagonal of a lift that diverged picks the host's row too
    double wmin = A[3][3], v0 = V[3][0], v1 = V[3][1], v2 = V[3][2], v3 = V[3][3];
    int n_min = 1;
    LM_UNROLL for (int i = 2; i >= 0; --i) {
        const double w = A[i][i];
        if (w < wmin) { wmin = w; v0 = V[i][0]; v1 = V[i][1]; v2 = V[i][2]; v3 = V[i][3]; n_min = 1; }
        else if (w == wmin) ++n_min;
    }
    *tie = n_min > 1;
    point[0] = v0 / v3; point[1] = v1 / v3; point[2] = v2 / v3;
    double e2 = 0;
    LM_UNROLL for (int i = 0; i < 4; ++i) { const double e = D[i][0] * point[0] + D[i][1] * point[1] + D[i][2] * point[2] + D[i][3]; e2 += e * e; }
    return sqrt(e2) / 4;
}

// ---- one image pair, cut into the two phases the kernel separates by a barrier; work item `lane` of `n_lanes` (the host: 0 of 1) ------------------
// kps_* [max_num][2] pixels, n_* key points (clamped into [0, max_num]); outputs of ONE image each: norm [max_num][2], l3d [max_num][3], flag [max_num].
LM_HD int clamp_count(int n, int max_num) { return n < 0 ? 0 : (n > max_num ? max_num : n); }

// phase 0: the message's lifted floats of every key point of both images (zeros behind the last key point), landmarks and flags zeroed
LM_HD void pair_phase0(const omni_stereo_model& m, const omni_camera_model& c, int max_num, const float* kps_up, int n_up, const float* kps_down, int n_down, float* norm_up, float* norm_down,
                       float* l3d_up, float* l3d_down, uint8_t* flag_up, uint8_t* flag_down, int lane, int n_lanes) {
    n_up = clamp_count(n_up, max_num); n_down = clamp_count(n_down, max_num);
    for (int k = lane; k < 2 * max_num; k += n_lanes) {
        const bool dn = k >= max_num;
        const int i = dn ? k - max_num : k;
        const float* kp = dn ? kps_down : kps_up;
        float* nrm = dn ? norm_down : norm_up;
        float* l3 = dn ? l3d_down : l3d_up;
        double q[2] = {0, 0};
        const bool live = i < (dn ? n_down : n_up);
        if (live) lift(m, c, kp[2 * i], kp[2 * i + 1], q);
        nrm[2 * i] = live ? (float)q[0] : 0.f; nrm[2 * i + 1] = live ? (float)q[1] : 0.f;
        l3[3 * i] = 0.f; l3[3 * i + 1] = 0.f; l3[3 * i + 2] = 0.f;
        (dn ? flag_down : flag_up)[i] = 0;
    }
}
LM_HD void pair_phase0(const omni_stereo_model& m, int max_num, const float* kps_up, int n_up, const float* kps_down, int n_down, float* norm_up, float* norm_down,
                       float* l3d_up, float* l3d_down, uint8_t* flag_up, uint8_t* flag_down, int lane, int n_lanes) {
    pair_phase0(m, cam::ideal(), max_num, kps_up, n_up, kps_down, n_down, norm_up, norm_down, l3d_up, l3d_down, flag_up, flag_down, lane, n_lanes);
}

// phase 1, ONE match: returns 1 when it was kept (and written), 0 otherwise.  *tie as triangulate().
LM_HD int pair_match(const omni_stereo_model& m, const omni_camera_model& c, const PairGeom& g, const float* kps_up, int n_up, const float* kps_down, int n_down, int iu, int id, float* l3d_up,
                     float* l3d_down, uint8_t* flag_up, uint8_t* flag_down, int* tie) {
    *tie = 0;
    if (iu < 0 || iu >= n_up || id < 0 || id >= n_down) return 0;
    double p0[2], p1[2], p[3], d[3], cam[3];
    lift(m, c, kps_up[2 * iu], kps_up[2 * iu + 1], p0);
    lift(m, c, kps_down[2 * id], kps_down[2 * id + 1], p1);
    const double err = triangulate(g, p0, p1, p, tie);
    d[0] = p[0] - g.pos_up[0]; d[1] = p[1] - g.pos_up[1]; d[2] = p[2] - g.pos_up[2];
    mat_vec(g.Rinv, d, cam);
    if (err > m.triangle_thres || cam[2] < 0) return 0;
    const float x = (float)p[0], y = (float)p[1], z = (float)p[2];
    l3d_up[3 * iu] = x; l3d_up[3 * iu + 1] = y; l3d_up[3 * iu + 2] = z; flag_up[iu] = 1;
    l3d_down[3 * id] = x; l3d_down[3 * id + 1] = y; l3d_down[3 * id + 2] = z; flag_down[id] = 1;
    return 1;
}
LM_HD int pair_match(const omni_stereo_model& m, const PairGeom& g, const float* kps_up, int n_up, const float* kps_down, int n_down, int iu, int id, float* l3d_up,
                     float* l3d_down, uint8_t* flag_up, uint8_t* flag_down, int* tie) {
    return pair_match(m, cam::ideal(), g, kps_up, n_up, kps_down, n_down, iu, id, l3d_up, l3d_down, flag_up, flag_down, tie);
}

// the number of matches phase 1 walks: none unless the up image has MORE than accept_min_3d_pts key points (loop_cam.cpp:385)
LM_HD int pair_live_matches(const omni_stereo_model& m, int max_num, int n_up, int n_matches) {
    return clamp_count(n_up, max_num) > m.accept_min_3d_pts ? clamp_count(n_matches, max_num) : 0;
}

// host form of the whole stage on the arrays of omni_landmarks_enqueue_dev ([up images | down images], pair p of key frame p / dirs, direction p % dirs):
// what the kernel computes, sequentially.  Returns the number of tied smallest eigenvalues met.
inline int landmarks_host(const omni_stereo_model& m, const omni_camera_model& cm, const double* poses7, int n_pairs, int max_num, const float* kps_xy, const int* n_kps, const int* match_up,
                          const int* match_down, const int* n_matches, float* norm2d, float* l3d, uint8_t* flag, int* count) {
    int ties = 0;
    const int dirs = m.dirs_per_keyframe;
    for (int p = 0; p < n_pairs; ++p) {
        const int iu = p, id = n_pairs + p;
        const float *ku = kps_xy + (int64_t)iu * max_num * 2, *kd = kps_xy + (int64_t)id * max_num * 2;
        float *l3u = l3d + (int64_t)iu * max_num * 3, *l3d_ = l3d + (int64_t)id * max_num * 3;
        uint8_t *fu = flag + (int64_t)iu * max_num, *fd = flag + (int64_t)id * max_num;
        pair_phase0(m, cm, max_num, ku, n_kps[iu], kd, n_kps[id], norm2d + (int64_t)iu * max_num * 2, norm2d + (int64_t)id * max_num * 2, l3u, l3d_, fu, fd, 0, 1);
        PairGeom g;
        pair_geom(poses7 + 7 * (p / dirs), m.up_extrinsic[p % dirs], m.down_extrinsic[p % dirs], g);
        const int nu = clamp_count(n_kps[iu], max_num), nd = clamp_count(n_kps[id], max_num), nm = pair_live_matches(m, max_num, n_kps[iu], n_matches[p]);
        int c = 0;
        for (int i = 0; i < nm; ++i) {
            int tie = 0;
            c += pair_match(m, cm, g, ku, nu, kd, nd, match_up[(int64_t)p * max_num + i], match_down[(int64_t)p * max_num + i], l3u, l3d_, fu, fd, &tie);
            ties += tie;
        }
        count[p] = c;
    }
    return ties;
}
inline int landmarks_host(const omni_stereo_model& m, const double* poses7, int n_pairs, int max_num, const float* kps_xy, const int* n_kps, const int* match_up,
                          const int* match_down, const int* n_matches, float* norm2d, float* l3d, uint8_t* flag, int* count) {
    return landmarks_host(m, cam::ideal(), poses7, n_pairs, max_num, kps_xy, n_kps, match_up, match_down, n_matches, norm2d, l3d, flag, count);
}

}  // namespace lm
}  // namespace omni
