// camera_plan.h -- the lens model of the lift, stated once: what the reference's camodocal camera does in cam->liftProjective before the caller divides by z
// (swarm_loop/src/loop_cam.cpp:558-569 for the message's landmarks_2d_norm, :403-407 for the triangulation, :289-291 for the depth landmarks), for the two
// model types its launch files name: PINHOLE (with distortion coefficients; launch/realsense.launch) and MEI (the default cam0_mei.yaml).  Plain C++ for g++
// AND hipcc: landmark_plan.h calls it one key point per lane, host/camera_model.hpp calls it for the host path, tests/cpp/camera_plan_pin.cpp pins it.
//
// UNPINNED: camodocal is not vendored and does not build here, so the formulas below ARE the specification -- written from the published model (Mei & Rives'
// unified projection with the plumb-bob distortion, camodocal's PinholeCamera / CataCamera liftProjective with their fixed 8 / 6 recursive rounds).  Parity with
// a camodocal build, bit for bit or otherwise, has not been measured; tests/test_camera_plan_cpu.py holds this header to a restatement of the same formulas
// and to its own forward model (project), nothing more.  host/fisheye_flatten.hpp flags its MEI model the same way.
//
// f64, every product and sum rounded on its own (contraction off), IEEE division and square root: the g++ build and the gfx950 build give the same bits.
//
//   lift(model, fx, fy, cx, cy, x, y)
//     1  mx_d = ((double)x - cx) / fx, my_d = ((double)y - cy) / fy                       (the ideal pinhole's whole lift, character for character)
//     2  d(mx, my): mx2 = mx*mx; my2 = my*my; mxy = mx*my; rho2 = mx2 + my2; rad = k1*rho2 + k2*rho2*rho2;
//                   dx = mx*rad + 2*p1*mxy + p2*(rho2 + 2*mx2);  dy = my*rad + 2*p2*mxy + p1*(rho2 + 2*my2);     C expressions as written, left to right
//     3  (mx_u, my_u) = (mx_d, my_d) - d(mx_d, my_d), then n - 1 times (mx_u, my_u) = (mx_d, my_d) - d(mx_u, my_u); n = 8 (PINHOLE), 6 (MEI); a constant trip
//        count, no convergence test.  PINHOLE with k1 = k2 = p1 = p2 = 0 exactly skips the step (camodocal's m_noDistortion).
//     4  PINHOLE: (mx_u, my_u), z = 1.  MEI: rho2 = mx_u*mx_u + my_u*my_u; z = xi == 1 ? (1 - rho2) / 2 : 1 - xi*(rho2 + 1) / (xi + sqrt(1 + (1 - xi*xi)*rho2));
//        the result is (mx_u / z, my_u / z).
//   Nothing is clamped: a diverging iteration or a negative radicand gives inf or NaN, which flow on as they do on the host.
//
//   project(model, fx, fy, cx, cy, X)   the forward model, for tests and synthetic data only: PINHOLE m = (X/Z, Y/Z); MEI: the point normalised to the unit
//        sphere, xi added to z, m = (x/z, y/z); both: m + d(m), pixel = (fx*m.x + cx, fy*m.y + cy).
#pragma once
#include <math.h>

#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define CAM_HD __host__ __device__ inline
#else
#define CAM_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace omni {
namespace cam {

// the ideal pinhole: what every entry point without a lens model passes
CAM_HD omni_camera_model ideal() {
    omni_camera_model m;
    m.type = OMNI_CAMERA_PINHOLE; m.k1 = 0; m.k2 = 0; m.p1 = 0; m.p2 = 0; m.xi = 0;
    return m;
}
CAM_HD bool is_ideal(const omni_camera_model& m) { return m.type == OMNI_CAMERA_PINHOLE && m.k1 == 0 && m.k2 == 0 && m.p1 == 0 && m.p2 == 0; }

// nullptr when the model can be lifted with, else what is wrong with it: an unknown type, a non-finite coefficient, MEI with xi <= 0
inline const char* check(const omni_camera_model& m) {
    if (m.type != OMNI_CAMERA_PINHOLE && m.type != OMNI_CAMERA_MEI) return "camera model: unknown type (0: PINHOLE, 1: MEI)";
    const double c[5] = {m.k1, m.k2, m.p1, m.p2, m.xi};
    for (int i = 0; i < 5; ++i)
        if (!(c[i] - c[i] == 0)) return "camera model: a coefficient (k1 k2 p1 p2 xi) is not finite";
    if (m.type == OMNI_CAMERA_MEI && !(m.xi > 0)) return "camera model: MEI needs xi > 0";
    return nullptr;
}

// step 2
CAM_HD void distortion(const omni_camera_model& m, double mx, double my, double* dx, double* dy) {
    const double k1 = m.k1, k2 = m.k2, p1 = m.p1, p2 = m.p2;
    const double mx2 = mx * mx, my2 = my * my, mxy = mx * my, rho2 = mx2 + my2, rad = k1 * rho2 + k2 * rho2 * rho2;
    *dx = mx * rad + 2 * p1 * mxy + p2 * (rho2 + 2 * mx2);
    *dy = my * rad + 2 * p2 * mxy + p1 * (rho2 + 2 * my2);
}

CAM_HD void lift(const omni_camera_model& m, double fx, double fy, double cx, double cy, float x, float y, double* out) {
    const double mx_d = ((double)x - cx) / fx;
    const double my_d = ((double)y - cy) / fy;
    double mx_u = mx_d, my_u = my_d;
    if (!is_ideal(m)) {
        const int n = m.type == OMNI_CAMERA_MEI ? 6 : 8;
        for (int i = 0; i < n; ++i) {                       // (round 0 reads the distorted point itself)
            double dx, dy;
            distortion(m, mx_u, my_u, &dx, &dy);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    if (m.type == OMNI_CAMERA_MEI) {
        const double xi = m.xi, rho2 = mx_u * mx_u + my_u * my_u;
        const double z = xi == 1.0 ? (1.0 - rho2) / 2.0 : 1.0 - xi * (rho2 + 1.0) / (xi + sqrt(1.0 + (1.0 - xi * xi) * rho2));
        out[0] = mx_u / z; out[1] = my_u / z;
    } else {
        out[0] = mx_u; out[1] = my_u;
    }
}

// the forward model (tests, synthetic data): a point in the camera's frame -> its pixel
inline void project(const omni_camera_model& m, double fx, double fy, double cx, double cy, const double* X, double* out) {
    double mx, my;
    if (m.type == OMNI_CAMERA_MEI) {
        const double n = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
        const double x = X[0] / n, y = X[1] / n, z = X[2] / n + m.xi;
        mx = x / z; my = y / z;
    } else {
        mx = X[0] / X[2]; my = X[1] / X[2];
    }
    double dx, dy;
    distortion(m, mx, my, &dx, &dy);
    mx = mx + dx; my = my + dy;
    out[0] = fx * mx + cx; out[1] = fy * my + cy;
}

}  // namespace cam
}  // namespace omni
