// pnp_plan.h -- the RANSAC half of compute_relative_pose (swarm_loop/src/loop_detector.cpp:355-413: cv::solvePnPRansac(3d, 2d, K = I, ..., iterations, 3, 0.99,
// inliers), 100 iterations, 1 000 in init_mode), stated once: the operations of host/geometry.hpp (CvRng, ransac_run's getSubset loop for five indices,
// epnp on exactly five points with its jacobi_eigen<N> / svd3 / lstsq_small, pnp_error) in the same order.  Plain C++ for g++ AND hipcc: pnp.hip gives every
// lane one hypothesis, tests/cpp/pnp_plan_pin.cpp runs the functions on the host and compares them with geom::ransac_run<PnPModel> and geom::solve_pnp_ransac;
// nothing else restates the arithmetic.  Every product and sum rounds on its own (contraction off), IEEE division and square root; no transcendental function
// (cbrt / cos / sin sit in geom::pnp_refit, which runs once per candidate on the host).
//
// The serial loop of ransac_run, taken apart as in ransac_plan.h:
//   subsets     PnPModel::check_subset is always true: iteration k's subset is the k-th group of five distinct draws of the fixed CvRng stream
//               (seed (uint64)-1; a draw equal to an index already in the group is drawn again), whatever the models were.
//   hypotheses  epnp5 and the inlier count good[k] (-1 when epnp5 fails: the iteration is used up, as ransac_run's `continue`) depend on the subset alone.
//   stop rule   a new best needs good > max(max_good, 4); then niters = RANSACUpdateNumIters(0.99, (count - good) / count, 5, niters) == min(T[good], niters)
//               with T[g] = the same function at max_iters = 1000, `niters` starting at the candidate's own limit (exhaustively equal, tests/test_pnp_plan_cpu.py).
//               The host fills T with its own pow / log.
//   mask        only the best model's: recomputed from the best (R, t) at the end.
//   rounds      subsets for the next R iterations, their R hypotheses, then the scan, until the scan's niters is reached.  R changes nothing but the amount
//               of work thrown away.
// jacobi_eigen's std::sort(order, W[a] > W[b]) is, for N <= 16, libstdc++'s insertion sort: sort_desc below is that algorithm, literally (EPnP reads the whole
// sorted order).  std::max / std::min are the ternaries they are (mx / mn): NaN betas occur and are filtered by finite().
//
// Statuses (OMNI_PNP_* of omni_hip.h):
//   SKIPPED   count < 6: solve_pnp_ransac returns false without drawing.
//   OK        max_good >= 6: mask = the inliers of the best model, Rt = that model (R row-major, then t).
//   NO_MODEL  the host function's `false`: no model, or a best model with five inliers.  mask all 0, Rt all 0.
//   HOST      given up: an iteration that ransac_run would execute needed more than kSubsetDrawBudget draws for its five indices.  With count >= 6 a draw
//             repeats with probability <= 4/6, so a group needs 8.7 draws on average at count 6 and 256 draws with probability below 1e-40: the budget exists
//             so that the loop is bounded whatever the stream, not because an input reaches it.  It only counts where the serial loop would get to.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ransac_plan.h"

// The solver's steps stay separate functions on the device (one call each instead of one function of EPnP's whole size: the register allocator of hipcc
// does not survive the latter); the host build inlines as it likes.  Calls change no arithmetic.
#if defined(__HIPCC__)
#define PNP_STEP __host__ __device__ __attribute__((noinline)) inline
#else
#define PNP_STEP inline
#endif

namespace omni {
namespace pnp {

constexpr int kMaxIters = 1000;                 // compute_relative_pose's limit in init_mode; the table T is computed at this limit
constexpr int kModelPoints = 5;
constexpr int kSubsetDrawBudget = 256;          // draws for ONE group of five distinct indices before the device gives up
constexpr int kMaxN = 2048;                     // correspondences per candidate: 20 bytes each, 40 KB of the workgroup's 64 KB of static LDS
constexpr int kRoundFirst = 64, kRound = 256;   // the kernel's round sizes: a true loop ends inside the first (one wave)
constexpr double kDblMax = 1.7976931348623157e308;

// T[g], g = 0 .. count: what `niters` becomes at most once a model with g inliers of count is the best.  HOST ONLY (pow / log)
inline void fill_T(int count, int* T) { for (int g = 0; g <= count; ++g) T[g] = rs::update_num_iters(0.99, (double)(count - g) / count, kModelPoints, kMaxIters); }

RS_HD double mx(double a, double b) { return a < b ? b : a; }      // std::max(a, b)
RS_HD double mn(double a, double b) { return b < a ? b : a; }      // std::min(a, b)
RS_HD bool finite(double v) { return fabs(v) <= kDblMax; }         // std::isfinite

// ---- geom::Vec2 / Vec3 / Mat3 with the operations epnp uses, each spelled as geometry.hpp spells it ------------------------------------------------------
struct V2 { double x, y; };
struct V3 { double x, y, z; };
RS_HD V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
RS_HD V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
RS_HD V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
RS_HD double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RS_HD V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
struct M3 { double m[3][3]; };
RS_HD V3 mul(const M3& a, V3 v) { return {a.m[0][0] * v.x + a.m[0][1] * v.y + a.m[0][2] * v.z, a.m[1][0] * v.x + a.m[1][1] * v.y + a.m[1][2] * v.z, a.m[2][0] * v.x + a.m[2][1] * v.y + a.m[2][2] * v.z}; }
RS_HD M3 mul(const M3& a, const M3& o) { M3 r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { r.m[i][j] = 0; for (int k = 0; k < 3; ++k) r.m[i][j] += a.m[i][k] * o.m[k][j]; } return r; }
RS_HD M3 transpose(const M3& a) { M3 r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[j][i]; return r; }
RS_HD double det(const M3& a) {
    return a.m[0][0] * (a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1]) - a.m[0][1] * (a.m[1][0] * a.m[2][2] - a.m[1][2] * a.m[2][0]) +
           a.m[0][2] * (a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0]);
}
struct Rt { M3 R; V3 t; };

// ---- std::sort(order, order + N, W[a] > W[b]) for N <= 16: libstdc++'s __insertion_sort (a value that beats the first goes to the front, every other one
// walks down while it beats its neighbour) ------------------------------------------------------------------------------------------------------------------
template <int N>
RS_HD void sort_desc(const double* W, int* order) {
    for (int i = 0; i < N; ++i) order[i] = i;
    for (int i = 1; i < N; ++i) {
        const int val = order[i];
        if (W[val] > W[order[0]]) { for (int j = i; j > 0; --j) order[j] = order[j - 1]; order[0] = val; }
        else { int j = i; while (j > 0 && W[val] > W[order[j - 1]]) { order[j] = order[j - 1]; --j; } order[j] = val; }      // (j > 0 never ends it: order[0] is not beaten)
    }
}
// geom::jacobi_eigen<N>: eigenvalues DESCENDING, eigenvectors as ROWS of V; A is destroyed
template <int N>
PNP_STEP void jacobi_eigen(double A[N][N], double W[N], double V[N][N]) {
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < N; ++i) { diag += A[i][i] * A[i][i]; for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j]; }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < N; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                for (int k = 0; k < N; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                for (int k = 0; k < N; ++k) { const double vpk = V[p][k], vqk = V[q][k]; V[p][k] = c * vpk - s * vqk; V[q][k] = s * vpk + c * vqk; }
            }
    }
    int order[N];
    for (int i = 0; i < N; ++i) W[i] = A[i][i];
    sort_desc<N>(W, order);
    // the rows in sorted order; A is free by now and takes the copy
    double Wt[N];
    for (int i = 0; i < N; ++i) { Wt[i] = W[order[i]]; for (int k = 0; k < N; ++k) A[i][k] = V[order[i]][k]; }
    for (int i = 0; i < N; ++i) { W[i] = Wt[i]; for (int k = 0; k < N; ++k) V[i][k] = A[i][k]; }
}
// geom::svd3: M = U diag(s) V^T through the eigen-decomposition of M^T M (s descending; U, V as columns)
PNP_STEP void svd3(const M3& M, M3& U, double s[3], M3& V) {
    double A[3][3], W[3], E[3][3];
    const M3 MtM = mul(transpose(M), M);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = MtM.m[i][j];
    jacobi_eigen<3>(A, W, E);
    V3 v[3], u[3];
    for (int i = 0; i < 3; ++i) { v[i] = {E[i][0], E[i][1], E[i][2]}; s[i] = sqrt(mx(W[i], 0.0)); }
    for (int i = 0; i < 2; ++i) u[i] = s[i] > 1e-300 ? (1.0 / s[i]) * mul(M, v[i]) : V3{i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, 0};
    u[2] = cross(u[0], u[1]);
    if (s[2] > 1e-12 * mx(s[0], 1e-300)) { const V3 m2 = (1.0 / s[2]) * mul(M, v[2]); if (dot(u[2], m2) < 0) u[2] = -1.0 * u[2]; }
    for (int i = 0; i < 3; ++i) { U.m[0][i] = u[i].x; U.m[1][i] = u[i].y; U.m[2][i] = u[i].z; V.m[0][i] = v[i].x; V.m[1][i] = v[i].y; V.m[2][i] = v[i].z; }
}
// geom::lstsq_small<ROWS, N>
template <int ROWS, int N>
PNP_STEP void lstsq_small(const double (&A)[ROWS][N], const double (&b)[ROWS], double (&x)[N]) {
    double AtA[N][N], Atb[N], W[N], V[N][N];
    for (int i = 0; i < N; ++i) { Atb[i] = 0; for (int r = 0; r < ROWS; ++r) Atb[i] += A[r][i] * b[r]; for (int j = 0; j < N; ++j) { AtA[i][j] = 0; for (int r = 0; r < ROWS; ++r) AtA[i][j] += A[r][i] * A[r][j]; } }
    jacobi_eigen<N>(AtA, W, V);
    for (int i = 0; i < N; ++i) x[i] = 0;
    for (int k = 0; k < N; ++k) {
        if (!(W[k] > 1e-26 * mx(W[0], 1e-300))) continue;
        double c = 0;
        for (int i = 0; i < N; ++i) c += V[k][i] * Atb[i];
        c /= W[k];
        for (int i = 0; i < N; ++i) x[i] += c * V[k][i];
    }
}

// ---- geom::epnp for exactly five points ------------------------------------------------------------------------------------------------------------------
struct Epnp5 {                     // what the steps behind the null vectors read
    V3 P[5]; V2 q[5];
    V3 cws[4];
    double al[5][4], v[4][12], L[6][10], rho[6];
};
PNP_STEP void gauss_newton(const Epnp5& e, double (&be)[4]) {
    for (int it = 0; it < 5; ++it) {
        double A[6][4], bb[6], x[4];
        for (int r = 0; r < 6; ++r) {
            const double* l = e.L[r];
            A[r][0] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
            A[r][1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
            A[r][2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
            A[r][3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
            bb[r] = e.rho[r] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] + l[5] * be[2] * be[2] +
                                l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
        }
        lstsq_small<6, 4>(A, bb, x);
        for (int k = 0; k < 4; ++k) be[k] += x[k];
    }
}
// compute_R_and_t: control points in the camera frame from the betas, sign from the first point's depth, Arun's alignment, mean reprojection error
PNP_STEP double r_and_t(const Epnp5& e, const double (&be)[4], Rt& rt) {
    const int n = 5;
    V3 ccs[4];
    for (int j = 0; j < 4; ++j) { double c[3] = {0, 0, 0}; for (int i = 0; i < 4; ++i) for (int k = 0; k < 3; ++k) c[k] += be[i] * e.v[i][3 * j + k]; ccs[j] = {c[0], c[1], c[2]}; }
    V3 pcs[5];
    for (int i = 0; i < n; ++i) { V3 p = {0, 0, 0}; for (int j = 0; j < 4; ++j) p = p + e.al[i][j] * ccs[j]; pcs[i] = p; }
    if (pcs[0].z < 0) { for (int j = 0; j < 4; ++j) ccs[j] = -1.0 * ccs[j]; for (int i = 0; i < n; ++i) pcs[i] = -1.0 * pcs[i]; }
    V3 pc0 = {0, 0, 0}, pw0 = {0, 0, 0};
    for (int i = 0; i < n; ++i) { pc0 = pc0 + pcs[i]; pw0 = pw0 + e.P[i]; }
    pc0 = (1.0 / n) * pc0; pw0 = (1.0 / n) * pw0;
    M3 ABt;
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) ABt.m[a][b] = 0;
    for (int i = 0; i < n; ++i) {
        const V3 a = pcs[i] - pc0, b = e.P[i] - pw0;
        const double av[3] = {a.x, a.y, a.z}, bv[3] = {b.x, b.y, b.z};
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) ABt.m[r][c] += av[r] * bv[c];
    }
    M3 U, V;
    double sv[3];
    svd3(ABt, U, sv, V);
    rt.R = mul(U, transpose(V));
    if (det(rt.R) < 0) for (int c = 0; c < 3; ++c) rt.R.m[2][c] = -rt.R.m[2][c];
    rt.t = pc0 - mul(rt.R, pw0);
    double sum = 0;
    for (int i = 0; i < n; ++i) { const V3 c = mul(rt.R, e.P[i]) + rt.t; const double dx = c.x / c.z - e.q[i].x, dy = c.y / c.z - e.q[i].y; sum += sqrt(dx * dx + dy * dy); }
    return sum / n;
}
// X [count][3], u [count][2]: float-valued (Point3f landmarks, rotate_pt_norm2d's float cast), widened here, which is exact
PNP_STEP bool epnp5(const float* X, const float* u, const int* idx, Rt& out) {
    const int n = 5;
    Epnp5 e;
    for (int i = 0; i < n; ++i) { e.P[i] = {(double)X[3 * idx[i]], (double)X[3 * idx[i] + 1], (double)X[3 * idx[i] + 2]}; e.q[i] = {(double)u[2 * idx[i]], (double)u[2 * idx[i] + 1]}; }
    // choose_control_points: the centroid and the principal axes scaled by sqrt(eigenvalue / n)
    V3 c0 = {0, 0, 0};
    for (int i = 0; i < n; ++i) c0 = c0 + e.P[i];
    c0 = (1.0 / n) * c0;
    double C[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, dc[3], uct[3][3];
    for (int i = 0; i < n; ++i) { const double d[3] = {e.P[i].x - c0.x, e.P[i].y - c0.y, e.P[i].z - c0.z}; for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) C[a][b] += d[a] * d[b]; }
    jacobi_eigen<3>(C, dc, uct);
    e.cws[0] = c0;
    for (int i = 0; i < 3; ++i) {
        int big = 0;
        for (int k = 1; k < 3; ++k) if (fabs(uct[i][k]) > fabs(uct[i][big])) big = k;
        const double sg = uct[i][big] < 0 ? -1.0 : 1.0, k = sqrt(mx(dc[i], 0.0) / n);
        e.cws[i + 1] = c0 + (sg * k) * V3{uct[i][0], uct[i][1], uct[i][2]};
    }
    // compute_barycentric_coordinates: pseudo-inverse of [c1-c0 | c2-c0 | c3-c0]
    M3 CC;
    for (int j = 0; j < 3; ++j) { const V3 d = e.cws[j + 1] - e.cws[0]; CC.m[0][j] = d.x; CC.m[1][j] = d.y; CC.m[2][j] = d.z; }
    M3 CCinv;
    {
        double A[3][3], W[3], V[3][3];
        const M3 CtC = mul(transpose(CC), CC);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = CtC.m[i][j];
        jacobi_eigen<3>(A, W, V);
        M3 S;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
            S.m[i][j] = 0;
            for (int k = 0; k < 3; ++k) if (W[k] > 1e-20 * mx(W[0], 1e-300)) S.m[i][j] += V[k][i] * V[k][j] / W[k];
        }
        CCinv = mul(S, transpose(CC));
    }
    for (int i = 0; i < n; ++i) {
        const V3 a = mul(CCinv, e.P[i] - e.cws[0]);
        e.al[i][1] = a.x; e.al[i][2] = a.y; e.al[i][3] = a.z; e.al[i][0] = 1.0 - a.x - a.y - a.z;
    }
    // fill_M (fu = fv = 1, uc = vc = 0) and M^T M, its four smallest eigenvectors
    {
        double MtM[12][12], Wm[12], Vm[12][12];
        for (int a = 0; a < 12; ++a) for (int b = 0; b < 12; ++b) MtM[a][b] = 0;
        for (int i = 0; i < n; ++i) {
            double m1[12], m2[12];
            for (int j = 0; j < 4; ++j) { m1[3 * j] = e.al[i][j]; m1[3 * j + 1] = 0; m1[3 * j + 2] = -e.al[i][j] * e.q[i].x; m2[3 * j] = 0; m2[3 * j + 1] = e.al[i][j]; m2[3 * j + 2] = -e.al[i][j] * e.q[i].y; }
            for (int a = 0; a < 12; ++a) for (int b = 0; b < 12; ++b) MtM[a][b] += m1[a] * m1[b] + m2[a] * m2[b];
        }
        jacobi_eigen<12>(MtM, Wm, Vm);
        for (int i = 0; i < 4; ++i) for (int k = 0; k < 12; ++k) e.v[i][k] = Vm[11 - i][k];          // v[0] = the smallest eigenvalue's vector
    }
    {                                                                                         // n == 5: canonical basis of the two-dimensional null space
        double basis[2][12];
        int nb = 0;
        for (int k = 0; k < 12 && nb < 2; ++k) {
            double c[12];
            for (int a = 0; a < 12; ++a) c[a] = e.v[0][a] * e.v[0][k] + e.v[1][a] * e.v[1][k];       // column k of the projector Pn
            for (int b = 0; b < nb; ++b) { double d = 0; for (int a = 0; a < 12; ++a) d += c[a] * basis[b][a]; for (int a = 0; a < 12; ++a) c[a] -= d * basis[b][a]; }
            double nr = 0;
            for (int a = 0; a < 12; ++a) nr += c[a] * c[a];
            nr = sqrt(nr);
            if (nr > 1e-3) { for (int a = 0; a < 12; ++a) basis[nb][a] = c[a] / nr; ++nb; }
        }
        if (nb == 2) for (int a = 0; a < 12; ++a) { e.v[0][a] = basis[0][a]; e.v[1][a] = basis[1][a]; }
    }
    for (int i = 0; i < 4; ++i) {
        int big = 0;
        for (int k = 1; k < 12; ++k) if (fabs(e.v[i][k]) > fabs(e.v[i][big])) big = k;
        if (e.v[i][big] < 0) for (int k = 0; k < 12; ++k) e.v[i][k] = -e.v[i][k];
    }
    // compute_L_6x10, compute_rho
    const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
    for (int r = 0; r < 6; ++r) {
        double d[4][3];
        for (int i = 0; i < 4; ++i) for (int k = 0; k < 3; ++k) d[i][k] = e.v[i][3 * pa[r] + k] - e.v[i][3 * pb[r] + k];
#define PNP_DT(a, b) (d[a][0] * d[b][0] + d[a][1] * d[b][1] + d[a][2] * d[b][2])
        const double row[10] = {PNP_DT(0, 0), 2 * PNP_DT(0, 1), PNP_DT(1, 1), 2 * PNP_DT(0, 2), 2 * PNP_DT(1, 2), PNP_DT(2, 2), 2 * PNP_DT(0, 3), 2 * PNP_DT(1, 3), 2 * PNP_DT(2, 3), PNP_DT(3, 3)};
#undef PNP_DT
        for (int k = 0; k < 10; ++k) e.L[r][k] = row[k];
        const V3 dd = e.cws[pa[r]] - e.cws[pb[r]];
        e.rho[r] = dot(dd, dd);
    }
    bool have = false;
    double best_err = 0;
    for (int ap = 1; ap <= 3; ++ap) {
        double be[4] = {0, 0, 0, 0};
        bool ok = true;
        if (ap == 1) {                                         // betas10 columns (B11 B12 B13 B14)
            double A[6][4], x[4];
            for (int r = 0; r < 6; ++r) { A[r][0] = e.L[r][0]; A[r][1] = e.L[r][1]; A[r][2] = e.L[r][3]; A[r][3] = e.L[r][6]; }
            lstsq_small<6, 4>(A, e.rho, x);
            const double b0 = sqrt(fabs(x[0])), sg = x[0] < 0 ? -1.0 : 1.0;
            if (!(b0 > 0)) ok = false;
            else { be[0] = b0; be[1] = sg * x[1] / b0; be[2] = sg * x[2] / b0; be[3] = sg * x[3] / b0; }
        } else if (ap == 2) {                                  // (B11 B12 B22)
            double A[6][3], x[3];
            for (int r = 0; r < 6; ++r) { A[r][0] = e.L[r][0]; A[r][1] = e.L[r][1]; A[r][2] = e.L[r][2]; }
            lstsq_small<6, 3>(A, e.rho, x);
            if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
            else { be[0] = sqrt(x[0]); be[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0) be[0] = -be[0];
        } else {                                               // (B11 B12 B22 B13 B23)
            double A[6][5], x[5];
            for (int r = 0; r < 6; ++r) for (int k = 0; k < 5; ++k) A[r][k] = e.L[r][k];
            lstsq_small<6, 5>(A, e.rho, x);
            if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
            else { be[0] = sqrt(x[0]); be[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0) be[0] = -be[0];
            if (be[0] == 0) ok = false; else be[2] = x[3] / be[0];
        }
        if (!ok || !finite(be[0]) || !finite(be[1]) || !finite(be[2]) || !finite(be[3])) continue;
        gauss_newton(e, be);
        Rt rt;
        const double err = r_and_t(e, be, rt);
        if (finite(err) && (!have || err < best_err)) { have = true; best_err = err; out = rt; }
    }
    return have;
}
// geom::pnp_error(i) <= (float)(3 * 3)
RS_HD bool inlier(const Rt& p, const float* X, const float* u, int i) {
    const V3 c = mul(p.R, V3{(double)X[3 * i], (double)X[3 * i + 1], (double)X[3 * i + 2]}) + p.t;
    const double dx = c.x / c.z - (double)u[2 * i], dy = c.y / c.z - (double)u[2 * i + 1];
    return (float)(dx * dx + dy * dy) <= 9.0f;
}
// one hypothesis: its model and inlier count, -1 when epnp5 fails
PNP_STEP int hypothesis(const float* X, const float* u, int count, const int* idx, Rt& rt) {
    if (!epnp5(X, u, idx, rt)) return -1;
    int good = 0;
    for (int k = 0; k < count; ++k) good += inlier(rt, X, u, k) ? 1 : 0;
    return good;
}
RS_HD void put_rt(double* out, const Rt& p) { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) out[3 * r + c] = p.R.m[r][c]; out[9] = p.t.x; out[10] = p.t.y; out[11] = p.t.z; }
RS_HD Rt get_rt(const double* in) { Rt p; for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p.R.m[r][c] = in[3 * r + c]; p.t = {in[9], in[10], in[11]}; return p; }

// ---- getSubset for five indices: the next group of the stream.  false when the group needed more than kSubsetDrawBudget draws (count >= 6) ---------------
RS_HD bool next_subset(uint64_t& state, int count, int* idx) {
    int i = 0;
    for (int d = 0; d < kSubsetDrawBudget; ++d) {
        const int v = (int)rs::rng_residue(rs::rng_next(state), count);
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || v == idx[j];
        if (seen) continue;
        idx[i] = v;
        if (++i == kModelPoints) return true;
    }
    return false;
}

// ---- the stopping rule as a scan over the iterations in order --------------------------------------------------------------------------------------------
struct Scan { int niters, max_good, best_iter, iters_run; };
RS_HD void scan_init(Scan& s, int max_iters) { s.niters = max_iters > 1 ? max_iters : 1; s.max_good = 0; s.best_iter = -1; s.iters_run = 0; }
// iteration `iter` (< s.niters) had `good` inliers: true when it is the new best model
RS_HD bool scan_step(Scan& s, int iter, int good, const int* T) {
    s.iters_run = iter + 1;
    if (good <= (s.max_good > kModelPoints - 1 ? s.max_good : kModelPoints - 1)) return false;
    s.max_good = good; s.best_iter = iter;
    if (T[good] < s.niters) s.niters = T[good];
    return true;
}
RS_HD int scan_status(const Scan& s) { return s.max_good >= 6 ? OMNI_PNP_OK : OMNI_PNP_NO_MODEL; }
RS_HD void put_info(int* info, int count, const Scan& s) { info[0] = count; info[1] = s.iters_run; info[2] = s.best_iter; info[3] = s.max_good; }

// ---- a whole candidate on the host, in rounds of R iterations (1 <= R <= kMaxIters): what the kernel computes ----------------------------------------------
// X [count][3], u [count][2]; max_iters in 1 .. kMaxIters; T [count + 1] (fill_T); mask [count]; Rt12 [12]; info = {count, iterations run, best iteration,
// max_good}.  Returns the status.
// REFERENCE AND TESTS ONLY (the pin and hook-check programs): it keeps about 120 KB of thread-local arrays per including program -- the host library runs
// geom::pnp_ransac and never calls this, so none of it lands in libomni_host's thread-local storage.
inline int pnp_ransac_host(const float* X, const float* u, int count, int max_iters, const int* T, int R, uint8_t* mask, double* Rt12, int* info) {
    Scan s;
    scan_init(s, max_iters);
    for (int k = 0; k < 12; ++k) Rt12[k] = 0;
    if (count < 6) { put_info(info, count, s); return OMNI_PNP_SKIPPED; }
    static thread_local int subset[kMaxIters][kModelPoints], good[kMaxIters];
    static thread_local Rt models[kMaxIters];
    uint64_t state = 0xffffffffffffffffull;
    bool over = false;
    int base = 0, status = -1;
    Rt best = get_rt(Rt12);
    while (status < 0) {
        int avail = 0;
        while (avail < R && !over) { if (next_subset(state, count, subset[avail])) ++avail; else over = true; }
        for (int j = 0; j < avail; ++j) good[j] = hypothesis(X, u, count, subset[j], models[j]);
        for (int j = 0; j <= R; ++j) {
            if (base + j >= s.niters) { status = scan_status(s); break; }
            if (j == R) break;
            if (j >= avail) { status = OMNI_PNP_HOST; break; }
            if (scan_step(s, base + j, good[j], T)) best = models[j];
        }
        base += R;
    }
    put_info(info, count, s);
    if (status == OMNI_PNP_OK) put_rt(Rt12, best);
    for (int i = 0; i < count; ++i) mask[i] = status == OMNI_PNP_OK && inlier(best, X, u, i) ? 1 : 0;
    return status;
}

}  // namespace pnp
}  // namespace omni
