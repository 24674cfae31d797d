// pgo_plan.h -- the 4-DoF pose graph over ego-motion and loop edges (the loop + ego-motion part of SwarmLocalizationSolver's sliding-window problem:
// swarm_localization_solver.cpp:1064-1100 setup_problem_with_loops_and_detections, :1156-1213 setup_problem_with_ego_motion, :1668-1712 solve_once; RelativePoseFactor4d,
// DeltaPose, NormalizeAngle, pose_error_4d of swarm_localization_factors.hpp), stated once.  Plain C++ for g++ AND hipcc: pgo.hip gives every start a workgroup,
// pgo_host.cpp and tests/cpp/pgo_plan_pin.cpp run the same functions on one thread; nothing else restates the arithmetic.  The two builds agree BIT FOR BIT, and
// everything that decides a bit is said here: every product and sum rounds on its own (contraction off), IEEE division and square root, floor, and NO library
// transcendental (sine and cosine are sincos_plan() below, the arctangent is pcm::atan2_plan); every sum over edges or poses has ONE order.
//
// Ceres, Eigen and swarm_msgs are not vendored, so parity with the reference is UNPINNED: this header is the specification.  Assumed for swarm_msgs:
// RelativePoseFactor4d::CreateCov6d and LoopEdge::get_sqrt_information_4d reduce, for the diagonal covariances this library keeps, to sqrt_inf = 1 / sqrt(cov) over
// (pos_cov x, y, z, ang_cov[2]) -- sqrt_inf_of_cov() below; a zero covariance gives what IEEE gives (inf), nothing is clamped.
//
// Records.  A pose is double[4] = x y z yaw; a `fixed` byte per pose marks the constant ones.  An edge is omni_pgo_edge {i, j, z[4], sqrt_inf[4], robust}.
//
// Residual of an edge (a = pose i, b = pose j; (s, c) = sincos_plan(a.yaw)):
//   dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z
//   D  = DeltaPose(a, b) = (c dx + s dy,  c dy - s dx,  dz,  N(b.yaw - a.yaw))          N(t) = t - 2 pi floor((t + pi) / (2 pi)), as the reference writes it
//   r  = w o (z.x - D.x,  z.y - D.y,  z.z - D.z,  N(z.yaw - D.yaw))                     w = sqrt_inf; the fourth component is normalised BEFORE it is scaled
// Jacobians (row = residual, column = x y z yaw of the pose), analytic:
//   dr/da = diag(w) [  c   s   0  -D.y ]          dr/db = diag(w) [ -c  -s   0   0 ]
//                   [ -s   c   0   D.x ]                          [  s  -c   0   0 ]
//                   [  0   0   1   0   ]                          [  0   0  -1   0 ]
//                   [  0   0   0   1   ]                          [  0   0   0  -1 ]
//   (d D.x / d a.yaw = -s dx + c dy = D.y, d D.y / d a.yaw = -c dx - s dy = -D.x; N() has slope 1 wherever it is differentiable.)
// Loss.  ss = ((r0^2 + r1^2) + r2^2) + r3^2.  Huber(1) as Ceres' Corrector applies it to a block (rho'' < 0, so alpha = 0): for a robust edge with ss > 1 residual and
// both Jacobians are scaled by k = 1 / sqrt(sqrt(ss)) (w becomes k w) and the edge's cost is (2 sqrt(ss) - 1) / 2; otherwise k = 1 and the cost is ss / 2.
//
// Sums.  plan_graph() builds on the host, per pose, the list of its incident edges in ascending edge index (CSR; an entry is 2 e + side, side 1: the pose is e's j).
// Every per-pose sum (the gradient J^T r, the 4 x 4 diagonal block of J^T J, J^T (J p)) is ONE chain over that list from zero, in that order.  Every scalar sum
// (the cost over edges; dot products over poses, whose entry is the pose's four products added left to right) is reduce(): the entries are cut into chunks of 256
// consecutive ones; a chunk (padded with +0) is summed by the tree  for stride = 128, 64 .. 1: v[l] += v[l + stride] for l < stride;  the chunk sums are added to
// the total in chunk order, starting from 0.  No floating-point atomics anywhere.
//
// Poses that take part: `active` = not fixed and with at least one edge.  A free pose without an edge does not move.  EMPTY: no active pose or no edge.
//
// Solver: Levenberg-Marquardt, the damping lambda diag(J^T J), the step from matrix-free preconditioned conjugate gradients on the normal equations.
//   cost = reduce(edge costs at the poses given); not finite -> NONFINITE.  lambda = initial_lambda, nu = 2.
//   outer iteration (at most max_iterations):
//     g = J^T r, B_p = the diagonal blocks, per active pose
//     try (at most 1 + max_lambda_retries times, with the same g and B):
//       M_p = B_p + lambda diag(B_p), factored L L^T (Cholesky, rows in order; a block that is not positive definite gives NaN and ends NONFINITE)
//       CG on (J^T J + lambda diag(J^T J)) d = -g from d = 0:  r = -g, z = M^-1 r, p = z, rz = r.z, rz0 = rz;  at most max_cg_iterations times:
//         q = J^T (J p) + lambda diag(B) o p;  pq = p.q;  stop unless pq > 0;  alpha = rz / pq;  d += alpha p;  r -= alpha q;  z = M^-1 r;  rz' = r.z;
//         stop if rz' <= cg_tolerance^2 rz0;  beta = rz' / rz;  p = z + beta p;  rz = rz'          (a step counts once alpha was applied)
//       dd = d.d, xx = x.x over active poses.  dd not finite -> NONFINITE.  sqrt(dd) <= parameter_tolerance (sqrt(xx) + parameter_tolerance) -> CONVERGED, the
//         step is not applied.
//       model = reduce over edges of  -(r.u) - (u.u) / 2  with u = J_i d_i + J_j d_j  (the decrease the linearisation promises)
//       cost' = reduce(edge costs at x + d); not finite -> NONFINITE.  rho = (cost - cost') / model.
//       accepted iff model > 0 and rho > 1e-3:  x += d;  lambda = max(lambda max(1/3, 1 - (2 rho - 1)^3), 1e-16);  nu = 2;
//         CONVERGED if cost - cost' <= function_tolerance cost;  next outer iteration.
//       rejected:  lambda = min(lambda nu, 1e32);  nu = 2 nu;  try again.  No try left -> MAX_ITERATIONS.
//   max_iterations outer iterations without a verdict -> MAX_ITERATIONS.
//   max_cg_iterations = 0 means 4 x the number of active poses: block-Jacobi CG needs on the order of the longest chain of the graph, which is why the window is
//   bounded and no whole-mission graph is promised.
//   NONFINITE returns the poses as they came, with final_cost = the offending cost (or, when a step was not finite, the cost of the last accepted poses).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/omni_hip.h"
#include "pcm_plan.h"

#if defined(__HIPCC__)
#define PGO_HD __host__ __device__ inline
#else
#define PGO_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace omni {
namespace pgo {

constexpr int kChunk = 256;           // entries per chunk of reduce(): part of the sum's SHAPE, so changing it changes bits
constexpr int THREADS = 256;          // pgo.hip: lanes of the workgroup that owns a start; how the work is spread, any multiple of 64 computes the same bits
constexpr int kBatch = 8;             // chunks whose trees run between the same barriers (how the work is spread, not what is computed)
constexpr int kRedDoubles = kBatch * kChunk + 2;   // the tree's buffer + two broadcast slots
constexpr int kEdgeFields = 12;       // per edge in a slab: r[4] | k w[4] | c | s | D.x | D.y, structure-of-arrays [12][m]
constexpr double kMinLambda = 1e-16, kMaxLambda = 1e32, kMinRelativeDecrease = 1e-3;

PGO_HD bool finite_plan(double v) { return v - v == 0; }             // false for NaN and +-inf

// ---- trigonometry ------------------------------------------------------------------------------------------------------------------------------------------------
// sincos_plan(x) from + - * /, floor and comparisons.  Reduction to a quadrant: k = floor(x 2/pi + 1/2); y = x - k pi/2 in two Cody-Waite rounds with pi/2 cut into
// 33-bit pieces (hi, lo) pairs P1 + P1T = P1 + P2 + P2T, the constants of fdlibm's __ieee754_rem_pio2 (k P1 and k P2 are exact for |k| < 2^20), the second round
// always taken; y = (y0, y1) with |y0| <= pi/4 (+ an ulp).  Polynomials of fixed degree 13 (sine) and 14 (cosine) in y0 with y1 as the tail, the coefficients and
// the evaluation order of FreeBSD's k_sin.c / k_cos.c.  The quadrant k mod 4 (by floor) picks and signs them.  Accuracy is promised for |x| <= 1e5 (a normalised
// angle is within pi); beyond 2^20 pi/2 the result is still the same on both builds but no longer close.  NaN or inf in, NaN out.
// Largest distance from numpy's sin / cos measured by tests/test_pgo_plan_cpu.py: see there and DESIGN.md 0.2r.
PGO_HD double sin_kernel(double x, double y) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, w = z * z, r = (S2 + z * (S3 + z * S4)) + (z * w) * (S5 + z * S6), v = z * x;
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
PGO_HD double cos_kernel(double x, double y) {
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x, w0 = z * z, r = z * (C1 + z * (C2 + z * C3)) + (w0 * w0) * (C4 + z * (C5 + z * C6)), hz = 0.5 * z, w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * y));
}
PGO_HD void sincos_plan(double x, double* sn, double* cs) {
    if (!finite_plan(x)) { *sn = x - x; *cs = x - x; return; }
    const double INVPIO2 = 6.36619772367581382433e-01, P1 = 1.57079632673412561417e+00, P2 = 6.07710050630396597660e-11, P2T = 2.02226624879595063154e-21;
    const double k = floor(x * INVPIO2 + 0.5);
    const double t = x - k * P1, w1 = k * P2, z = t - w1, w2 = k * P2T - ((t - z) - w1), y0 = z - w2, y1 = (z - y0) - w2;
    const int q = (int)(k - 4.0 * floor(k * 0.25));                  // 0 .. 3
    const double s = sin_kernel(y0, y1), c = cos_kernel(y0, y1);
    *sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    *cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}
PGO_HD double normalize_angle(double a) {                          // NormalizeAngle (swarm_localization_factors.hpp:34-40)
    const double PI = 3.14159265358979323846, TWO_PI = 2.0 * PI;
    return a - TWO_PI * floor((a + PI) / TWO_PI);
}
PGO_HD double yaw_of_quat(double w, double x, double y, double z) {  // quat2eulers' yaw (ZYX) with the arctangent of pcm_plan.h
    return pcm::atan2_plan(2 * (w * z + x * y), 1 - 2 * (y * y + z * z));
}
PGO_HD double sqrt_inf_of_cov(double cov) { return 1.0 / sqrt(cov); }

// DeltaPose(a, b) (swarm_localization_factors.hpp:138-149), 4 DoF
PGO_HD void delta_pose(const double* a, const double* b, double* d) {
    double s, c;
    sincos_plan(a[3], &s, &c);
    const double dx = b[0] - a[0], dy = b[1] - a[1];
    d[0] = c * dx + s * dy; d[1] = c * dy - s * dx; d[2] = b[2] - a[2]; d[3] = normalize_angle(b[3] - a[3]);
}
// PoseMulti(a, b) (:163-172): a . b, for the host's initial values
PGO_HD void pose_mul(const double* a, const double* b, double* o) {
    double s, c;
    sincos_plan(a[3], &s, &c);
    const double x = c * b[0] - s * b[1], y = s * b[0] + c * b[1];
    o[0] = x + a[0]; o[1] = y + a[1]; o[2] = b[2] + a[2]; o[3] = normalize_angle(b[3] + a[3]);
}
PGO_HD void pose_inverse(const double* a, double* o) {              // the pose whose product with a is the identity
    const double zero[4] = {0, 0, 0, 0};
    delta_pose(a, zero, o);
}

// ---- one edge ------------------------------------------------------------------------------------------------------------------------------------------------------
struct EdgeLin { double r[4], w[4], c, s, dx, dy; };                 // what a slab keeps per edge: corrected residual, corrected weights, and what the Jacobians need

PGO_HD double linearize(const omni_pgo_edge& e, const double* x, EdgeLin* o) {      // returns the edge's cost
    const double* a = x + 4 * (size_t)e.i;
    const double* b = x + 4 * (size_t)e.j;
    double d[4];
    sincos_plan(a[3], &o->s, &o->c);
    const double dx = b[0] - a[0], dy = b[1] - a[1];
    d[0] = o->c * dx + o->s * dy; d[1] = o->c * dy - o->s * dx; d[2] = b[2] - a[2]; d[3] = normalize_angle(b[3] - a[3]);
    const double r0 = e.sqrt_inf[0] * (e.z[0] - d[0]), r1 = e.sqrt_inf[1] * (e.z[1] - d[1]), r2 = e.sqrt_inf[2] * (e.z[2] - d[2]),
                 r3 = e.sqrt_inf[3] * normalize_angle(e.z[3] - d[3]);
    const double ss = ((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3;
    double k = 1.0, cost = 0.5 * ss;
    if (e.robust && ss > 1.0) { const double rt = sqrt(ss); k = 1.0 / sqrt(rt); cost = 0.5 * (2.0 * rt - 1.0); }
    o->r[0] = k * r0; o->r[1] = k * r1; o->r[2] = k * r2; o->r[3] = k * r3;
    for (int q = 0; q < 4; ++q) o->w[q] = k * e.sqrt_inf[q];
    o->dx = d[0]; o->dy = d[1];
    return cost;
}
// the Jacobian of side 0 (pose i) or 1 (pose j), row-major [4][4], zeros written out
PGO_HD void jacobian(const EdgeLin& l, int side, double* J) {
    for (int q = 0; q < 16; ++q) J[q] = 0.0;
    if (side == 0) {
        J[0] = l.w[0] * l.c; J[1] = l.w[0] * l.s; J[3] = -(l.w[0] * l.dy);
        J[4] = -(l.w[1] * l.s); J[5] = l.w[1] * l.c; J[7] = l.w[1] * l.dx;
        J[10] = l.w[2]; J[15] = l.w[3];
    } else {
        J[0] = -(l.w[0] * l.c); J[1] = -(l.w[0] * l.s);
        J[4] = l.w[1] * l.s; J[5] = -(l.w[1] * l.c);
        J[10] = -l.w[2]; J[15] = -l.w[3];
    }
}
// u += J_side p is never needed: u = J_i p_i + J_j p_j in one expression per row
PGO_HD void j_times(const EdgeLin& l, const double* pi, const double* pj, double* u) {
    const double ex = pi[0] - pj[0], ey = pi[1] - pj[1];           // rows 0 and 1 see (p_i - p_j) in x and y, and p_i's yaw alone
    u[0] = l.w[0] * ((l.c * ex + l.s * ey) - l.dy * pi[3]);
    u[1] = l.w[1] * ((l.c * ey - l.s * ex) + l.dx * pi[3]);
    u[2] = l.w[2] * (pi[2] - pj[2]);
    u[3] = l.w[3] * (pi[3] - pj[3]);
}
// o = J_side^T v
PGO_HD void jt_times(const EdgeLin& l, int side, const double* v, double* o) {
    const double t0 = l.w[0] * v[0], t1 = l.w[1] * v[1], t2 = l.w[2] * v[2], t3 = l.w[3] * v[3];
    const double ox = l.c * t0 - l.s * t1, oy = l.s * t0 + l.c * t1;
    if (side == 0) { o[0] = ox; o[1] = oy; o[2] = t2; o[3] = (l.dx * t1 - l.dy * t0) + t3; }
    else { o[0] = -ox; o[1] = -oy; o[2] = -t2; o[3] = -t3; }
}

PGO_HD void store_lin(double* E, int m, int e, const EdgeLin& l) {
    for (int q = 0; q < 4; ++q) { E[(size_t)q * m + e] = l.r[q]; E[(size_t)(4 + q) * m + e] = l.w[q]; }
    E[(size_t)8 * m + e] = l.c; E[(size_t)9 * m + e] = l.s; E[(size_t)10 * m + e] = l.dx; E[(size_t)11 * m + e] = l.dy;
}
PGO_HD EdgeLin load_lin(const double* E, int m, int e) {
    EdgeLin l;
    for (int q = 0; q < 4; ++q) { l.r[q] = E[(size_t)q * m + e]; l.w[q] = E[(size_t)(4 + q) * m + e]; }
    l.c = E[(size_t)8 * m + e]; l.s = E[(size_t)9 * m + e]; l.dx = E[(size_t)10 * m + e]; l.dy = E[(size_t)11 * m + e];
    return l;
}

// ---- the 4 x 4 blocks: lower triangles in row order, (r, c) at r (r + 1) / 2 + c -----------------------------------------------------------------------------------
// M = B + lambda diag(B) -> its Cholesky factor with the diagonal stored INVERTED
PGO_HD void factor_block(const double* B, double lambda, double* L) {
    double inv[4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c <= r; ++c) {
            double sum = B[r * (r + 1) / 2 + c];
            if (r == c) sum = sum + lambda * sum;
            for (int k = 0; k < c; ++k) sum -= L[r * (r + 1) / 2 + k] * L[c * (c + 1) / 2 + k];
            if (r == c) { inv[r] = 1.0 / sqrt(sum); L[r * (r + 1) / 2 + r] = inv[r]; }
            else L[r * (r + 1) / 2 + c] = sum * inv[c];
        }
}
PGO_HD void solve_block(const double* L, const double* b, double* z) {
    double y[4];
    for (int r = 0; r < 4; ++r) {
        double sum = b[r];
        for (int k = 0; k < r; ++k) sum -= L[r * (r + 1) / 2 + k] * y[k];
        y[r] = sum * L[r * (r + 1) / 2 + r];
    }
    for (int r = 3; r >= 0; --r) {
        double sum = y[r];
        for (int k = 3; k > r; --k) sum -= L[k * (k + 1) / 2 + r] * z[k];
        z[r] = sum * L[r * (r + 1) / 2 + r];
    }
}
PGO_HD double dot4(const double* a, const double* b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// ---- refusals and the plan of a graph (host) -----------------------------------------------------------------------------------------------------------------------
inline const char* params_refusal(const omni_pgo_params& p) {
    if (p.max_iterations < 0 || p.max_cg_iterations < 0 || p.max_lambda_retries < 0) return "a negative cap";
    if (!(p.initial_lambda > 0) || !finite_plan(p.initial_lambda)) return "initial_lambda is not positive and finite";
    if (!(p.function_tolerance >= 0) || !finite_plan(p.function_tolerance)) return "function_tolerance is negative or not finite";
    if (!(p.parameter_tolerance >= 0) || !finite_plan(p.parameter_tolerance)) return "parameter_tolerance is negative or not finite";
    if (!(p.cg_tolerance >= 0) || !finite_plan(p.cg_tolerance)) return "cg_tolerance is negative or not finite";
    return nullptr;
}
inline const char* graph_refusal(const omni_pgo_edge* edges, int n_poses, int n_edges) {
    if (n_poses < 1 || n_poses > OMNI_PGO_MAX_POSES) return "n_poses outside 1..4096";
    if (n_edges < 0 || n_edges > OMNI_PGO_MAX_EDGES) return "n_edges outside 0..16384";
    for (int e = 0; e < n_edges; ++e) {
        if (edges[e].i < 0 || edges[e].i >= n_poses || edges[e].j < 0 || edges[e].j >= n_poses) return "an edge names a pose outside the graph";
        if (edges[e].i == edges[e].j) return "an edge joins a pose with itself";
    }
    return nullptr;
}
inline const char* starts_refusal(int n_starts) { return n_starts < 1 || n_starts > OMNI_PGO_MAX_STARTS ? "n_starts outside 1..64" : nullptr; }
inline omni_pgo_params default_params() {
    omni_pgo_params p;
    p.max_iterations = 50; p.max_cg_iterations = 0; p.max_lambda_retries = 16; p.reserved = 0;
    p.initial_lambda = 1e-4; p.function_tolerance = 1e-6; p.parameter_tolerance = 1e-8; p.cg_tolerance = 1e-6;
    return p;
}
// offsets [n + 1], incident [2 m], active [n]; returns the number of active poses.  The graph has passed graph_refusal().
inline int plan_graph(const uint8_t* fixed, const omni_pgo_edge* edges, int n, int m, int32_t* offsets, int32_t* incident, uint8_t* active) {
    for (int p = 0; p <= n; ++p) offsets[p] = 0;
    for (int e = 0; e < m; ++e) { ++offsets[edges[e].i + 1]; ++offsets[edges[e].j + 1]; }
    for (int p = 0; p < n; ++p) offsets[p + 1] += offsets[p];
    int n_active = 0;
    for (int p = 0; p < n; ++p) { active[p] = !fixed[p] && offsets[p + 1] > offsets[p]; n_active += active[p]; }
    // ascending edge index per pose: the edges are visited in order, offsets[p] is pose p's cursor while the lists fill and is moved back afterwards
    for (int e = 0; e < m; ++e) { incident[offsets[edges[e].i]++] = 2 * e; incident[offsets[edges[e].j]++] = 2 * e + 1; }
    for (int p = n; p > 0; --p) offsets[p] = offsets[p - 1];
    offsets[0] = 0;
    return n_active;
}

// ---- a start's slab ------------------------------------------------------------------------------------------------------------------------------------------------
struct Graph {
    int n, m, n_active;
    const omni_pgo_edge* edges;
    const uint8_t* active;
    const int32_t* offsets;
    const int32_t* incident;
};
// per pose: x xc g d rr z p q dg [4] each, B L [10] each; per edge: E0 E1 [12], u [4]
PGO_HD size_t slab_doubles(int n, int m) { return (size_t)(9 * 4 + 20) * n + (size_t)(2 * kEdgeFields + 4) * m; }

// A team: tid() of size() lanes walk items tid, tid + size, ..; sync() separates phases; red points at kRedDoubles doubles all lanes see.  The host's team is one
// lane and no barrier.
struct HostTeam {
    double* red;
    PGO_HD int tid() const { return 0; }
    PGO_HD int size() const { return 1; }
    PGO_HD void sync() const {}
};

// The fixed-shape sum of entry(0) .. entry(count - 1); entry(k) is called exactly once, by one lane, so it may store what it computed on the way.  Every lane returns
// the total.
template <class Team, class F>
PGO_HD double reduce(const Team& t, int count, F entry) {
    double total = 0.0;                                              // lane 0's copy is the one that counts
    for (int base = 0; base < count; base += kBatch * kChunk) {
        const int left = count - base, chunks = left >= kBatch * kChunk ? kBatch : (left + kChunk - 1) / kChunk;
        for (int k = t.tid(); k < chunks * kChunk; k += t.size()) t.red[k] = k < left ? entry(base + k) : 0.0;
        t.sync();
        for (int stride = kChunk / 2; stride >= 1; stride >>= 1) {
            for (int k = t.tid(); k < chunks * stride; k += t.size()) {
                const int c = k / stride, l = k - c * stride;
                t.red[c * kChunk + l] = t.red[c * kChunk + l] + t.red[c * kChunk + l + stride];
            }
            t.sync();
        }
        if (t.tid() == 0) for (int c = 0; c < chunks; ++c) total = total + t.red[c * kChunk];
        t.sync();
    }
    if (t.tid() == 0) t.red[kBatch * kChunk] = total;
    t.sync();
    total = t.red[kBatch * kChunk];
    t.sync();
    return total;
}

// One start.  x_in / x_out [n][4] (may not alias the slab); slab: slab_doubles(n, m) doubles owned by this team.
template <class Team>
PGO_HD void solve_team(const Team& t, const Graph& G, const omni_pgo_params& pr, const double* x_in, double* slab, double* x_out, omni_pgo_stats* st) {
    const int n = G.n, m = G.m;
    const size_t n4 = (size_t)4 * n;
    double *x = slab, *xc = x + n4, *g = xc + n4, *d = g + n4, *rr = d + n4, *z = rr + n4, *p = z + n4, *q = p + n4, *dg = q + n4, *B = dg + n4, *L = B + (size_t)10 * n,
           *E0 = L + (size_t)10 * n, *E1 = E0 + (size_t)kEdgeFields * m, *u = E1 + (size_t)kEdgeFields * m;
    const int max_cg = pr.max_cg_iterations > 0 ? pr.max_cg_iterations : 4 * G.n_active;
    int status = OMNI_PGO_MAX_ITERATIONS, iterations = 0, cg_total = 0;
    double cost0 = 0.0, cost = 0.0;

    for (size_t k = t.tid(); k < n4; k += t.size()) { x[k] = x_in[k]; x_out[k] = x_in[k]; }
    t.sync();
    if (G.n_active == 0 || m == 0) {
        if (t.tid() == 0) { st->initial_cost = 0.0; st->final_cost = 0.0; st->iterations = 0; st->cg_iterations = 0; st->status = OMNI_PGO_EMPTY; st->reserved = 0; }
        return;
    }
    cost0 = cost = reduce(t, m, [&](int e) { EdgeLin l; const double c = linearize(G.edges[e], x, &l); store_lin(E0, m, e, l); return c; });
    bool nonfinite = !finite_plan(cost), done = nonfinite;
    double lambda = pr.initial_lambda, nu = 2.0;

    for (int it = 0; it < pr.max_iterations && !done; ++it) {
        iterations = it + 1;
        // the gradient and the diagonal blocks: one chain per pose over its incident edges
        for (int v = t.tid(); v < n; v += t.size()) {
            double gv[4] = {0, 0, 0, 0}, Bv[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (G.active[v])
                for (int k = G.offsets[v]; k < G.offsets[v + 1]; ++k) {
                    const int e = G.incident[k] >> 1, side = G.incident[k] & 1;
                    const EdgeLin l = load_lin(E0, m, e);
                    double J[16];
                    jacobian(l, side, J);
                    for (int c = 0; c < 4; ++c) gv[c] += ((J[c] * l.r[0] + J[4 + c] * l.r[1]) + J[8 + c] * l.r[2]) + J[12 + c] * l.r[3];
                    for (int r = 0; r < 4; ++r)
                        for (int c = 0; c <= r; ++c) Bv[r * (r + 1) / 2 + c] += ((J[r] * J[c] + J[4 + r] * J[4 + c]) + J[8 + r] * J[8 + c]) + J[12 + r] * J[12 + c];
                }
            for (int c = 0; c < 4; ++c) { g[4 * (size_t)v + c] = gv[c]; dg[4 * (size_t)v + c] = Bv[c * (c + 1) / 2 + c]; }
            for (int c = 0; c < 10; ++c) B[10 * (size_t)v + c] = Bv[c];
        }
        t.sync();

        bool accepted = false;
        for (int attempt = 0; attempt <= pr.max_lambda_retries && !done && !accepted; ++attempt) {
            // the preconditioner and the first CG vectors
            double rz = reduce(t, n, [&](int v) {
                double* dv = d + 4 * (size_t)v; double* rv = rr + 4 * (size_t)v; double* zv = z + 4 * (size_t)v; double* pv = p + 4 * (size_t)v;
                for (int c = 0; c < 4; ++c) { dv[c] = 0.0; rv[c] = 0.0; zv[c] = 0.0; pv[c] = 0.0; }
                if (!G.active[v]) return 0.0;
                factor_block(B + 10 * (size_t)v, lambda, L + 10 * (size_t)v);
                for (int c = 0; c < 4; ++c) rv[c] = -g[4 * (size_t)v + c];
                solve_block(L + 10 * (size_t)v, rv, zv);
                for (int c = 0; c < 4; ++c) pv[c] = zv[c];
                return dot4(rv, zv);
            });
            const double rz_stop = (pr.cg_tolerance * pr.cg_tolerance) * rz;
            for (int k = 0; k < max_cg; ++k) {
                for (int e = t.tid(); e < m; e += t.size()) {
                    const EdgeLin l = load_lin(E0, m, e);
                    double ue[4];
                    j_times(l, p + 4 * (size_t)G.edges[e].i, p + 4 * (size_t)G.edges[e].j, ue);
                    for (int c = 0; c < 4; ++c) u[(size_t)c * m + e] = ue[c];
                }
                t.sync();
                const double pq = reduce(t, n, [&](int v) {
                    double* qv = q + 4 * (size_t)v;
                    double acc[4] = {0, 0, 0, 0};
                    if (!G.active[v]) { for (int c = 0; c < 4; ++c) qv[c] = 0.0; return 0.0; }
                    for (int kk = G.offsets[v]; kk < G.offsets[v + 1]; ++kk) {
                        const int e = G.incident[kk] >> 1, side = G.incident[kk] & 1;
                        const EdgeLin l = load_lin(E0, m, e);
                        const double ue[4] = {u[e], u[(size_t)m + e], u[(size_t)2 * m + e], u[(size_t)3 * m + e]};
                        double o[4];
                        jt_times(l, side, ue, o);
                        for (int c = 0; c < 4; ++c) acc[c] += o[c];
                    }
                    const double* pv = p + 4 * (size_t)v;
                    for (int c = 0; c < 4; ++c) qv[c] = acc[c] + (lambda * dg[4 * (size_t)v + c]) * pv[c];
                    return dot4(pv, qv);
                });
                if (!(pq > 0.0)) break;
                const double alpha = rz / pq;
                ++cg_total;
                const double rz_new = reduce(t, n, [&](int v) {
                    if (!G.active[v]) return 0.0;
                    double* dv = d + 4 * (size_t)v; double* rv = rr + 4 * (size_t)v; double* zv = z + 4 * (size_t)v;
                    const double* pv = p + 4 * (size_t)v; const double* qv = q + 4 * (size_t)v;
                    for (int c = 0; c < 4; ++c) { dv[c] = dv[c] + alpha * pv[c]; rv[c] = rv[c] - alpha * qv[c]; }
                    solve_block(L + 10 * (size_t)v, rv, zv);
                    return dot4(rv, zv);
                });
                if (rz_new <= rz_stop) break;
                const double beta = rz_new / rz;
                for (int v = t.tid(); v < n; v += t.size())
                    if (G.active[v]) for (int c = 0; c < 4; ++c) p[4 * (size_t)v + c] = z[4 * (size_t)v + c] + beta * p[4 * (size_t)v + c];
                t.sync();
                rz = rz_new;
            }
            // the step's size; the candidate poses
            const double dd = reduce(t, n, [&](int v) {
                for (int c = 0; c < 4; ++c) xc[4 * (size_t)v + c] = x[4 * (size_t)v + c] + d[4 * (size_t)v + c];
                return G.active[v] ? dot4(d + 4 * (size_t)v, d + 4 * (size_t)v) : 0.0;
            });
            const double xx = reduce(t, n, [&](int v) { return G.active[v] ? dot4(x + 4 * (size_t)v, x + 4 * (size_t)v) : 0.0; });
            if (!finite_plan(dd)) { nonfinite = done = true; break; }
            if (sqrt(dd) <= pr.parameter_tolerance * (sqrt(xx) + pr.parameter_tolerance)) { status = OMNI_PGO_CONVERGED; done = true; break; }
            const double model = reduce(t, m, [&](int e) {
                const EdgeLin l = load_lin(E0, m, e);
                double ue[4];
                j_times(l, d + 4 * (size_t)G.edges[e].i, d + 4 * (size_t)G.edges[e].j, ue);
                return -dot4(l.r, ue) - 0.5 * dot4(ue, ue);
            });
            const double cost_new = reduce(t, m, [&](int e) { EdgeLin l; const double c = linearize(G.edges[e], xc, &l); store_lin(E1, m, e, l); return c; });
            if (!finite_plan(cost_new)) { cost = cost_new; nonfinite = done = true; break; }
            const double rho = (cost - cost_new) / model;
            if (model > 0.0 && rho > kMinRelativeDecrease) {
                accepted = true;
                double* sw = x; x = xc; xc = sw;
                sw = E0; E0 = E1; E1 = sw;
                const double tt = 2.0 * rho - 1.0, f = 1.0 - (tt * tt) * tt, scaled = lambda * (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
                lambda = scaled > kMinLambda ? scaled : kMinLambda;
                nu = 2.0;
                const double decrease = cost - cost_new;
                if (decrease <= pr.function_tolerance * cost) { status = OMNI_PGO_CONVERGED; done = true; }
                cost = cost_new;
            } else {
                const double grown = lambda * nu;
                lambda = grown < kMaxLambda ? grown : kMaxLambda;
                nu = 2.0 * nu;
            }
        }
        if (!accepted && !done) done = true;                        // no try left: MAX_ITERATIONS
    }
    if (nonfinite) status = OMNI_PGO_NONFINITE;
    else {
        for (size_t k = t.tid(); k < n4; k += t.size()) x_out[k] = x[k];
    }
    if (t.tid() == 0) {
        st->initial_cost = cost0; st->final_cost = cost; st->iterations = iterations; st->cg_iterations = cg_total; st->status = status; st->reserved = 0;
    }
}

// the cheapest start among those that ended CONVERGED or MAX_ITERATIONS, the lower index on a tie; -1 when there is none
inline int pick_best(const omni_pgo_stats* st, int n_starts) {
    int best = -1;
    for (int k = 0; k < n_starts; ++k) {
        if (st[k].status != OMNI_PGO_CONVERGED && st[k].status != OMNI_PGO_MAX_ITERATIONS) continue;
        if (best < 0 || st[k].final_cost < st[best].final_cost) best = k;
    }
    return best;
}

// ---- the host build: every start on the calling thread ---------------------------------------------------------------------------------------------------------------
// poses_in / poses_out [n_starts][n][4], fixed [n], edges [m], stats [n_starts].  Returns a refusal or null.
inline const char* solve_host(const omni_pgo_params& pr, const double* poses_in, const uint8_t* fixed, const omni_pgo_edge* edges, int n, int m, int n_starts,
                              double* poses_out, omni_pgo_stats* stats, int* best) {
    const char* why = graph_refusal(edges, n, m);
    if (!why) why = starts_refusal(n_starts);
    if (!why) why = params_refusal(pr);
    if (why) return why;
    std::vector<int32_t> offsets((size_t)n + 1), incident((size_t)2 * m);
    std::vector<uint8_t> active((size_t)n);
    std::vector<double> slab(slab_doubles(n, m)), red((size_t)kRedDoubles);
    Graph G;
    G.n = n; G.m = m; G.edges = edges; G.active = active.data(); G.offsets = offsets.data(); G.incident = incident.data();
    G.n_active = plan_graph(fixed, edges, n, m, offsets.data(), incident.data(), active.data());
    HostTeam team;
    team.red = red.data();
    for (int k = 0; k < n_starts; ++k) solve_team(team, G, pr, poses_in + (size_t)k * 4 * n, slab.data(), poses_out + (size_t)k * 4 * n, stats + k);
    *best = pick_best(stats, n_starts);
    return nullptr;
}

}  // namespace pgo
}  // namespace omni
