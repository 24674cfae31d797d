// pcm_plan.h -- pairwise consistency maximisation of loop edges (SwarmLocalOutlierRejection::OutlierRejectionLoopEdgesPCM, swarm_localization/src/
// swarm_outlier_rejection/swarm_outlier_rejection.cpp:173-298), stated once.  Plain C++ for g++ AND hipcc: pcm.hip gives every pair of edges a lane, pcm_host.cpp and
// tests/cpp/pcm_plan_pin.cpp run the same functions on the host; nothing else restates the arithmetic.  Every product and sum rounds on its own (contraction off),
// IEEE division and square root, and NO library transcendental: the log map's arctangent is atan2_plan() below, built from + - * / alone, because glibc's and the
// device library's need not agree in the last bit.
//
// swarm_msgs (Swarm::Pose, DroneTrajectory::get_relative_pose_by_ts, LoopEdge::same_robot_pair, computeSquaredMahalanobisDistance) is not vendored, so parity with
// the reference is UNPINNED: this header is the specification.  What it restates, on edge records that carry what the reference looks up by time stamp:
//   same_robot_pair   1: e2 joins the same drones in the same order as e1 (an edge of one drone with itself gives 1), 2: swapped, 0: other drones (no verdict)
//   per pair (:188-236)
//     p2      = e2's relative pose, inverted when swapped
//     odom_a  = inverse(P_a(e1)) * P_a(e2), odom_b likewise, from the SELF POSES the edges carry (swapped: e2's self_pose_b / self_pose_a) -- the reference asks
//               its ego-motion trajectory for the relative pose between the two stamps
//     err     = odom_a * p2 * inverse(odom_b) * inverse(p1), composed left to right
//     v       = (err's translation, err's rotation vector): the log map of LoopGeometry::check_loop_odometry_consistency -- sign flip to w >= 0,
//               k = vn > 1e-12 ? ang / vn : 2
//     c       = (cov(e1) + cov(e2)) + (cov(odom_a) + cov(odom_b)), diagonals; cov(odom) = |arc(e2) - arc(e1)| * (pos_covariance_per_meter x3,
//               yaw_covariance_per_meter x3) with the cumulative path lengths the edges carry
//     smd     = sum v_i^2 / c_i, i = 0 .. 5 in order
//     consistent iff smd < pcm_thres.  A zero covariance gives what IEEE gives (0/0 = NaN: not consistent; x/0 = inf: not consistent); nothing is clamped.
//   Quaternions are taken as they come (unit, as geom::Pose holds them); a composition normalises its product as geom::Pose::operator* does.
//
// The clique rule (the heuristic of FMC::maxCliqueHeu in words, written from scratch on bitset rows): vertices are visited in index order; a vertex whose degree is
// below the best size so far is skipped; otherwise S = its neighbours whose degree is at least the best size; repeatedly the HIGHEST-indexed member u of S joins the
// clique and S = S & N(u) & {degree >= best size}; the clique is the start vertex plus the picks; a strictly larger clique replaces the best.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define PCM_HD __host__ __device__ inline
#else
#define PCM_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace omni {
namespace pcm {

constexpr int kFields = 29;       // doubles per edge in the structure-of-arrays: relative_pose 7 | self_pose_a 7 | self_pose_b 7 | arc_a arc_b | pos_cov 3 | ang_cov 3
constexpr int THREADS = 256;      // pcm.hip: four waves, one row word each

struct Pose { double px, py, pz, w, x, y, z; };
struct Edge { int a, b; Pose rel, sa, sb; double arc_a, arc_b, cov[6]; };

PCM_HD Pose pose7(const double* p) { return {p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }
PCM_HD Edge load(const omni_pcm_edge& e) {
    Edge r;
    r.a = e.drone_a; r.b = e.drone_b; r.rel = pose7(e.relative_pose); r.sa = pose7(e.self_pose_a); r.sb = pose7(e.self_pose_b); r.arc_a = e.arc_a; r.arc_b = e.arc_b;
    for (int k = 0; k < 3; ++k) { r.cov[k] = e.pos_cov[k]; r.cov[3 + k] = e.ang_cov[k]; }
    return r;
}
// field f of edge e of the structure-of-arrays F [kFields][cap], drones D [2][cap]
PCM_HD void store_soa(double* F, int* D, int cap, int e, const omni_pcm_edge& s) {
    for (int k = 0; k < 7; ++k) { F[(size_t)k * cap + e] = s.relative_pose[k]; F[(size_t)(7 + k) * cap + e] = s.self_pose_a[k]; F[(size_t)(14 + k) * cap + e] = s.self_pose_b[k]; }
    F[(size_t)21 * cap + e] = s.arc_a; F[(size_t)22 * cap + e] = s.arc_b;
    for (int k = 0; k < 3; ++k) { F[(size_t)(23 + k) * cap + e] = s.pos_cov[k]; F[(size_t)(26 + k) * cap + e] = s.ang_cov[k]; }
    D[e] = s.drone_a; D[cap + e] = s.drone_b;
}
PCM_HD Pose pose_soa(const double* F, int cap, int e, int f0) {
    return {F[(size_t)f0 * cap + e], F[(size_t)(f0 + 1) * cap + e], F[(size_t)(f0 + 2) * cap + e], F[(size_t)(f0 + 3) * cap + e], F[(size_t)(f0 + 4) * cap + e],
            F[(size_t)(f0 + 5) * cap + e], F[(size_t)(f0 + 6) * cap + e]};
}
PCM_HD Edge load_soa(const double* F, const int* D, int cap, int e) {
    Edge r;
    r.a = D[e]; r.b = D[cap + e]; r.rel = pose_soa(F, cap, e, 0); r.sa = pose_soa(F, cap, e, 7); r.sb = pose_soa(F, cap, e, 14);
    r.arc_a = F[(size_t)21 * cap + e]; r.arc_b = F[(size_t)22 * cap + e];
    for (int k = 0; k < 6; ++k) r.cov[k] = F[(size_t)(23 + k) * cap + e];
    return r;
}

PCM_HD int same_robot_pair(int a1, int b1, int a2, int b2) { return a1 == a2 && b1 == b2 ? 1 : (a1 == b2 && b1 == a2 ? 2 : 0); }

// ---- poses: geom::Quat / geom::Pose of host/geometry.hpp, operation by operation ---------------------------------------------------------------------------------
PCM_HD void rotate(const Pose& q, double vx, double vy, double vz, double& ox, double& oy, double& oz) {       // Quat::R() * v
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z, twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y,
                 tyz = tz * q.y, tzz = tz * q.z;
    ox = (1 - (tyy + tzz)) * vx + (txy - twz) * vy + (txz + twy) * vz;
    oy = (txy + twz) * vx + (1 - (txx + tzz)) * vy + (tyz - twx) * vz;
    oz = (txz - twy) * vx + (tyz + twx) * vy + (1 - (txx + tyy)) * vz;
}
PCM_HD Pose mul(const Pose& a, const Pose& b) {                     // Pose::operator*: {pos + att * o.pos, (att * o.att).normalized()}
    Pose r;
    double rx, ry, rz;
    rotate(a, b.px, b.py, b.pz, rx, ry, rz);
    r.px = a.px + rx; r.py = a.py + ry; r.pz = a.pz + rz;
    const double w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
                 z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    const double n = sqrt(w * w + x * x + y * y + z * z);
    r.w = w / n; r.x = x / n; r.y = y / n; r.z = z / n;
    return r;
}
PCM_HD Pose inverse(const Pose& a) {                                // Pose::inverse: {-1.0 * (qi * pos), qi}
    Pose r;
    r.px = 0; r.py = 0; r.pz = 0; r.w = a.w; r.x = -a.x; r.y = -a.y; r.z = -a.z;
    double rx, ry, rz;
    rotate(r, a.px, a.py, a.pz, rx, ry, rz);
    r.px = -1.0 * rx; r.py = -1.0 * ry; r.pz = -1.0 * rz;
    return r;
}

// ---- the arctangent ----------------------------------------------------------------------------------------------------------------------------------------------
// atan2_plan(y, x) from + - * / and comparisons.  Reduction: t = min(|x|, |y|) / max(|x|, |y|) in [0, 1]; c = the nearest of 0, 1/4, 1/2, 3/4, 1 (exact in binary);
// z = (t - c) / (1 + t * c), |z| <= 1/8; atan(t) = atan(c) + atan(z) with atan(c) as a (hi, lo) pair and atan(z) = z - z^3/3 + ... - z^19/19 (ten terms of the
// series: the first one left out is below 2^-66 of z).  Then pi/2 - r when |y| > |x|, pi - r when x is negative, the sign of y; pi/2 and pi as (hi, lo) pairs.
// Largest distance from numpy's arctan2 (glibc) measured by tests/test_pcm_plan_cpu.py: see there and DESIGN.md 0.2q.
PCM_HD double atan_poly(double z) {
    const double s = z * z;
    double p = -1.0 / 19.0;
    p = 1.0 / 17.0 + s * p; p = -1.0 / 15.0 + s * p; p = 1.0 / 13.0 + s * p; p = -1.0 / 11.0 + s * p; p = 1.0 / 9.0 + s * p; p = -1.0 / 7.0 + s * p; p = 1.0 / 5.0 + s * p;
    p = -1.0 / 3.0 + s * p;
    return z + z * (s * p);
}
PCM_HD double atan2_plan(double y, double x) {
    if (x != x || y != y) return x + y;                                               // NaN in, NaN out
    const bool neg_x = __builtin_signbit(x) != 0, neg_y = __builtin_signbit(y) != 0;
    const double ax = neg_x ? -x : x, ay = neg_y ? -y : y;
    const bool swap = ay > ax;
    const double lo = swap ? ax : ay, hi = swap ? ay : ax;
    const double inf = __builtin_huge_val();
    double t;
    if (hi == 0) t = 0;                                                              // atan2(+-0, +-0): 0 or pi
    else if (lo == inf) t = 1;                                                       // both infinite: pi/4
    else t = lo / hi;
    const int ci = (int)(t * 4 + 0.5);                                               // 0 .. 4
    const double c = ci * 0.25;
    const double z = (t - c) / (1 + t * c);
    const double bh = ci == 0 ? 0.0 : ci == 1 ? 0x1.f5b75f92c80ddp-3 : ci == 2 ? 0x1.dac670561bb4fp-2 : ci == 3 ? 0x1.4978fa3269ee1p-1 : 0x1.921fb54442d18p-1;
    const double bl = ci == 0 ? 0.0 : ci == 1 ? 0x1.8ab6e3cf7afbdp-57 : ci == 2 ? 0x1.a2b7f222f65e2p-56 : ci == 3 ? 0x1.2419a87f2a458p-56 : 0x1.1a62633145c07p-55;
    double r = bh + (atan_poly(z) + bl);
    if (swap) r = 0x1.921fb54442d18p+0 - (r - 0x1.1a62633145c07p-54);
    if (neg_x) r = 0x1.921fb54442d18p+1 - (r - 0x1.1a62633145c07p-53);
    return neg_y ? -r : r;
}

// ---- one pair ----------------------------------------------------------------------------------------------------------------------------------------------------
// e1 = the NEW edge, e2 = an earlier one.  Returns same_robot_pair; *smd is written when it is not 0.
PCM_HD int pair_smd(const Edge& e1, const Edge& e2, double pos_per_m, double yaw_per_m, double* smd) {
    const int orient = same_robot_pair(e1.a, e1.b, e2.a, e2.b);
    if (orient == 0) return 0;
    const bool sw = orient == 2;
    const Pose p2 = sw ? inverse(e2.rel) : e2.rel;
    const Pose a2 = sw ? e2.sb : e2.sa, b2 = sw ? e2.sa : e2.sb;
    const double arc_a2 = sw ? e2.arc_b : e2.arc_a, arc_b2 = sw ? e2.arc_a : e2.arc_b;
    const Pose odom_a = mul(inverse(e1.sa), a2), odom_b = mul(inverse(e1.sb), b2);
    const Pose err = mul(mul(mul(odom_a, p2), inverse(odom_b)), inverse(e1.rel));
    const bool flip = err.w < 0;
    const double qw = flip ? -err.w : err.w, qx = flip ? -err.x : err.x, qy = flip ? -err.y : err.y, qz = flip ? -err.z : err.z;
    const double vn = sqrt(qx * qx + qy * qy + qz * qz), ang = 2 * atan2_plan(vn, qw), k = vn > 1e-12 ? ang / vn : 2.0;
    const double v[6] = {err.px, err.py, err.pz, k * qx, k * qy, k * qz};
    const double la = fabs(arc_a2 - e1.arc_a), lb = fabs(arc_b2 - e1.arc_b);
    double s = 0;
    for (int i = 0; i < 6; ++i) {
        const double per = i < 3 ? pos_per_m : yaw_per_m;
        const double c = (e1.cov[i] + e2.cov[i]) + (la * per + lb * per);
        s += v[i] * v[i] / c;
    }
    *smd = s;
    return orient;
}
PCM_HD bool consistent(int orient, double smd, double thres) { return orient != 0 && smd < thres; }

// ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
inline const char* capacity_refusal(int capacity) {
    if (capacity < OMNI_PCM_MIN_CAPACITY || capacity > OMNI_PCM_MAX_CAPACITY) return "capacity outside 64..32768";
    if (capacity % 64) return "capacity is no multiple of 64";
    return nullptr;
}

// ---- the rows on the host: what the kernels compute ----------------------------------------------------------------------------------------------------------------
// edges [n_total]; vertices [first, n_total) are new.  rows [n_total - first][stride] (zeroed here), degree_add [n_total] (zeroed here), smd (may be null)
// [n_total - first][n_total].
inline void rows_host(const omni_pcm_edge* edges, int n_total, int first, const omni_pcm_params& pr, int stride, uint64_t* rows, int32_t* degree_add, double* smd_out) {
    for (size_t k = 0; k < (size_t)(n_total - first) * stride; ++k) rows[k] = 0;
    for (int k = 0; k < n_total; ++k) degree_add[k] = 0;
    if (smd_out) for (size_t k = 0; k < (size_t)(n_total - first) * n_total; ++k) smd_out[k] = 0;
    for (int i = first; i < n_total; ++i) {
        const Edge e1 = load(edges[i]);
        for (int j = 0; j < i; ++j) {
            double smd = 0;
            const int orient = pair_smd(e1, load(edges[j]), pr.pos_covariance_per_meter, pr.yaw_covariance_per_meter, &smd);
            if (smd_out && orient) smd_out[(size_t)(i - first) * n_total + j] = smd;
            if (!consistent(orient, smd, pr.pcm_thres)) continue;
            rows[(size_t)(i - first) * stride + (j >> 6)] |= 1ull << (j & 63);
            if (j >= first) rows[(size_t)(j - first) * stride + (i >> 6)] |= 1ull << (i & 63);
            ++degree_add[i]; ++degree_add[j];
        }
    }
}

// ---- the clique heuristic ------------------------------------------------------------------------------------------------------------------------------------------
// rows: n vertices, row v at rows + v * stride, bits >= n zero, diagonal zero.  work: 2 * stride words.  deg [n]: filled here (popcounts).  Returns the size; clique
// [n] holds the vertices, the start vertex first, then the picks in the order taken.
inline int highest_bit(const uint64_t* s, int words) {
    for (int w = words - 1; w >= 0; --w) if (s[w]) return w * 64 + 63 - __builtin_clzll(s[w]);
    return -1;
}
inline int max_clique(const uint64_t* rows, int n, int stride, int32_t* deg, uint64_t* work, int32_t* clique, int32_t* cur) {
    const int words = (n + 63) / 64;
    uint64_t *S = work, *E = work + stride;
    for (int v = 0; v < n; ++v) { int d = 0; for (int w = 0; w < words; ++w) d += __builtin_popcountll(rows[(size_t)v * stride + w]); deg[v] = d; }
    int best = 0, e_for = -1;
    for (int v = 0; v < n; ++v) {
        if (deg[v] < best) continue;
        if (e_for != best) {                                        // E = {degree >= best}: rebuilt when the best size changed
            for (int w = 0; w < words; ++w) E[w] = 0;
            for (int u = 0; u < n; ++u) if (deg[u] >= best) E[u >> 6] |= 1ull << (u & 63);
            e_for = best;
        }
        for (int w = 0; w < words; ++w) S[w] = rows[(size_t)v * stride + w] & E[w];
        int size = 0;
        cur[size++] = v;
        for (int u = highest_bit(S, words); u >= 0; u = highest_bit(S, words)) {
            cur[size++] = u;
            for (int w = 0; w < words; ++w) S[w] &= rows[(size_t)u * stride + w] & E[w];
        }
        if (size > best) { best = size; for (int k = 0; k < size; ++k) clique[k] = cur[k]; }
    }
    return best;
}

}  // namespace pcm
}  // namespace omni
