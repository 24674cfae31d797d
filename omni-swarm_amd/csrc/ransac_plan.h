// ransac_plan.h -- the homography RANSAC of compute_correspond_features (swarm_loop/src/loop_detector.cpp:574-598: the 3-D-flag filter, then
// cv::findHomography(old_2d, new_2d, RANSAC, 3, mask)), stated once: the operations of host/geometry.hpp (CvRng, ransac_run's getSubset loop,
// HomographyModel::collinear / check_subset / run_kernel / error, jacobi_eigen<9>) in the same order.  Plain C++ for g++ AND hipcc: homography.hip spreads
// these functions over lanes, tests/cpp/ransac_plan_pin.cpp runs them on the host and compares them with geom::find_homography_ransac; nothing else restates
// the arithmetic.  Every product and sum rounds on its own (contraction off), IEEE division and square root.
//
// The serial loop of ransac_run, taken apart (what makes a parallel form give the SAME result):
//   subsets     getSubset consumes the CvRng stream (seed (uint64)-1) and calls check_subset, which reads only the points: iteration k's subset is the
//               k-th ATTEMPT (four distinct indices, redrawn until distinct) that passes check_subset, whatever the models were.  Gen below walks the
//               stream attempt by attempt; check_subset of different attempts is independent.
//   hypotheses  run_kernel and the inlier count good[k] (-1 when run_kernel fails) depend on the subset alone.
//   stop rule   niters = RANSACUpdateNumIters(conf, (count - good) / count, 4, niters) == min(T[good], niters) with T[g] = the same function at
//               max_iters = 2000 (update_num_iters below; exhaustively equal, tests/test_ransac_plan_cpu.py).  The host fills T with its own pow / log:
//               no transcendental is evaluated on the device.  The scan over good[] is integer work.
//   mask        only the best model's: recomputed from the best H at the end.
//   rounds      subsets for the next R iterations, their R hypotheses, then the scan, until the scan's niters is reached.  R changes nothing but the
//               amount of work thrown away.
// Only the eigenvector of the SMALLEST eigenvalue is read: the arg-min of the diagonal replaces jacobi_eigen's sort.  Equal where the smallest eigenvalue is
// unique; ties are counted (*ties) and stay outside what the tests gate.
//
// Statuses (OMNI_HG_* of omni_hip.h):
//   UNFILTERED  count < 4: no homography is asked for; the caller keeps the flagged matches (compute_correspond_features returns false).
//   OK          mask = the inliers of the best model, H = that model.
//   NO_MODEL    find_homography_ransac's `false`: mask all 0.  count == 4 with a failing run_kernel; no model with more than 3 inliers; count <= kEnumMax
//               and NO ordered 4-subset passes check_subset (the host then spends its 10 000 attempts in iteration 0 and returns false: decided here by
//               looking at all of them, at most 360).
//   HOST        given up: an iteration that ransac_run would execute needed more than kAttemptBudget attempts, or the stream position passed kDrawBudget
//               draws.  The caller runs geom::find_homography_ransac for this pair.  Both budgets are 3 to 4 times what non-degenerate input needed in a
//               seeded search (75 attempts, 64 240 draws); they exist so that duplicated or collinear points (9 627 attempts, 8.8 M draws there) cannot hold
//               the GPU for tens of milliseconds.  A budget only counts where the serial loop would get to: the result does not depend on R.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ inline
#else
#define RS_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define RS_UNROLL _Pragma("unroll")
#else
#define RS_UNROLL
#endif

namespace omni {
namespace rs {

constexpr int kMaxIters = 2000;                 // findHomography's maxIters
constexpr int kAttemptBudget = 256;             // attempts of one iteration before the device gives up (the host's own limit: 10 000)
constexpr int kDrawBudget = 262144;             // numbers drawn for one pair before the device gives up
constexpr int kEnumMax = 6;                     // up to this count all count! / (count - 4)! ordered subsets are looked at first
constexpr int kMaxN = 1024;                     // matches per pair (the matcher's limit)
constexpr int kRawChunk = 256;                  // numbers drawn per generation step
constexpr int kAttChunk = kRawChunk / 4;        // ... hold at most this many attempts
constexpr int kRoundFirst = 64, kRound = 256;   // the kernel's round sizes: a true loop ends inside the first
constexpr double kFltEpsilon = 1.1920928955078125e-07, kDblEpsilon = 2.220446049250313e-16;

// ---- RANSACUpdateNumIters and the table the scan reads: HOST ONLY (pow / log) --------------------------------------------------------------------
inline int update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = p < 0. ? 0. : (p > 1. ? 1. : p); ep = ep < 0. ? 0. : (ep > 1. ? 1. : ep);
    double num = 1. - p > 2.2250738585072014e-308 ? 1. - p : 2.2250738585072014e-308, denom = 1. - pow(1. - ep, model_points);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num); denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)lrint(num / denom);
}
// T[g], g = 0 .. count: what `niters` becomes at most once a model with g inliers of count is the best
inline void fill_T(int count, int* T) { for (int g = 0; g <= count; ++g) T[g] = update_num_iters(0.995, (double)(count - g) / count, 4, kMaxIters); }

// ---- the flag filter (:574): match i of the list is kept when its query key point has a 3-D landmark ---------------------------------------------
RS_HD bool flag_keep(int query_idx, const uint8_t* flags, int n_flags) { return query_idx >= 0 && query_idx < n_flags && flags[query_idx] != 0; }

// ---- cv::RNG and getSubset ------------------------------------------------------------------------------------------------------------------------
RS_HD unsigned rng_next(uint64_t& s) { s = (uint64_t)(unsigned)s * 4164903690u + (unsigned)(s >> 32); return (unsigned)s; }
RS_HD unsigned rng_residue(unsigned raw, int count) { return raw % (unsigned)count; }      // uniform(0, count): exact integer remainder

struct Gen {
    uint64_t state;        // CvRng
    int idx[4], i;         // the attempt being drawn
    int draws;             // numbers consumed so far
    int attempts;          // failed attempts of the iteration being served
    int over;              // a budget was passed: no further subsets
};
RS_HD void gen_init(Gen& g) { g.state = 0xffffffffffffffffull; g.i = 0; g.draws = 0; g.attempts = 0; g.over = 0; g.idx[0] = g.idx[1] = g.idx[2] = g.idx[3] = 0; }
// one number of the stream, already reduced: 1 when it completes an attempt (g.idx = four distinct indices)
RS_HD int gen_feed(Gen& g, int v) {                        // (no indexed access: the attempt stays in registers)
    ++g.draws;
    if ((g.i > 0 && v == g.idx[0]) || (g.i > 1 && v == g.idx[1]) || (g.i > 2 && v == g.idx[2])) return 0;
    if (g.i == 0) g.idx[0] = v; else if (g.i == 1) g.idx[1] = v; else if (g.i == 2) g.idx[2] = v; else g.idx[3] = v;
    if (++g.i < 4) return 0;
    g.i = 0;
    return 1;
}
// the attempt that STARTS at number `pos` of a chunk of n reduced numbers: the position behind its last number (idx = its four indices), 0 when the chunk
// ends first.  Which positions do start an attempt is only known serially; every position can be tried at once.
RS_HD int gen_attempt_at(const unsigned* reduced, int pos, int n, int* idx) {
    Gen g;
    gen_init(g);
    for (int e = pos; e < n; ++e)
        if (gen_feed(g, (int)reduced[e])) { idx[0] = g.idx[0]; idx[1] = g.idx[1]; idx[2] = g.idx[2]; idx[3] = g.idx[3]; return e + 1; }
    return 0;
}
// a completed attempt, in stream order, with its check_subset verdict and the stream position behind it: 1 = the next iteration's subset, 0 = rejected,
// -1 = a budget was passed (this and every later iteration has no subset)
RS_HD int gen_attempt(Gen& g, bool pass, int draws_end) {
    if (g.over) return -1;
    if (draws_end > kDrawBudget) { g.over = 1; return -1; }
    if (pass) { g.attempts = 0; return 1; }
    if (++g.attempts >= kAttemptBudget) { g.over = 1; return -1; }
    return 0;
}

// ---- HomographyModel: points are [n][2] floats (OpenCV's Point2f), src = the OLD image's, dst = the NEW image's ----------------------------------
RS_HD bool collinear(const float* m, const int* idx) {           // haveCollinearPoints, count = 4: triples with the LAST point only
    const int i = 3;
    bool hit = false;                                            // (the host returns at the first hit: the same verdict)
    RS_UNROLL for (int j = 0; j < i; ++j) {
        const double dx1 = (double)m[2 * idx[j]] - (double)m[2 * idx[i]], dy1 = (double)m[2 * idx[j] + 1] - (double)m[2 * idx[i] + 1];
        RS_UNROLL for (int k = 0; k < j; ++k) {
            const double dx2 = (double)m[2 * idx[k]] - (double)m[2 * idx[i]], dy2 = (double)m[2 * idx[k] + 1] - (double)m[2 * idx[i] + 1];
            if (fabs(dx2 * dy1 - dy2 * dx1) <= kFltEpsilon * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) hit = true;
        }
    }
    return hit;
}
RS_HD double det_rows(const float* m, int a, int b, int c) {     // geom::det of the rows (x, y, 1)
    const double a00 = m[2 * a], a01 = m[2 * a + 1], a02 = 1, a10 = m[2 * b], a11 = m[2 * b + 1], a12 = 1, a20 = m[2 * c], a21 = m[2 * c + 1], a22 = 1;
    return a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
}
RS_HD bool check_subset(const float* src, const float* dst, const int* idx) {
    if (collinear(src, idx) || collinear(dst, idx)) return false;
    int negative = 0;                                            // the triangles {0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}
    negative += det_rows(src, idx[0], idx[1], idx[2]) * det_rows(dst, idx[0], idx[1], idx[2]) < 0;
    negative += det_rows(src, idx[1], idx[2], idx[3]) * det_rows(dst, idx[1], idx[2], idx[3]) < 0;
    negative += det_rows(src, idx[0], idx[2], idx[3]) * det_rows(dst, idx[0], idx[2], idx[3]) < 0;
    negative += det_rows(src, idx[0], idx[1], idx[3]) * det_rows(dst, idx[0], idx[1], idx[3]) < 0;
    return negative == 0 || negative == 4;
}
// true when some ORDERED 4-subset of the count points passes check_subset; lanes split the first index
RS_HD bool any_valid_subset(const float* src, const float* dst, int count, int lane, int n_lanes) {
    int idx[4];
    for (int a = lane; a < count; a += n_lanes)
        for (int b = 0; b < count; ++b) { if (b == a) continue;
            for (int c = 0; c < count; ++c) { if (c == a || c == b) continue;
                for (int d = 0; d < count; ++d) { if (d == a || d == b || d == c) continue;
                    idx[0] = a; idx[1] = b; idx[2] = c; idx[3] = d;
                    if (check_subset(src, dst, idx)) return true;
                } } }
    return false;
}

// jacobi_eigen<9> up to the sort: A is destroyed, its diagonal holds the eigenvalues, V's ROWS the eigenvectors
RS_HD void jacobi9(double A[9][9], double V[9][9]) {
    RS_UNROLL for (int i = 0; i < 9; ++i) { RS_UNROLL for (int j = 0; j < 9; ++j) V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
        RS_UNROLL for (int i = 0; i < 9; ++i) { diag += A[i][i] * A[i][i]; RS_UNROLL for (int j = i + 1; j < 9; ++j) off += A[i][j] * A[i][j]; }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        RS_UNROLL for (int p = 0; p < 8; ++p) {
            RS_UNROLL for (int q = p + 1; q < 9; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), s = t * c;
                RS_UNROLL for (int k = 0; k < 9; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                RS_UNROLL for (int k = 0; k < 9; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                RS_UNROLL for (int k = 0; k < 9; ++k) { const double vpk = V[p][k], vqk = V[q][k]; V[p][k] = c * vpk - s * vqk; V[q][k] = s * vpk + c * vqk; }
            }
        }
    }
}
// HomographyEstimatorCallback::runKernel on four points (M = src, m = dst): H[9] with H[8] = 1.  *tie = 1 when the smallest eigenvalue is not unique.
RS_HD bool run_kernel(const float* src, const float* dst, const int* idx, double* H, int* tie) {
    const int count = 4;
    *tie = 0;
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    RS_UNROLL for (int i = 0; i < count; ++i) { cmx += (double)dst[2 * idx[i]]; cmy += (double)dst[2 * idx[i] + 1]; cMx += (double)src[2 * idx[i]]; cMy += (double)src[2 * idx[i] + 1]; }
    cmx /= count; cmy /= count; cMx /= count; cMy /= count;
    RS_UNROLL for (int i = 0; i < count; ++i) {
        smx += fabs((double)dst[2 * idx[i]] - cmx); smy += fabs((double)dst[2 * idx[i] + 1] - cmy);
        sMx += fabs((double)src[2 * idx[i]] - cMx); sMy += fabs((double)src[2 * idx[i] + 1] - cMy);
    }
    if (fabs(smx) < kDblEpsilon || fabs(smy) < kDblEpsilon || fabs(sMx) < kDblEpsilon || fabs(sMy) < kDblEpsilon) return false;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
    const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    double LtL[9][9], V[9][9];
    RS_UNROLL for (int j = 0; j < 9; ++j) { RS_UNROLL for (int k = 0; k < 9; ++k) LtL[j][k] = 0; }
    RS_UNROLL for (int i = 0; i < count; ++i) {
        const double x = ((double)dst[2 * idx[i]] - cmx) * smx, y = ((double)dst[2 * idx[i] + 1] - cmy) * smy;
        const double X = ((double)src[2 * idx[i]] - cMx) * sMx, Y = ((double)src[2 * idx[i] + 1] - cMy) * sMy;
        const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x}, Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
        RS_UNROLL for (int j = 0; j < 9; ++j) { RS_UNROLL for (int k = j; k < 9; ++k) LtL[j][k] += Lx[j] * Lx[k] + Ly[j] * Ly[k]; }
    }
    RS_UNROLL for (int j = 0; j < 9; ++j) { RS_UNROLL for (int k = 0; k < j; ++k) LtL[j][k] = LtL[k][j]; }
    jacobi9(LtL, V);
    // the row of the smallest eigenvalue (selects, not an indexed read: the rows stay in registers)
    double wmin = LtL[0][0], h0[9];
    int n_min = 1;
    RS_UNROLL for (int k = 0; k < 9; ++k) h0[k] = V[0][k];
    RS_UNROLL for (int i = 1; i < 9; ++i) {
        const double w = LtL[i][i];
        if (w < wmin) { wmin = w; n_min = 1; RS_UNROLL for (int k = 0; k < 9; ++k) h0[k] = V[i][k]; }
        else if (w == wmin) ++n_min;
    }
    *tie = n_min > 1;
    double tmp[9], out[9];
    RS_UNROLL for (int r = 0; r < 3; ++r) { RS_UNROLL for (int c = 0; c < 3; ++c) { tmp[r * 3 + c] = 0; RS_UNROLL for (int k = 0; k < 3; ++k) tmp[r * 3 + c] += invHnorm[r * 3 + k] * h0[k * 3 + c]; } }
    RS_UNROLL for (int r = 0; r < 3; ++r) { RS_UNROLL for (int c = 0; c < 3; ++c) { out[r * 3 + c] = 0; RS_UNROLL for (int k = 0; k < 3; ++k) out[r * 3 + c] += tmp[r * 3 + k] * Hnorm2[k * 3 + c]; } }
    if (fabs(out[8]) < 1e-300) return false;
    RS_UNROLL for (int k = 0; k < 9; ++k) H[k] = out[k] / out[8];
    return true;
}
// HomographyModel::error(i) <= (float)(3 * 3)
RS_HD bool inlier(const double* H, const float* src, const float* dst, int i) {
    const double sx = src[2 * i], sy = src[2 * i + 1], tx = dst[2 * i], ty = dst[2 * i + 1];
    const double ww = 1. / (H[6] * sx + H[7] * sy + 1.);
    const double dx = (H[0] * sx + H[1] * sy + H[2]) * ww - tx, dy = (H[3] * sx + H[4] * sy + H[5]) * ww - ty;
    return (float)(dx * dx + dy * dy) <= 9.0f;
}
// one hypothesis: its model and inlier count, -1 when run_kernel fails
RS_HD int hypothesis(const float* src, const float* dst, int count, const int* idx, double* H, int* tie) {
    if (!run_kernel(src, dst, idx, H, tie)) return -1;
    int good = 0;
    for (int k = 0; k < count; ++k) good += inlier(H, src, dst, k) ? 1 : 0;
    return good;
}

// ---- the stopping rule as a scan over the iterations in order -------------------------------------------------------------------------------------
struct Scan { int niters, max_good, best_iter, iters_run; };
RS_HD void scan_init(Scan& s) { s.niters = kMaxIters; s.max_good = 0; s.best_iter = -1; s.iters_run = 0; }
// iteration `iter` (< s.niters) had `good` inliers: true when it is the new best model
RS_HD bool scan_step(Scan& s, int iter, int good, const int* T) {
    s.iters_run = iter + 1;
    if (good <= (s.max_good > 3 ? s.max_good : 3)) return false;
    s.max_good = good; s.best_iter = iter;
    if (T[good] < s.niters) s.niters = T[good];
    return true;
}
RS_HD void put_info(int* info, int count, const Scan& s) { info[0] = count; info[1] = s.iters_run; info[2] = s.best_iter; info[3] = s.max_good; }

// the cases that need no stream: count < 4, count == 4, a small count with no valid subset.  Returns the status, or -1 when RANSAC has to run.  `any_valid`:
// any_valid_subset() of the pair (only read when 4 < count <= kEnumMax).  mask [count], H [9], info [4] are written for every status returned.
RS_HD int special_cases(const float* src, const float* dst, int count, bool any_valid, uint8_t* mask, double* H, int* info, int* tie) {
    Scan s;
    scan_init(s);
    *tie = 0;
    for (int k = 0; k < 9; ++k) H[k] = 0;
    if (count < 4) { put_info(info, count, s); return OMNI_HG_UNFILTERED; }
    if (count == 4) {
        const int idx[4] = {0, 1, 2, 3};
        double h[9];
        const bool ok = run_kernel(src, dst, idx, h, tie);
        s.iters_run = 1;
        if (ok) { s.best_iter = 0; s.max_good = 4; for (int k = 0; k < 9; ++k) H[k] = h[k]; }
        for (int i = 0; i < 4; ++i) mask[i] = ok ? 1 : 0;
        put_info(info, count, s);
        return ok ? OMNI_HG_OK : OMNI_HG_NO_MODEL;
    }
    if (count <= kEnumMax && !any_valid) {
        for (int i = 0; i < count; ++i) mask[i] = 0;
        put_info(info, count, s);
        return OMNI_HG_NO_MODEL;
    }
    return -1;
}

// ---- the whole pair on the host, in rounds of R iterations (1 <= R <= kMaxIters): what the kernel computes --------------------------------------------
// src / dst [count][2]; T [count + 1] (fill_T); mask [count]; H [9]; info = {count, iterations run, best iteration, max_good}.  Returns the status;
// *ties = hypotheses with a tied smallest eigenvalue among those evaluated.
inline int ransac_host(const float* src, const float* dst, int count, const int* T, int R, uint8_t* mask, double* H, int* info, int* ties) {
    int tie = 0;
    *ties = 0;
    const int st = special_cases(src, dst, count, count > 4 && count <= kEnumMax ? any_valid_subset(src, dst, count, 0, 1) : true, mask, H, info, &tie);
    if (st >= 0) { *ties = tie; return st; }
    static thread_local unsigned short queue[kMaxIters + kAttChunk][4];
    static thread_local int good[kMaxIters];
    static thread_local double Hs[kMaxIters][9];
    Gen g;
    gen_init(g);
    Scan s;
    scan_init(s);
    int nq = 0, base = 0, status = -1;
    double best[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    while (status < 0) {
        while (nq < R && !g.over) {                                 // the next attempts of the stream, kRawChunk numbers at a time
            for (int d = 0; d < kRawChunk && !g.over; ++d) {
                const int v = (int)rng_residue(rng_next(g.state), count);
                if (!gen_feed(g, v)) continue;
                const int r = gen_attempt(g, check_subset(src, dst, g.idx), g.draws);
                if (r == 1) { for (int k = 0; k < 4; ++k) queue[nq][k] = (unsigned short)g.idx[k]; ++nq; }
            }
        }
        const int avail = nq < R ? nq : R;
        for (int j = 0; j < avail; ++j) {
            const int idx[4] = {queue[j][0], queue[j][1], queue[j][2], queue[j][3]};
            good[j] = hypothesis(src, dst, count, idx, Hs[j], &tie);
            *ties += tie;
        }
        for (int j = 0; j < R; ++j) {
            if (base + j >= s.niters) { status = s.max_good > 0 ? OMNI_HG_OK : OMNI_HG_NO_MODEL; break; }
            if (j >= avail) { status = OMNI_HG_HOST; break; }
            if (scan_step(s, base + j, good[j], T)) for (int k = 0; k < 9; ++k) best[k] = Hs[j][k];
        }
        base += R;
        for (int j = R; j < nq; ++j) for (int k = 0; k < 4; ++k) queue[j - R][k] = queue[j][k];
        nq = nq > R ? nq - R : 0;
    }
    put_info(info, count, s);
    for (int k = 0; k < 9; ++k) H[k] = status == OMNI_HG_OK ? best[k] : 0.0;
    for (int i = 0; i < count; ++i) mask[i] = status == OMNI_HG_OK && inlier(best, src, dst, i) ? 1 : 0;
    return status;
}

}  // namespace rs
}  // namespace omni
