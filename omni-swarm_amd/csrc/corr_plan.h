// The correspondences of a loop candidate, stated ONCE: what the two compute_correspond_features of host/loop_geometry.hpp (swarm_loop/src/loop_detector.cpp:431-624)
// make of the matcher's lists and the homography masks, up to the input of compute_relative_pose, with the same operations in the same order:
//   direction pairing   pair_dirs: step s of candidate (main_dir_new, main_dir_old) pairs direction (main_dir_new + s) % MAX_DIRS of the new frame with direction
//                       ((main_dir_old - main_dir_new + MAX_DIRS) % MAX_DIRS + main_dir_new + s) % MAX_DIRS of the old one (:211-216);
//   per pair            the flag filter on the matches (keep: the rule of the homography stage's filter, ransac_plan.h flag_keep, so that the mask's positions are
//                       the kept list's), then the compaction by the homography mask -- and the quirk of :200: a pair with fewer than 4 flagged matches asks for no
//                       homography and contributes its flagged matches unfiltered;
//   gathers             X = the new image's landmarks_3d at the match's query index, u = the old image's landmarks_2d_norm at its train index rotated onto the old
//                       main camera by dq_old (geom::rotate_pt_norm2d: Eigen's toRotationMatrix, the product, the clamp of z, the division, the cast to float);
//                       the quaternion algebra that makes dq_old stays with the caller;
//   per candidate       the concatenation over its pairs in pairing order, matched_dir_count (pairs with at least MIN_MATCH_PRE_DIR correspondences) against
//                       MIN_DIRECTION_LOOP, and the size gate of compute_loop_core (:291).
// new_norm_2d and old_3d, which nothing behind that gate reads, are not assembled: n_corr is the size they would have.  corr_assemble.hip only spreads this over
// lanes; corr_assemble_host.cpp is this header under g++ (omni_corr_assemble_host: the kernel's stand-in).  Contraction off on both sides: products and sums round
// one by one.  Plain C++, no HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/omni_hip.h"
#include "ransac_plan.h"

#if defined(__HIPCC__)
#define CORR_HD __host__ __device__ inline
#else
#define CORR_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace omni {
namespace corr {

constexpr int THREADS = 256;                         // corr_assemble_kernel: one workgroup per candidate, one wave per pair in the compaction
constexpr int kMaxPairs = 4;                         // pairs per candidate: MAX_DIRS at most (= THREADS / 64)
constexpr int kMaxCall = 64;                         // candidates and pairs per call (the matcher's limit)

CORR_HD void pair_dirs(int main_dir_new, int main_dir_old, int max_dirs, int step, int* dir_new, int* dir_old) {
    const int d = main_dir_new + step;
    *dir_new = d % max_dirs;
    *dir_old = ((main_dir_old - main_dir_new + max_dirs) % max_dirs + d) % max_dirs;
}

// matches of pair p as the stage reads them: none for an empty image (BFMatcher on an empty set), never more than max_n
CORR_HD int n_matches(const omni_corr_io& io, int p) {
    if (io.nq[p] <= 0 || io.nt[p] <= 0) return 0;
    const int n = io.n_matches[p];
    return n < 0 ? 0 : (n > io.max_n ? io.max_n : n);
}
// the flag filter on match i of pair p (:574); the indices it would gather with come back
CORR_HD bool keep(const omni_corr_io& io, int p, int i, int* qi, int* ti) {
    const size_t at = (size_t)p * io.max_n;
    int nf = io.n_flags[p];
    nf = nf < 0 ? 0 : (nf > io.max_n ? io.max_n : nf);
    *qi = io.q_idx[at + i]; *ti = io.t_idx[at + i];
    return rs::flag_keep(*qi, io.q_flags + at, nf) && *qi < io.nq[p] && *qi < io.max_n && *ti >= 0 && *ti < io.nt[p] && *ti < io.max_n;
}
// whether the flagged match of rank `rank` in a pair with n_kept flagged matches stays (:200-205)
CORR_HD bool survives(const omni_corr_io& io, int p, int n_kept, int rank) { return n_kept < 4 || io.mask[(size_t)p * io.max_n + rank] != 0; }

// geom::rotate_pt_norm2d(pt, q) with q = (w, x, y, z), cast to float
CORR_HD void rotate_norm(double px, double py, const double* q, float* out) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double m00 = 1 - (tyy + tzz), m01 = txy - twz, m02 = txz + twy;
    const double m10 = txy + twz, m11 = 1 - (txx + tzz), m12 = tyz - twx;
    const double m20 = txz - twy, m21 = tyz + twx, m22 = 1 - (txx + tyy);
    const double vz = 1;
    const double rx = m00 * px + m01 * py + m02 * vz, ry = m10 * px + m11 * py + m12 * vz;
    double rz = m20 * px + m21 * py + m22 * vz;
    if (rz < 1e-3 && rz > 0) rz = 1e-3;
    if (rz > -1e-3 && rz < 0) rz = -1e-3;
    out[0] = (float)(rx / rz); out[1] = (float)(ry / rz);
}
// the two gathers of the match (qi, ti) of pair p
CORR_HD void gather(const omni_corr_io& io, int p, int qi, int ti, float* X3, float* u2) {
    const size_t at = (size_t)p * io.max_n;
    const float* s = io.q_3d + 3 * (at + qi);
    X3[0] = s[0]; X3[1] = s[1]; X3[2] = s[2];
    const float* n = io.t_norm + 2 * (at + ti);
    rotate_norm((double)n[0], (double)n[1], io.dq_old + 4 * p, u2);
}
// compute_correspond_features' verdict (:235) and compute_loop_core's size gate (:291); a pair the homography stage handed back hands the candidate back
CORR_HD int gate(const omni_corr_cand& c, int n_corr, int matched_dir_count, bool any_host) {
    if (any_host) return OMNI_CORR_HOST;
    if (n_corr == 0 || matched_dir_count < c.min_direction_loop) return OMNI_CORR_REJECT;
    return (n_corr > c.min_loop_num || (c.init_mode != 0 && n_corr > c.init_mode_min_loop_num)) ? OMNI_CORR_OK : OMNI_CORR_REJECT;
}

// What both entries refuse before they touch anything; NULL when the call may go ahead.  cands == nullptr: the table lives in device memory, its maker has checked
// it with this function before the upload (the kernel clamps every count and index it reads and never writes outside a candidate's cap slots)
inline const char* refusal(int n_cands, int n_pairs, int max_n, int cap, const omni_corr_cand* cands) {
    if (n_cands < 1 || n_cands > kMaxCall) return "n_cands outside [1, 64]";
    if (n_pairs < 0 || n_pairs > kMaxCall) return "n_pairs outside [0, 64]";
    if (max_n < 1 || max_n > rs::kMaxN) return "max_n outside [1, 1024]";
    if (cap < 1 || cap > kMaxPairs * rs::kMaxN) return "cap outside [1, 4096]";
    if (!cands) return nullptr;
    for (int c = 0; c < n_cands; ++c) {
        if (cands[c].pair_count < 0 || cands[c].pair_count > kMaxPairs) return "a candidate with more than 4 pairs";
        if (cands[c].pair_first < 0 || cands[c].pair_first + cands[c].pair_count > n_pairs) return "a candidate's pairs lie outside the call's";
        if ((int64_t)cands[c].pair_count * max_n > cap) return "cap below pair_count * max_n";
    }
    return nullptr;
}

// the whole stage on the host, bit for bit
inline void assemble_host(const omni_corr_io& io) {
    for (int c = 0; c < io.n_cands; ++c) {
        const omni_corr_cand& cd = io.cands[c];
        int n_corr = 0, matched = 0;
        bool any_host = false;
        for (int j = 0; j < cd.pair_count; ++j) {
            const int p = cd.pair_first + j, n = n_matches(io, p);
            const size_t at = (size_t)p * io.max_n;
            if (io.hg_status[p] == OMNI_HG_HOST) any_host = true;
            int n_kept = 0, qi, ti;
            for (int i = 0; i < n; ++i) if (keep(io, p, i, &qi, &ti)) ++n_kept;
            int rank = 0, k = 0;
            for (int i = 0; i < n; ++i) {
                if (!keep(io, p, i, &qi, &ti)) continue;
                if (survives(io, p, n_kept, rank++)) {
                    io.new_idx[at + k] = qi; io.old_idx[at + k] = ti;
                    gather(io, p, qi, ti, io.X + 3 * ((size_t)c * io.cap + n_corr + k), io.u + 2 * ((size_t)c * io.cap + n_corr + k));
                    ++k;
                }
            }
            io.n_pair_corr[p] = k;
            if (k >= cd.min_match_pre_dir) ++matched;
            n_corr += k;
        }
        io.n_corr[c] = n_corr; io.matched_dir_count[c] = matched; io.gate[c] = gate(cd, n_corr, matched, any_host);
    }
}

}  // namespace corr
}  // namespace omni
