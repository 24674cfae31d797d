// Pins omni-swarm_amd/csrc/ransac_plan.h (the arithmetic of the GPU homography RANSAC, csrc/homography.hip) to the host functions it restates:
// geom::find_homography_ransac / ransac_run / HomographyModel / jacobi_eigen<9> (host/geometry.hpp) and the image-pair
// LoopGeometry::compute_correspond_features (host/loop_geometry.hpp).  Built with plain g++ (tests/homography_cases.py); the GPU tests use the `plan` mode as
// the reference the kernels must equal bit for bit.
//
//   ransac_plan_pin plan R   the header: flag filter, fill_T, rs::ransac_host in rounds of R iterations
//   ransac_plan_pin host     the host functions on the same input: compute_correspond_features with the case's match list behind its matcher callback (the
//                            reduced index lists, its return value), find_homography_ransac (ok, mask, H), and ransac_run once more around a model that
//                            counts (iterations run, best iteration, tied smallest eigenvalues by jacobi_eigen<9> itself)
//   ransac_plan_pin time     the host's cost: per case one text line "n_kept milliseconds" of geom::find_homography_ransac alone on the flagged matches, one thread
//                            (tools/homography_timing.py sets it beside the device time)
//   ransac_plan_pin scan     no input: RANSACUpdateNumIters(0.995, (count - good) / count, 4, niters) against min(T[good], niters) for every count 5..200,
//                            good 4..count, niters 0..2000; prints "combinations mismatches"
//
// stdin, repeated until EOF (binary, native endianness): int32 n_matches, nq, nt, n_flags; q_idx, t_idx [n_matches] i32; q_xy [nq][2] f32; t_xy [nt][2] f32;
//   flags [n_flags] u8
// stdout per case: int32 status, n_kept, info[4], ties, ret, n_reduced; H [9] f64; kept [n_matches] i32, new_idx, old_idx [n_matches] i32 (-1 behind the end);
//   mask [n_matches] u8 (over the kept list, 0 behind its end).  A pair the header hands back (OMNI_HG_HOST) has ret = n_reduced = -1.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/ransac_plan.h"
#include "../../omni-swarm_amd/host/loop_geometry.hpp"

using namespace omni;

struct Case {
    int n = 0, nq = 0, nt = 0, nf = 0;
    std::vector<int> qi, ti;
    std::vector<float> qxy, txy;
    std::vector<uint8_t> flags;
};
template <typename T> static bool get(std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, stdin) == n; }
template <typename T> static void put(const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), stdout); }

static int read_case(Case& c) {                  // 1: a case, 0: clean end of input, -1: truncated
    int hdr[4];
    const size_t got = fread(hdr, sizeof(int), 4, stdin);
    if (got == 0) return 0;
    if (got != 4) return -1;
    c.n = hdr[0]; c.nq = hdr[1]; c.nt = hdr[2]; c.nf = hdr[3];
    if (c.n < 0 || c.nq < 0 || c.nt < 0 || c.nf < 0 || c.n > rs::kMaxN) return -1;
    return get(c.qi, (size_t)c.n) && get(c.ti, (size_t)c.n) && get(c.qxy, (size_t)c.nq * 2) && get(c.txy, (size_t)c.nt * 2) && get(c.flags, (size_t)c.nf) ? 1 : -1;
}

struct Out {
    int status = 0, n_kept = 0, info[4] = {0, 0, -1, 0}, ties = 0, ret = 0, n_reduced = 0;
    std::vector<double> H = std::vector<double>(9, 0.0);
    std::vector<int> kept, new_idx, old_idx;
    std::vector<uint8_t> mask;
};

// a HomographyModel that counts what ransac_run does with it
struct Counting {
    geom::HomographyModel m;
    int passes = 0, best_iter = -1, ties = 0;
    bool check_subset(const int* idx, int n) { const bool ok = m.check_subset(idx, n); passes += ok; return ok; }
    bool run_kernel(const int* idx, int count) {
        // the two smallest eigenvalues of this subset's LtL by the host's own jacobi_eigen<9>
        const std::vector<geom::Vec2>&src = m.src, &dst = m.dst;
        geom::Vec2 cM, cm, sM, sm;
        for (int i = 0; i < count; ++i) { cm.x += dst[idx[i]].x; cm.y += dst[idx[i]].y; cM.x += src[idx[i]].x; cM.y += src[idx[i]].y; }
        cm.x /= count; cm.y /= count; cM.x /= count; cM.y /= count;
        for (int i = 0; i < count; ++i) { sm.x += std::fabs(dst[idx[i]].x - cm.x); sm.y += std::fabs(dst[idx[i]].y - cm.y); sM.x += std::fabs(src[idx[i]].x - cM.x); sM.y += std::fabs(src[idx[i]].y - cM.y); }
        if (!(std::fabs(sm.x) < DBL_EPSILON || std::fabs(sm.y) < DBL_EPSILON || std::fabs(sM.x) < DBL_EPSILON || std::fabs(sM.y) < DBL_EPSILON)) {
            sm.x = count / sm.x; sm.y = count / sm.y; sM.x = count / sM.x; sM.y = count / sM.y;
            double LtL[9][9] = {}, W[9], V[9][9];
            for (int i = 0; i < count; ++i) {
                const double x = (dst[idx[i]].x - cm.x) * sm.x, y = (dst[idx[i]].y - cm.y) * sm.y, X = (src[idx[i]].x - cM.x) * sM.x, Y = (src[idx[i]].y - cM.y) * sM.y;
                const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x}, Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
                for (int j = 0; j < 9; ++j) for (int k = j; k < 9; ++k) LtL[j][k] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
            }
            for (int j = 0; j < 9; ++j) for (int k = 0; k < j; ++k) LtL[j][k] = LtL[k][j];
            geom::jacobi_eigen<9>(LtL, W, V);
            ties += W[8] == W[7];
        }
        return m.run_kernel(idx, count);
    }
    float error(int i) const { return m.error(i); }
    void keep_best() { m.keep_best(); best_iter = passes - 1; }
};

static void run_plan(const Case& c, int R, Out& o) {
    std::vector<float> src, dst;
    for (int i = 0; i < c.n; ++i) {
        if (!rs::flag_keep(c.qi[i], c.flags.data(), c.nf)) continue;
        o.kept[o.n_kept++] = i;
        src.push_back(c.txy[2 * c.ti[i]]); src.push_back(c.txy[2 * c.ti[i] + 1]);
        dst.push_back(c.qxy[2 * c.qi[i]]); dst.push_back(c.qxy[2 * c.qi[i] + 1]);
    }
    std::vector<int> T((size_t)o.n_kept + 1, 0);
    if (o.n_kept > 0) rs::fill_T(o.n_kept, T.data());
    o.status = rs::ransac_host(src.data(), dst.data(), o.n_kept, T.data(), R, o.mask.data(), o.H.data(), o.info, &o.ties);
    if (o.status == OMNI_HG_HOST) { o.ret = o.n_reduced = -1; return; }
    o.ret = o.status != OMNI_HG_UNFILTERED;
    for (int j = 0; j < o.n_kept; ++j)
        if (o.status == OMNI_HG_UNFILTERED || o.mask[j]) { o.new_idx[o.n_reduced] = c.qi[o.kept[j]]; o.old_idx[o.n_reduced] = c.ti[o.kept[j]]; ++o.n_reduced; }
}

static void run_host(const Case& c, Out& o) {
    ImageDescriptor nw, old;
    auto fill = [](ImageDescriptor& im, const std::vector<float>& xy, int n) {
        im.landmark_num = n;
        im.landmarks_2d.resize((size_t)n);
        for (int k = 0; k < n; ++k) im.landmarks_2d[(size_t)k] = {xy[2 * k], xy[2 * k + 1]};
        im.landmarks_2d_norm.assign((size_t)n, Point2f{});
        im.landmarks_3d.assign((size_t)n, Point3f{});
        im.feature_descriptor.assign((size_t)n * 4, 0.f);
    };
    fill(nw, c.qxy, c.nq); fill(old, c.txy, c.nt);
    nw.landmarks_flag.assign(c.flags.begin(), c.flags.end());
    LoopGeometry g;
    g.match = [&c](const float*, int, const float*, int, int, std::vector<DMatch>& out) { out.clear(); for (int i = 0; i < c.n; ++i) out.push_back({c.qi[i], c.ti[i], 0.f}); };
    std::vector<geom::Vec2> n2, o2;
    std::vector<geom::Vec3> n3, o3;
    std::vector<int> ni, oi;
    o.ret = g.compute_correspond_features(nw, old, n2, n3, ni, o2, o3, oi) ? 1 : 0;
    o.n_reduced = (int)ni.size();
    std::copy(ni.begin(), ni.end(), o.new_idx.begin()); std::copy(oi.begin(), oi.end(), o.old_idx.begin());
    // the filter of :574 once more, for the kept list and the point lists find_homography_ransac is given
    std::vector<geom::Vec2> old_2d, new_2d;
    for (int i = 0; i < c.n; ++i) {
        if (c.qi[i] >= (int)nw.landmarks_flag.size() || !nw.landmarks_flag[c.qi[i]]) continue;
        o.kept[o.n_kept++] = i;
        new_2d.push_back({nw.landmarks_2d[c.qi[i]].x, nw.landmarks_2d[c.qi[i]].y}); old_2d.push_back({old.landmarks_2d[c.ti[i]].x, old.landmarks_2d[c.ti[i]].y});
    }
    const int n = o.n_kept;
    o.info[0] = n;
    if (n < 4) { o.status = OMNI_HG_UNFILTERED; return; }
    std::vector<uint8_t> mask;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool ok = geom::find_homography_ransac(old_2d, new_2d, 3.0, mask, H);
    o.status = ok ? OMNI_HG_OK : OMNI_HG_NO_MODEL;
    for (int k = 0; k < 9; ++k) o.H[k] = ok ? H[k] : 0.0;
    int good = 0;
    for (int i = 0; i < n; ++i) { o.mask[i] = mask[i]; good += mask[i]; }
    o.info[3] = ok ? good : 0;
    if (n == 4) { o.info[1] = 1; o.info[2] = ok ? 0 : -1; return; }
    Counting cm{geom::HomographyModel{old_2d, new_2d, {}, {}}};
    std::vector<uint8_t> mask2;
    const bool ok2 = geom::ransac_run(cm, n, 4, 3.0, 0.995, 2000, mask2);
    if (ok2 != ok || (ok && mask2 != mask)) { fprintf(stderr, "ransac_plan_pin: the counting model changed ransac_run's result\n"); exit(3); }
    o.info[1] = cm.passes; o.info[2] = cm.best_iter; o.ties = cm.ties;
}

static void run_time(const Case& c) {
    std::vector<geom::Vec2> old_2d, new_2d;
    for (int i = 0; i < c.n; ++i) {
        if (!rs::flag_keep(c.qi[i], c.flags.data(), c.nf)) continue;
        new_2d.push_back({c.qxy[2 * c.qi[i]], c.qxy[2 * c.qi[i] + 1]}); old_2d.push_back({c.txy[2 * c.ti[i]], c.txy[2 * c.ti[i] + 1]});
    }
    std::vector<uint8_t> mask;
    const auto t0 = std::chrono::steady_clock::now();
    if (old_2d.size() >= 4) geom::find_homography_ransac(old_2d, new_2d, 3.0, mask);
    printf("%zu %.4f\n", old_2d.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

static int run_scan() {
    long long combos = 0, bad = 0;
    std::vector<int> T(201);
    for (int count = 5; count <= 200; ++count) {
        rs::fill_T(count, T.data());
        for (int good = 4; good <= count; ++good)
            for (int niters = 0; niters <= 2000; ++niters) {
                const int ref = geom::ransac_update_num_iters(0.995, (double)(count - good) / count, 4, niters);
                ++combos;
                bad += ref != (T[good] < niters ? T[good] : niters);
            }
    }
    printf("%lld %lld\n", combos, bad);
    return 0;
}

int main(int argc, char** argv) {
    const bool plan = argc == 3 && !strcmp(argv[1], "plan"), host = argc == 2 && !strcmp(argv[1], "host"), timing = argc == 2 && !strcmp(argv[1], "time");
    if (argc == 2 && !strcmp(argv[1], "scan")) return run_scan();
    const int R = plan ? atoi(argv[2]) : 0;
    if ((!plan && !host && !timing) || (plan && (R < 1 || R > rs::kMaxIters))) { fprintf(stderr, "usage: ransac_plan_pin plan R | host | time < cases;  ransac_plan_pin scan\n"); return 2; }
    Case c;
    int rc;
    while ((rc = read_case(c)) == 1) {
        for (int i = 0; i < c.n; ++i)
            if (c.qi[i] < 0 || c.qi[i] >= c.nq || c.ti[i] < 0 || c.ti[i] >= c.nt) { fprintf(stderr, "ransac_plan_pin: a match outside its images\n"); return 1; }
        if (timing) { run_time(c); continue; }
        Out o;
        o.kept.assign((size_t)c.n, -1); o.new_idx.assign((size_t)c.n, -1); o.old_idx.assign((size_t)c.n, -1); o.mask.assign((size_t)c.n, 0);
        if (plan) run_plan(c, R, o); else run_host(c, o);
        const int head[9] = {o.status, o.n_kept, o.info[0], o.info[1], o.info[2], o.info[3], o.ties, o.ret, o.n_reduced};
        fwrite(head, sizeof(int), 9, stdout);
        put(o.H); put(o.kept); put(o.new_idx); put(o.old_idx); put(o.mask);
    }
    if (rc < 0) { fprintf(stderr, "ransac_plan_pin: truncated or inconsistent case\n"); return 1; }
    return 0;
}
