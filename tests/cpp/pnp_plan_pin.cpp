// Pins omni-swarm_amd/csrc/pnp_plan.h (the arithmetic of the GPU PnP RANSAC, csrc/pnp.hip) to the host functions it restates: geom::ransac_run<PnPModel>,
// geom::epnp, geom::pnp_error and geom::solve_pnp_ransac (host/geometry.hpp).  Built with plain g++ (tests/pnp_cases.py); the GPU tests use the `plan` mode as
// the reference the kernel must equal bit for bit.
//
//   pnp_plan_pin plan R   the header: fill_T, pnp::pnp_ransac_host in rounds of R iterations, then geom::pnp_refit on its mask and model
//   pnp_plan_pin host     the host functions on the same input: ransac_run around a PnPModel that counts (ok, mask, best model, iterations run, best
//                         iteration), then geom::solve_pnp_ransac (return value, pose, inlier list)
//   pnp_plan_pin time     the host's cost: per case one text line "count milliseconds" of geom::pnp_ransac alone, one thread (tools/pnp_timing.py)
//   pnp_plan_pin scan     no input: RANSACUpdateNumIters(0.99, (count - good) / count, 5, niters) against min(T[good], niters) for every count 6..300, then
//                         300..2048 in steps of 97, good 5..count, niters 1..1000; prints "combinations mismatches"
//
// stdin, repeated until EOF (binary, native endianness): int32 count, max_iters; X [count][3] f32; u [count][2] f32
// stdout per case: int32 status, info[4], ret, n_inliers; Rt [12] f64 (the best EPnP model, zeros unless OK); pose [12] f64 (the refit, zeros unless ret == 1);
//   mask [count] u8; inliers [count] i32 (-1 behind the end).  A candidate the header hands back (OMNI_PNP_HOST) has ret = -1.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/pnp_plan.h"
#include "../../omni-swarm_amd/host/geometry.hpp"

using namespace omni;

struct Case {
    int count = 0, max_iters = 0;
    std::vector<float> X, u;
};
static int read_case(Case& c) {                  // 1: a case, 0: clean end of input, -1: truncated
    int hdr[2];
    const size_t got = fread(hdr, sizeof(int), 2, stdin);
    if (got == 0) return 0;
    if (got != 2) return -1;
    c.count = hdr[0]; c.max_iters = hdr[1];
    if (c.count < 0 || c.count > pnp::kMaxN || c.max_iters < 1 || c.max_iters > pnp::kMaxIters) return -1;
    c.X.resize((size_t)c.count * 3); c.u.resize((size_t)c.count * 2);
    if (c.count && (fread(c.X.data(), 4, c.X.size(), stdin) != c.X.size() || fread(c.u.data(), 4, c.u.size(), stdin) != c.u.size())) return -1;
    return 1;
}
static void lists(const Case& c, std::vector<geom::Vec3>& X, std::vector<geom::Vec2>& u) {
    for (int i = 0; i < c.count; ++i) { X.push_back({c.X[3 * i], c.X[3 * i + 1], c.X[3 * i + 2]}); u.push_back({c.u[2 * i], c.u[2 * i + 1]}); }
}
static void rt12(const geom::Rt& p, double* o) { for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) o[3 * r + k] = p.R.m[r][k]; o[9] = p.t.x; o[10] = p.t.y; o[11] = p.t.z; }
static geom::Rt rt_of(const double* o) { geom::Rt p; for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) p.R.m[r][k] = o[3 * r + k]; p.t = {o[9], o[10], o[11]}; return p; }

struct Out {
    int status = 0, info[4] = {0, 0, -1, 0}, ret = 0, n_inliers = 0;
    double Rt[12] = {}, pose[12] = {};
    std::vector<uint8_t> mask;
    std::vector<int> inliers;
};

// a PnPModel that counts what ransac_run does with it (check_subset is always true: run_kernel is called once per iteration)
struct Counting {
    geom::PnPModel m;
    int iters = 0, best_iter = -1;
    bool check_subset(const int* idx, int n) const { return m.check_subset(idx, n); }
    bool run_kernel(const int* idx, int n) { ++iters; return m.run_kernel(idx, n); }
    float error(int i) const { return m.error(i); }
    void keep_best() { m.keep_best(); best_iter = iters - 1; }
};

static void run_plan(const Case& c, int R, Out& o) {
    std::vector<int> T((size_t)c.count + 1, 0);
    if (c.count > 0) pnp::fill_T(c.count, T.data());
    o.status = pnp::pnp_ransac_host(c.X.data(), c.u.data(), c.count, c.max_iters, T.data(), R, o.mask.data(), o.Rt, o.info);
    if (o.status == OMNI_PNP_HOST) { o.ret = -1; return; }
    if (o.status != OMNI_PNP_OK) return;
    std::vector<geom::Vec3> X;
    std::vector<geom::Vec2> u;
    lists(c, X, u);
    geom::Rt pose;
    std::vector<int> inl;
    o.ret = geom::pnp_refit(X, u, o.mask, rt_of(o.Rt), pose, inl) ? 1 : 0;
    if (o.ret) rt12(pose, o.pose);
    o.n_inliers = (int)inl.size();
    std::copy(inl.begin(), inl.end(), o.inliers.begin());
}

static void run_host(const Case& c, Out& o) {
    std::vector<geom::Vec3> X;
    std::vector<geom::Vec2> u;
    lists(c, X, u);
    o.info[0] = c.count;
    if (c.count < 6) o.status = OMNI_PNP_SKIPPED;
    else {
        Counting cm{geom::PnPModel{X, u, {}, {}}};
        std::vector<uint8_t> mask;
        const bool ok = geom::ransac_run(cm, c.count, 5, 3.0, 0.99, c.max_iters, mask);
        int good = 0;
        for (int i = 0; ok && i < c.count; ++i) good += mask[i];
        o.status = ok && good >= 6 ? OMNI_PNP_OK : OMNI_PNP_NO_MODEL;
        o.info[1] = cm.iters; o.info[2] = cm.best_iter; o.info[3] = good;
        if (o.status == OMNI_PNP_OK) { rt12(cm.m.best, o.Rt); o.mask = mask; }
    }
    geom::Rt pose;
    std::vector<int> inl;
    o.ret = geom::solve_pnp_ransac(X, u, c.max_iters, 3.0, 0.99, pose, inl) ? 1 : 0;
    if (o.ret) rt12(pose, o.pose); else inl.clear();      // (a `false` with five inliers leaves them in the list: no caller reads it then)
    o.n_inliers = (int)inl.size();
    std::copy(inl.begin(), inl.end(), o.inliers.begin());
}

static void run_time(const Case& c) {
    std::vector<geom::Vec3> X;
    std::vector<geom::Vec2> u;
    lists(c, X, u);
    std::vector<uint8_t> mask;
    geom::Rt best;
    const auto t0 = std::chrono::steady_clock::now();
    geom::pnp_ransac(X, u, c.max_iters, 3.0, 0.99, mask, best);
    printf("%d %.4f\n", c.count, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

static int run_scan() {
    long long combos = 0, bad = 0;
    std::vector<int> T(pnp::kMaxN + 1);
    for (int count = 6; count <= pnp::kMaxN; count += count < 300 ? 1 : 97) {
        pnp::fill_T(count, T.data());
        for (int good = 5; good <= count; ++good)
            for (int niters = 1; niters <= pnp::kMaxIters; ++niters) {
                const int ref = geom::ransac_update_num_iters(0.99, (double)(count - good) / count, 5, niters);
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
    if ((!plan && !host && !timing) || (plan && (R < 1 || R > pnp::kMaxIters))) { fprintf(stderr, "usage: pnp_plan_pin plan R | host | time < cases;  pnp_plan_pin scan\n"); return 2; }
    Case c;
    int rc;
    while ((rc = read_case(c)) == 1) {
        if (timing) { run_time(c); continue; }
        Out o;
        o.mask.assign((size_t)c.count, 0); o.inliers.assign((size_t)c.count, -1);
        if (plan) run_plan(c, R, o); else run_host(c, o);
        const int head[7] = {o.status, o.info[0], o.info[1], o.info[2], o.info[3], o.ret, o.n_inliers};
        fwrite(head, sizeof(int), 7, stdout);
        fwrite(o.Rt, 8, 12, stdout); fwrite(o.pose, 8, 12, stdout);
        if (c.count) { fwrite(o.mask.data(), 1, (size_t)c.count, stdout); fwrite(o.inliers.data(), 4, (size_t)c.count, stdout); }
    }
    if (rc < 0) { fprintf(stderr, "pnp_plan_pin: truncated or inconsistent case\n"); return 1; }
    return 0;
}
