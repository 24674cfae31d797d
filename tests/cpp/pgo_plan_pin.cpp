// csrc/pgo_plan.h alone under g++ (tests/test_pgo_plan_cpu.py builds this twice: plain, and with -fsanitize=address,undefined), heap buffers of exactly the promised
// sizes.  Checks, on seeded graphs:
//   - delta_pose / pose_mul / pose_inverse / yaw_of_quat against geom::Pose::DeltaPose(a, b, true), operator* and yaw() of host/geometry.hpp (1e-12: the sines,
//     cosines and arctangents may differ in the last bits, nothing else does);
//   - reduce() against the same tree written as a recursion, bit for bit, at counts around the chunk and batch boundaries;
//   - plan_graph: every edge twice, ascending per pose, offsets[n] = 2 m;
//   - solve_host on a chain with a loop made from ground truth: CONVERGED, final cost below 1e-18, poses within 1e-9; two starts, best = the cheaper;
//   - the statuses EMPTY (all fixed; no edge) and NONFINITE (an infinite sqrt_inf) with the poses returned untouched; every refusal.
// usage: pgo_plan_pin <seed>; prints "OK"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/pgo_plan.h"
#include "../../omni-swarm_amd/host/geometry.hpp"

using namespace omni;

static uint64_t g_state = 1;
static double rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_state >> 11) / 9007199254740992.0 - 0.5; }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static geom::Pose to_pose(const double* p) { return {{p[0], p[1], p[2]}, geom::quat_from_yaw(p[3])}; }
static double wrap_diff(double a, double b) { return std::fabs(std::remainder(a - b, 2 * M_PI)); }
static bool close_pose(const double* p, const geom::Pose& g, double tol) {
    return std::fabs(p[0] - g.pos.x) < tol && std::fabs(p[1] - g.pos.y) < tol && std::fabs(p[2] - g.pos.z) < tol && wrap_diff(p[3], g.yaw()) < tol;
}
static double tree(const double* v, int l, int s) { return s == pgo::kChunk ? v[l] : tree(v, l, 2 * s) + tree(v, l + s, 2 * s); }

int main(int argc, char** argv) {
    g_state = argc > 1 ? (uint64_t)atoll(argv[1]) * 2654435761ull + 1 : 1;
    // ---- the pose algebra
    for (int k = 0; k < 2000; ++k) {
        const double a[4] = {rnd() * 20, rnd() * 20, rnd() * 4, rnd() * 2 * M_PI}, b[4] = {rnd() * 20, rnd() * 20, rnd() * 4, rnd() * 2 * M_PI};
        double d[4], m[4], inv[4], id[4];
        pgo::delta_pose(a, b, d);
        CHECK(close_pose(d, geom::Pose::DeltaPose(to_pose(a), to_pose(b), true), 1e-12));
        CHECK(d[3] >= -M_PI && d[3] < M_PI);
        pgo::pose_mul(a, b, m);
        CHECK(close_pose(m, to_pose(a) * to_pose(b), 1e-12));
        pgo::pose_inverse(a, inv);
        pgo::pose_mul(a, inv, id);
        CHECK(std::fabs(id[0]) < 1e-13 && std::fabs(id[1]) < 1e-13 && std::fabs(id[2]) < 1e-13 && wrap_diff(id[3], 0) < 1e-13);
        const geom::Quat q = geom::Quat{rnd(), rnd() * 0.2, rnd() * 0.2, rnd()}.normalized();
        CHECK(wrap_diff(pgo::yaw_of_quat(q.w, q.x, q.y, q.z), geom::quat2eulers(q).z) < 1e-14);
    }
    // ---- the fixed-shape sum
    {
        const int counts[] = {1, 2, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4100};
        for (int count : counts) {
            double* v = new double[count];
            for (int k = 0; k < count; ++k) v[k] = rnd() * std::pow(10.0, (int)(rnd() * 12));
            double* red = new double[pgo::kRedDoubles];
            pgo::HostTeam team;
            team.red = red;
            const double got = pgo::reduce(team, count, [&](int k) { return v[k]; });
            double want = 0.0, pad[pgo::kChunk];
            for (int base = 0; base < count; base += pgo::kChunk) {
                for (int l = 0; l < pgo::kChunk; ++l) pad[l] = base + l < count ? v[base + l] : 0.0;
                want = want + tree(pad, 0, 1);
            }
            CHECK(std::memcmp(&got, &want, 8) == 0);
            delete[] v; delete[] red;
        }
    }
    // ---- a chain with a loop, from ground truth
    const int n = 40, m = n;
    double* truth = new double[4 * n];
    truth[0] = rnd(); truth[1] = rnd(); truth[2] = rnd(); truth[3] = rnd() * 6;
    for (int k = 1; k < n; ++k) {
        const double step[4] = {0.5 + 0.3 * rnd(), 0.2 * rnd(), 0.1 * rnd(), 0.6 * rnd()};
        pgo::pose_mul(truth + 4 * (k - 1), step, truth + 4 * k);
    }
    omni_pgo_edge* edges = new omni_pgo_edge[m];
    for (int e = 0; e < m; ++e) {
        edges[e].i = e < n - 1 ? e : n - 1; edges[e].j = e < n - 1 ? e + 1 : 0; edges[e].robust = e >= n - 1; edges[e].reserved = 0;
        pgo::delta_pose(truth + 4 * edges[e].i, truth + 4 * edges[e].j, edges[e].z);
        for (int q = 0; q < 4; ++q) edges[e].sqrt_inf[q] = pgo::sqrt_inf_of_cov(q < 3 ? 0.01 : 0.003);
    }
    uint8_t* fixed = new uint8_t[n];
    for (int k = 0; k < n; ++k) fixed[k] = k == 0;
    {
        int32_t* off = new int32_t[n + 1];
        int32_t* inc = new int32_t[2 * m];
        uint8_t* act = new uint8_t[n];
        CHECK(pgo::plan_graph(fixed, edges, n, m, off, inc, act) == n - 1);
        CHECK(off[0] == 0 && off[n] == 2 * m && !act[0] && act[1]);
        std::vector<int> seen(2 * m, 0);
        for (int p = 0; p < n; ++p)
            for (int k = off[p]; k < off[p + 1]; ++k) {
                CHECK(inc[k] >= 0 && inc[k] < 2 * m && !seen[inc[k]]++);
                CHECK(((inc[k] & 1) ? edges[inc[k] >> 1].j : edges[inc[k] >> 1].i) == p);
                CHECK(k == off[p] || inc[k] > inc[k - 1]);
            }
        delete[] off; delete[] inc; delete[] act;
    }
    double* in = new double[2 * 4 * n];
    double* out = new double[2 * 4 * n];
    omni_pgo_stats* st = new omni_pgo_stats[2];
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 4 * n; ++k) in[s * 4 * n + k] = truth[k] + (k < 4 ? 0.0 : (s ? 0.02 : 0.3) * rnd());
    omni_pgo_params pr = pgo::default_params();
    pr.function_tolerance = 0; pr.parameter_tolerance = 1e-13; pr.cg_tolerance = 1e-10; pr.max_iterations = 100;
    int best = -2;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 2, out, st, &best) == nullptr);
    for (int s = 0; s < 2; ++s) {
        CHECK(st[s].status == OMNI_PGO_CONVERGED && st[s].final_cost < 1e-18 && st[s].initial_cost > 1e-3 && st[s].iterations >= 1 && st[s].cg_iterations >= 1);
        for (int k = 0; k < 4 * n; ++k) CHECK(std::fabs(out[s * 4 * n + k] - truth[k]) < 1e-9);
    }
    CHECK(best == (st[1].final_cost < st[0].final_cost ? 1 : 0));
    printf("COST %.3e %.3e\n", st[0].final_cost, st[1].final_cost);
    // ---- statuses
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, 0, 1, out, st, &best) == nullptr && st[0].status == OMNI_PGO_EMPTY && best == -1 && std::memcmp(in, out, 32 * n) == 0);
    for (int k = 0; k < n; ++k) fixed[k] = 1;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) == nullptr && st[0].status == OMNI_PGO_EMPTY && std::memcmp(in, out, 32 * n) == 0);
    for (int k = 0; k < n; ++k) fixed[k] = k == 0;
    edges[5].sqrt_inf[1] = pgo::sqrt_inf_of_cov(0.0);
    CHECK(std::isinf(edges[5].sqrt_inf[1]));
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) == nullptr && st[0].status == OMNI_PGO_NONFINITE && best == -1 && std::memcmp(in, out, 32 * n) == 0);
    CHECK(!pgo::finite_plan(st[0].final_cost));
    edges[5].sqrt_inf[1] = 10;
    pr.max_iterations = 1; pr.function_tolerance = 0; pr.parameter_tolerance = 0;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) == nullptr && st[0].status == OMNI_PGO_MAX_ITERATIONS && st[0].iterations == 1 && best == 0);
    // ---- refusals
    pr = pgo::default_params();
    CHECK(pgo::solve_host(pr, in, fixed, edges, 0, m, 1, out, st, &best) != nullptr);
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 0, out, st, &best) != nullptr && pgo::solve_host(pr, in, fixed, edges, n, m, 65, out, st, &best) != nullptr);
    CHECK(pgo::graph_refusal(edges, OMNI_PGO_MAX_POSES + 1, 0) && pgo::graph_refusal(edges, n, OMNI_PGO_MAX_EDGES + 1) && pgo::graph_refusal(edges, n, -1));
    edges[3].j = n;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) != nullptr);
    edges[3].j = edges[3].i;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) != nullptr);
    edges[3].j = 4;
    pr.initial_lambda = 0;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) != nullptr);
    pr = pgo::default_params(); pr.max_cg_iterations = -1;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) != nullptr);
    pr = pgo::default_params(); pr.function_tolerance = NAN;
    CHECK(pgo::solve_host(pr, in, fixed, edges, n, m, 1, out, st, &best) != nullptr);
    delete[] truth; delete[] edges; delete[] fixed; delete[] in; delete[] out; delete[] st;
    printf("OK\n");
    return 0;
}
