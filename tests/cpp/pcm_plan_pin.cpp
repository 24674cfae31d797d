// csrc/pcm_plan.h alone under g++ (tests/test_pcm_plan_cpu.py builds this twice: plain, and with -fsanitize=address,undefined), heap buffers of exactly the promised
// sizes.  Checks, on seeded scenes of two and three drones:
//   - pair_smd against the same error pose put together from host/geometry.hpp's geom::Pose and std::atan2 (relative difference below 1e-9: the arctangents may
//     differ in the last bits, nothing else does);
//   - edges made from ground-truth poses: smd below 1e-20 in both orientations and for an edge of one drone with itself;
//   - rows_host: symmetric, zero diagonal, degree = popcount, a call for vertices [first, n) returns the rows of the call for all of them, and the degrees add up;
//   - a zero covariance: NaN (0 / 0) or inf, not consistent;
//   - max_clique returns a clique, of the full size on an all-consistent graph.
// usage: pcm_plan_pin <seed>; prints "SMD <largest relative difference>" and "OK"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../omni-swarm_amd/csrc/pcm_plan.h"
#include "../../omni-swarm_amd/host/geometry.hpp"

using namespace omni;

static uint64_t g_state = 1;
static double rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_state >> 11) / 9007199254740992.0 - 0.5; }
static geom::Pose rnd_pose(double tscale, double rscale) {
    geom::Pose p;
    p.pos = {rnd() * tscale, rnd() * tscale, rnd() * tscale};
    p.att = geom::Quat{rscale >= 1 ? rnd() : 1.0, rnd() * rscale, rnd() * rscale, rnd() * rscale}.normalized();
    return p;
}
static void put(double* d, const geom::Pose& p) { d[0] = p.pos.x; d[1] = p.pos.y; d[2] = p.pos.z; d[3] = p.att.w; d[4] = p.att.x; d[5] = p.att.y; d[6] = p.att.z; }
static geom::Pose get(const double* d) { return {{d[0], d[1], d[2]}, geom::Quat{d[3], d[4], d[5], d[6]}}; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Scene {
    int steps = 60;
    std::vector<geom::Pose> G;
    std::vector<std::vector<geom::Pose>> P;
    std::vector<std::vector<double>> arc;
    explicit Scene(int drones) {
        for (int d = 0; d < drones; ++d) {
            G.push_back(rnd_pose(8, 1));
            std::vector<geom::Pose> p;
            std::vector<double> a;
            geom::Pose cur = rnd_pose(2, 1);
            double len = 0;
            for (int t = 0; t < steps; ++t) {
                const geom::Pose nxt = cur * rnd_pose(0.8, 0.1);
                len += geom::norm(nxt.pos - cur.pos);
                cur = nxt;
                p.push_back(cur); a.push_back(len);
            }
            P.push_back(p); arc.push_back(a);
        }
    }
    omni_pcm_edge edge(int64_t id, int a, int b, double noise, bool displaced) const {
        const int ta = (int)((rnd() + 0.5) * steps) % steps, tb = (int)((rnd() + 0.5) * steps) % steps;
        geom::Pose rel = (G[a] * P[a][ta]).inverse() * (G[b] * P[b][tb]);
        if (noise > 0) rel = rel * rnd_pose(noise, noise * 0.5);
        if (displaced) rel = rel * rnd_pose(6, 1);
        omni_pcm_edge e;
        e.id = id; e.drone_a = a; e.drone_b = b;
        put(e.relative_pose, rel); put(e.self_pose_a, P[a][ta]); put(e.self_pose_b, P[b][tb]);
        e.arc_a = arc[a][ta]; e.arc_b = arc[b][tb];
        for (int k = 0; k < 3; ++k) { e.pos_cov[k] = 0.05; e.ang_cov[k] = 0.05; }
        return e;
    }
};

// the error pose from geom::Pose, the log map with std::atan2
static double smd_geom(const omni_pcm_edge& e1, const omni_pcm_edge& e2, int orient, const omni_pcm_params& pr) {
    const bool sw = orient == 2;
    const geom::Pose p1 = get(e1.relative_pose), p2 = sw ? get(e2.relative_pose).inverse() : get(e2.relative_pose);
    const geom::Pose oa = get(e1.self_pose_a).inverse() * get(sw ? e2.self_pose_b : e2.self_pose_a), ob = get(e1.self_pose_b).inverse() * get(sw ? e2.self_pose_a : e2.self_pose_b);
    const geom::Pose dp = oa * p2 * ob.inverse() * p1.inverse();
    const geom::Quat q = dp.att.w < 0 ? geom::Quat{-dp.att.w, -dp.att.x, -dp.att.y, -dp.att.z} : dp.att;
    const double vn = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z), ang = 2 * std::atan2(vn, q.w), k = vn > 1e-12 ? ang / vn : 2.0;
    const double v[6] = {dp.pos.x, dp.pos.y, dp.pos.z, k * q.x, k * q.y, k * q.z};
    const double la = std::fabs((sw ? e2.arc_b : e2.arc_a) - e1.arc_a), lb = std::fabs((sw ? e2.arc_a : e2.arc_b) - e1.arc_b);
    double s = 0;
    for (int i = 0; i < 6; ++i) {
        const double per = i < 3 ? pr.pos_covariance_per_meter : pr.yaw_covariance_per_meter;
        s += v[i] * v[i] / ((i < 3 ? e1.pos_cov[i] + e2.pos_cov[i] : e1.ang_cov[i - 3] + e2.ang_cov[i - 3]) + (la * per + lb * per));
    }
    return s;
}

static bool bit(const uint64_t* rows, int stride, int i, int j) { return (rows[(size_t)i * stride + (j >> 6)] >> (j & 63)) & 1; }

int main(int argc, char** argv) {
    g_state = argc > 1 ? (uint64_t)atoll(argv[1]) * 2654435761ull + 1 : 1;
    const omni_pcm_params pr{0.6, 0.01, 0.003};
    double worst = 0;
    int consistent_pairs = 0, inconsistent_pairs = 0, orient_seen[3] = {0, 0, 0};
    for (int n : {1, 2, 63, 64, 65, 130}) {
        Scene sc(3);
        std::vector<omni_pcm_edge> e;
        for (int k = 0; k < n; ++k) {
            const double r = rnd() + 0.5;
            int a = r < 0.5 ? 0 : 1, b = 1 - a;
            if (r > 0.8) { a = 2; b = 0; }
            if (r > 0.9) { a = b = 1; }
            e.push_back(sc.edge(100 + k, a, b, 0.07, rnd() > 0.25));
        }
        const int stride = (n + 63) / 64;
        std::vector<uint64_t> rows((size_t)n * stride);
        std::vector<int32_t> deg((size_t)n);
        std::vector<double> smd((size_t)n * n);
        pcm::rows_host(e.data(), n, 0, pr, stride, rows.data(), deg.data(), smd.data());
        for (int i = 0; i < n; ++i) {
            int d = 0;
            CHECK(!bit(rows.data(), stride, i, i));
            for (int j = 0; j < n; ++j) { CHECK(bit(rows.data(), stride, i, j) == bit(rows.data(), stride, j, i)); d += bit(rows.data(), stride, i, j); }
            for (int j = n; j < stride * 64; ++j) CHECK(!bit(rows.data(), stride, i, j));
            CHECK(d == deg[(size_t)i]);
            for (int j = 0; j < i; ++j) {
                const int o = pcm::same_robot_pair(e[i].drone_a, e[i].drone_b, e[j].drone_a, e[j].drone_b);
                ++orient_seen[o];
                if (!o) { CHECK(!bit(rows.data(), stride, i, j) && smd[(size_t)i * n + j] == 0); continue; }
                const double s = smd[(size_t)i * n + j], g = smd_geom(e[i], e[j], o, pr);
                const double rel = std::fabs(s - g) / (std::fabs(g) > 1e-300 ? std::fabs(g) : 1e-300);
                if (rel > worst) worst = rel;
                CHECK(bit(rows.data(), stride, i, j) == (s < pr.pcm_thres));
                (s < pr.pcm_thres ? consistent_pairs : inconsistent_pairs)++;
            }
        }
        // the same graph in two calls
        for (int first : {1, n / 2, n - 1}) {
            if (first < 1 || first >= n) continue;
            std::vector<uint64_t> r0((size_t)first * stride), r1((size_t)(n - first) * stride);
            std::vector<int32_t> d0((size_t)first), d1((size_t)n);
            pcm::rows_host(e.data(), first, 0, pr, stride, r0.data(), d0.data(), nullptr);
            pcm::rows_host(e.data(), n, first, pr, stride, r1.data(), d1.data(), nullptr);
            for (int i = first; i < n; ++i) for (int w = 0; w < stride; ++w) CHECK(r1[(size_t)(i - first) * stride + w] == rows[(size_t)i * stride + w]);
            for (int i = 0; i < n; ++i) CHECK((i < first ? d0[(size_t)i] : 0) + d1[(size_t)i] == deg[(size_t)i]);
        }
        // the clique
        std::vector<int32_t> cd((size_t)n), clique((size_t)n), cur((size_t)n);
        std::vector<uint64_t> work((size_t)2 * stride);
        const int size = pcm::max_clique(rows.data(), n, stride, cd.data(), work.data(), clique.data(), cur.data());
        CHECK(size >= 1 && size <= n);
        for (int x = 0; x < size; ++x) for (int y = 0; y < x; ++y) CHECK(clique[(size_t)x] != clique[(size_t)y] && bit(rows.data(), stride, clique[(size_t)x], clique[(size_t)y]));
    }
    CHECK(worst < 1e-9 && consistent_pairs > 100 && inconsistent_pairs > 100 && orient_seen[0] > 100 && orient_seen[1] > 100 && orient_seen[2] > 100);
    printf("SMD %.3e\n", worst);
    {   // ground truth: the error pose is the identity
        Scene sc(2);
        const omni_pcm_edge ab = sc.edge(1, 0, 1, 0, false), ab2 = sc.edge(2, 0, 1, 0, false), ba = sc.edge(3, 1, 0, 0, false), aa = sc.edge(4, 0, 0, 0, false), aa2 = sc.edge(5, 0, 0, 0, false);
        double s = 1;
        CHECK(pcm::pair_smd(pcm::load(ab2), pcm::load(ab), 0.01, 0.003, &s) == 1 && s < 1e-20);
        CHECK(pcm::pair_smd(pcm::load(ba), pcm::load(ab), 0.01, 0.003, &s) == 2 && s < 1e-20);
        CHECK(pcm::pair_smd(pcm::load(ab), pcm::load(ba), 0.01, 0.003, &s) == 2 && s < 1e-20);
        CHECK(pcm::pair_smd(pcm::load(aa2), pcm::load(aa), 0.01, 0.003, &s) == 1 && s < 1e-20);
        CHECK(pcm::pair_smd(pcm::load(aa), pcm::load(ab), 0.01, 0.003, &s) == 0);
        printf("GT %.3e\n", s);
        // zero covariances: the same frames (arc difference 0) and zero edge covariances -> 0 / 0 or x / 0
        omni_pcm_edge z1 = ab, z2 = ab;
        for (int k = 0; k < 3; ++k) z1.pos_cov[k] = z1.ang_cov[k] = z2.pos_cov[k] = z2.ang_cov[k] = 0;
        z2.id = 9;
        const int o = pcm::pair_smd(pcm::load(z2), pcm::load(z1), 0.01, 0.003, &s);
        CHECK(o == 1 && !(s < 0.6) && !pcm::consistent(o, s, 0.6) && (std::isnan(s) || std::isinf(s)));
    }
    {   // an all-consistent graph of 130 vertices: the clique is everything
        const int n = 130, stride = 3;
        std::vector<uint64_t> rows((size_t)n * stride, 0);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) if (i != j) rows[(size_t)i * stride + (j >> 6)] |= 1ull << (j & 63);
        std::vector<int32_t> cd((size_t)n), clique((size_t)n), cur((size_t)n);
        std::vector<uint64_t> work((size_t)2 * stride);
        CHECK(pcm::max_clique(rows.data(), n, stride, cd.data(), work.data(), clique.data(), cur.data()) == n && clique[0] == 0 && clique[1] == n - 1);
        CHECK(pcm::max_clique(rows.data(), 0, stride, cd.data(), work.data(), clique.data(), cur.data()) == 0);
    }
    // the arctangent's edge values
    const double pi = 3.141592653589793, inf = __builtin_huge_val();
    CHECK(pcm::atan2_plan(0.0, 1.0) == 0 && !std::signbit(pcm::atan2_plan(0.0, 1.0)) && std::signbit(pcm::atan2_plan(-0.0, 1.0)));
    CHECK(pcm::atan2_plan(0.0, -1.0) == pi && pcm::atan2_plan(-0.0, -0.0) == -pi && pcm::atan2_plan(0.0, 0.0) == 0 && pcm::atan2_plan(1.0, 0.0) == pi / 2);
    CHECK(pcm::atan2_plan(inf, inf) == pi / 4 && pcm::atan2_plan(1.0, inf) == 0 && pcm::atan2_plan(-inf, 1.0) == -pi / 2 && std::isnan(pcm::atan2_plan(NAN, 1.0)));
    printf("OK\n");
    return 0;
}
