// LoopGeometry::pnp_ransac (host/loop_geometry.hpp): compute_loop on the frame pairs of tests/test_geometry_cpu.py (the "loop" text protocol of
// tests/cpp/geometry_check.cpp) three times -- without the hook, with the hook fed by geom::pnp_ransac, with the hook fed by csrc/pnp_plan.h
// (pnp::pnp_ransac_host, what the GPU kernel computes; a candidate it hands back returns -1 from the hook) -- and compares every field of the Correspondence and
// of the LoopEdge.  Prints "HOOK <ok> <same as host hook> <same as plan hook> <hook calls> <candidates handed back> <correspondences> <pnp inliers>".
#include <cstdio>
#include <cstring>
#include <iostream>

#include "../../omni-swarm_amd/csrc/pnp_plan.h"
#include "../../omni-swarm_amd/host/loop_geometry.hpp"

extern "C" int oracle_bf_match(const float* q, int nq, const float* t, int nt, int dim, int mode, int* q_idx, int* t_idx, float* dist_out);

using namespace omni;
using namespace omni::geom;

static Pose read_pose() { Pose p; std::cin >> p.pos.x >> p.pos.y >> p.pos.z >> p.att.w >> p.att.x >> p.att.y >> p.att.z; return p; }

static FisheyeFrameDescriptor read_frame() {
    FisheyeFrameDescriptor f;
    int n_img;
    std::cin >> f.msg_id >> f.drone_id >> f.timestamp >> f.landmark_num;
    f.pose_drone = to_msg(read_pose());
    std::cin >> n_img;
    f.images.resize(n_img);
    for (auto& im : f.images) {
        std::cin >> im.landmark_num;
        im.camera_extrinsic = to_msg(read_pose());
        im.pose_drone = f.pose_drone;
        im.drone_id = f.drone_id;
        const int n = im.landmark_num;
        im.landmarks_2d.resize(n); im.landmarks_2d_norm.resize(n); im.landmarks_3d.resize(n); im.landmarks_flag.resize(n); im.feature_descriptor.resize((size_t)n * 64);
        for (int i = 0; i < n; ++i) {
            int flag;
            std::cin >> im.landmarks_2d[i].x >> im.landmarks_2d[i].y >> im.landmarks_2d_norm[i].x >> im.landmarks_2d_norm[i].y >> im.landmarks_3d[i].x >>
                im.landmarks_3d[i].y >> im.landmarks_3d[i].z >> flag;
            im.landmarks_flag[i] = (uint8_t)flag;
            for (int k = 0; k < 64; ++k) std::cin >> im.feature_descriptor[(size_t)i * 64 + k];
        }
    }
    return f;
}

template <typename T> static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T))); }
static bool same(const LoopGeometry::Correspondence& a, const LoopGeometry::Correspondence& b) {
    return same_bytes(a.new_norm_2d, b.new_norm_2d) && same_bytes(a.old_norm_2d, b.old_norm_2d) && same_bytes(a.new_3d, b.new_3d) && same_bytes(a.old_3d, b.old_3d) &&
           a.new_idx == b.new_idx && a.old_idx == b.old_idx && a.dirs_new == b.dirs_new && a.dirs_old == b.dirs_old;
}
static bool same(const Pose& a, const Pose& b) { return !memcmp(&a, &b, sizeof(Pose)); }
static bool same(const LoopEdge& a, const LoopEdge& b) {
    return a.id == b.id && a.keyframe_id_a == b.keyframe_id_a && a.keyframe_id_b == b.keyframe_id_b && a.drone_id_a == b.drone_id_a && a.drone_id_b == b.drone_id_b &&
           a.pnp_inlier_num == b.pnp_inlier_num && a.ts_a == b.ts_a && a.ts_b == b.ts_b && same(a.relative_pose, b.relative_pose) && same(a.self_pose_a, b.self_pose_a) &&
           same(a.self_pose_b, b.self_pose_b) && !memcmp(a.pos_cov, b.pos_cov, sizeof(a.pos_cov)) && !memcmp(a.ang_cov, b.ang_cov, sizeof(a.ang_cov));
}

int main() {
    int dn, dold, init_mode, is4;
    while (std::cin >> dn >> dold >> init_mode >> is4) {
        const FisheyeFrameDescriptor nw = read_frame(), old = read_frame();
        bool ok[3];
        LoopEdge e[3];
        LoopGeometry::Correspondence c[3];
        int calls = 0, handed_back = 0;
        for (int v = 0; v < 3; ++v) {
            LoopGeometry g;
            g.is_4dof = is4 != 0; g.self_id = old.drone_id;
            g.match = [](const float* q, int nq, const float* t, int nt, int dim, std::vector<DMatch>& out) {
                out.clear();
                if (nq <= 0 || nt <= 0) return;
                std::vector<int> qi(nq), ti(nq); std::vector<float> dd(nq);
                const int n = oracle_bf_match(q, nq, t, nt, dim, 0, qi.data(), ti.data(), dd.data());
                for (int i = 0; i < n; ++i) out.push_back({qi[i], ti[i], dd[i]});
            };
            if (v == 1)
                g.pnp_ransac = [&](const std::vector<Vec3>& X, const std::vector<Vec2>& u, int iterations, std::vector<uint8_t>& mask, Rt& best) {
                    ++calls;
                    return pnp_ransac(X, u, iterations, 3.0, 0.99, mask, best) ? 1 : 0;
                };
            if (v == 2)
                g.pnp_ransac = [&](const std::vector<Vec3>& X, const std::vector<Vec2>& u, int iterations, std::vector<uint8_t>& mask, Rt& best) {
                    ++calls;
                    const int n = (int)X.size();
                    if (n > pnp::kMaxN) { ++handed_back; return -1; }
                    std::vector<float> Xf, uf;
                    for (int i = 0; i < n; ++i) { Xf.push_back((float)X[i].x); Xf.push_back((float)X[i].y); Xf.push_back((float)X[i].z); uf.push_back((float)u[i].x); uf.push_back((float)u[i].y); }
                    std::vector<int> T((size_t)n + 1, 0);
                    if (n > 0) pnp::fill_T(n, T.data());
                    double rt[12];
                    int info[4];
                    mask.assign((size_t)n, 0);
                    const int st = pnp::pnp_ransac_host(Xf.data(), uf.data(), n, iterations, T.data(), 64, mask.data(), rt, info);
                    if (st == OMNI_PNP_HOST) { ++handed_back; return -1; }
                    if (st != OMNI_PNP_OK) return 0;
                    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) best.R.m[r][k] = rt[3 * r + k];
                    best.t = {rt[9], rt[10], rt[11]};
                    return 1;
                };
            ok[v] = g.compute_loop(nw, old, dn, dold, e[v], init_mode != 0, &c[v]);
        }
        std::printf("HOOK %d %d %d %d %d %zu %d\n", ok[0] ? 1 : 0, ok[1] == ok[0] && same(c[1], c[0]) && same(e[1], e[0]) ? 1 : 0,
                    ok[2] == ok[0] && same(c[2], c[0]) && same(e[2], e[0]) ? 1 : 0, calls, handed_back, c[0].new_norm_2d.size(), e[0].pnp_inlier_num);
    }
    return 0;
}
