// pose_graph.hpp -- SwarmPoseGraph: the loop + ego-motion part of swarm_localization's sliding-window problem (swarm_localization_solver.cpp:1064-1100
// setup_problem_with_loops_and_detections, :1156-1213 setup_problem_with_ego_motion, :218-269 init_pose_by_loops) built from what the key-frame pipeline keeps: the
// key frames it saw per drone with their pose_drone, and the loop edges good_edges() returns.  The arithmetic (4-DoF pose algebra, yaw of a quaternion, the square-root
// information) is csrc/pgo_plan.h's; the problem built here is what omni_pgo_solve_multi / omni_pgo_solve_host take.
//
//   poses        the last `window` key frames of every drone, pose_drone reduced to x y z yaw.  Consecutive key frames of a drone whose reduced poses are identical
//                (a zero-length step) share ONE pose of the problem, as :1176 skips identical blocks; they are counted in `merged`.
//   ego motion   one edge between consecutive poses of a drone: z = DeltaPose of the two odometry poses, cov = step length x (pos_covariance_per_meter x 3,
//                yaw_covariance_per_meter), sqrt_inf = 1 / sqrt(cov), no loss.
//   loops        the edges given whose two frames are in the window and whose drones are in the problem: z = the relative pose's x y z yaw, sqrt_inf = 1 / sqrt(pos_cov
//                xyz, ang_cov[2]), robust.  An edge between two frames merged into one pose says nothing and is left out with the ones outside the window.
//   initial      this drone's poses start at their odometry.  Another drone's frame is placed as init_pose_by_loops does: breadth-first from this drone, the drones
//                taken from a queue, the edges scanned in the order given; the first edge that joins a placed drone's frame a with a frame b of a drone not yet
//                placed gives offset = P_a . rel . inverse(P_b) (rel inverted when the edge runs the other way), P_a the frame's INITIAL pose and P_b its odometry
//                pose, and every pose of that drone starts at offset . odometry.  A drone no edge reaches is left out of the problem and counted.
//   constant     the oldest window pose of this drone.
//   starts       start 0 is the above; start k > 0 of K turns every other drone's initial poses about that drone's oldest window pose by a yaw of 2 pi k / K
//                (solve_with_multiple_init, :781-846, draws its other starts at random; these are fixed).
#pragma once
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../csrc/pgo_plan.h"

namespace omni {

class SwarmPoseGraph {
public:
    struct Params {
        int self_id = 1, window = 50, starts = 1;
        double pos_covariance_per_meter = 0.01, yaw_covariance_per_meter = 0.003;
    };
    struct Loop { int64_t id = 0; int drone_a = 0, drone_b = 0; int64_t keyframe_a = 0, keyframe_b = 0; double rel[7] = {0, 0, 0, 1, 0, 0, 0}, pos_cov[3] = {0, 0, 0}, ang_cov[3] = {0, 0, 0}; };
    struct Frame { int drone = 0, pose_index = -1; int64_t keyframe_id = 0; double odom[4] = {0, 0, 0, 0}, init[4] = {0, 0, 0, 0}; };
    struct Problem {
        std::vector<Frame> frames;                 // every window frame of every drone in the problem, drones ascending, oldest first
        int n_poses = 0, n_starts = 1;
        std::vector<double> poses;                 // [n_starts][n_poses][4]
        std::vector<uint8_t> fixed;                // [n_poses]
        std::vector<omni_pgo_edge> edges;          // ego motion first (drones ascending), then the loops in the order given
        int ego_edges = 0, loop_edges = 0, loops_outside = 0, unreachable_drones = 0, merged = 0;
    };
    static constexpr int kMinWindow = 2, kMaxWindow = 256;

    explicit SwarmPoseGraph(const Params& p) : p_(p) {}
    const Params& params() const { return p_; }

    // a key frame this pipeline saw, local or remote, in the order they came; pose7 = xyz + quaternion wxyz
    void note_frame(int drone, int64_t keyframe_id, const double* pose7) {
        Track& t = tracks_[drone];
        Seen s;
        s.keyframe_id = keyframe_id;
        s.odom[0] = pose7[0]; s.odom[1] = pose7[1]; s.odom[2] = pose7[2]; s.odom[3] = pgo::yaw_of_quat(pose7[3], pose7[4], pose7[5], pose7[6]);
        t.push_back(s);
        while ((int)t.size() > kMaxWindow) t.pop_front();           // nothing older than the largest window is ever read
    }
    static void reduce_pose(const double* pose7, double* out4) { out4[0] = pose7[0]; out4[1] = pose7[1]; out4[2] = pose7[2]; out4[3] = pgo::yaw_of_quat(pose7[3], pose7[4], pose7[5], pose7[6]); }

    Problem build(const std::vector<Loop>& loops) const {
        Problem P;
        P.n_starts = p_.starts;
        // the window frames of every drone, by (drone, key frame)
        std::map<int, std::vector<Seen>> win;
        std::map<std::pair<int, int64_t>, int> at;                  // -> index in win[drone]
        for (const auto& kv : tracks_) {
            const Track& t = kv.second;
            const size_t first = t.size() > (size_t)p_.window ? t.size() - (size_t)p_.window : 0;
            std::vector<Seen>& w = win[kv.first];
            for (size_t k = first; k < t.size(); ++k) { at[{kv.first, t[k].keyframe_id}] = (int)w.size(); w.push_back(t[k]); }
        }
        // breadth-first placement of the other drones
        std::map<int, std::vector<double>> offset;                  // drone -> its frame in this drone's (4 doubles)
        if (win.count(p_.self_id)) {
            offset[p_.self_id] = {0, 0, 0, 0};
            std::deque<int> queue{p_.self_id};
            while (!queue.empty()) {
                const int d = queue.front();
                queue.pop_front();
                for (const Loop& e : loops) {
                    const bool fwd = e.drone_a == d && !offset.count(e.drone_b), bwd = e.drone_b == d && !offset.count(e.drone_a);
                    if (!fwd && !bwd) continue;
                    const auto ia = at.find({e.drone_a, e.keyframe_a}), ib = at.find({e.drone_b, e.keyframe_b});
                    if (ia == at.end() || ib == at.end()) continue;
                    double rel[4], inv[4], pa[4], t1[4], off[4];
                    reduce_pose(e.rel, rel);
                    const int other = fwd ? e.drone_b : e.drone_a;
                    const double* od_here = win[d][(size_t)(fwd ? ia : ib)->second].odom;
                    const double* od_other = win[other][(size_t)(fwd ? ib : ia)->second].odom;
                    if (!fwd) { pgo::pose_inverse(rel, inv); std::memcpy(rel, inv, sizeof rel); }
                    pgo::pose_mul(offset[d].data(), od_here, pa);
                    pgo::pose_mul(pa, rel, t1);
                    pgo::pose_inverse(od_other, inv);
                    pgo::pose_mul(t1, inv, off);
                    offset[other] = {off[0], off[1], off[2], off[3]};
                    queue.push_back(other);
                }
            }
        }
        for (const auto& kv : win) if (!offset.count(kv.first)) ++P.unreachable_drones;
        // poses and ego-motion edges
        std::map<std::pair<int, int64_t>, int> pose_of;
        std::vector<std::pair<int, int>> first_pose;                // per drone in the problem: (drone, its oldest pose)
        std::vector<double> init;
        for (const auto& kv : win) {
            if (!offset.count(kv.first)) continue;
            const std::vector<Seen>& w = kv.second;
            first_pose.push_back({kv.first, P.n_poses});
            for (size_t k = 0; k < w.size(); ++k) {
                const bool same = k > 0 && std::memcmp(w[k].odom, w[k - 1].odom, sizeof w[k].odom) == 0;
                Frame f;
                f.drone = kv.first; f.keyframe_id = w[k].keyframe_id;
                std::memcpy(f.odom, w[k].odom, sizeof f.odom);
                pgo::pose_mul(offset[kv.first].data(), w[k].odom, f.init);
                if (same) { ++P.merged; f.pose_index = P.n_poses - 1; }
                else {
                    f.pose_index = P.n_poses++;
                    init.insert(init.end(), f.init, f.init + 4);
                    if (k > 0) {
                        omni_pgo_edge e;
                        std::memset(&e, 0, sizeof e);
                        e.i = f.pose_index - 1; e.j = f.pose_index;
                        pgo::delta_pose(w[k - 1].odom, w[k].odom, e.z);
                        const double dx = w[k].odom[0] - w[k - 1].odom[0], dy = w[k].odom[1] - w[k - 1].odom[1], dz = w[k].odom[2] - w[k - 1].odom[2];
                        const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
                        for (int q = 0; q < 4; ++q) e.sqrt_inf[q] = pgo::sqrt_inf_of_cov(len * (q < 3 ? p_.pos_covariance_per_meter : p_.yaw_covariance_per_meter));
                        P.edges.push_back(e);
                        ++P.ego_edges;
                    }
                }
                pose_of[{f.drone, f.keyframe_id}] = f.pose_index;
                P.frames.push_back(f);
            }
        }
        // loop edges
        for (const Loop& l : loops) {
            const auto ia = pose_of.find({l.drone_a, l.keyframe_a}), ib = pose_of.find({l.drone_b, l.keyframe_b});
            if (ia == pose_of.end() || ib == pose_of.end() || ia->second == ib->second) { ++P.loops_outside; continue; }
            omni_pgo_edge e;
            std::memset(&e, 0, sizeof e);
            e.i = ia->second; e.j = ib->second; e.robust = 1;
            reduce_pose(l.rel, e.z);
            for (int q = 0; q < 4; ++q) e.sqrt_inf[q] = pgo::sqrt_inf_of_cov(q < 3 ? l.pos_cov[q] : l.ang_cov[2]);
            P.edges.push_back(e);
            ++P.loop_edges;
        }
        // the constant pose and the starts
        P.fixed.assign((size_t)P.n_poses, 0);
        for (const auto& fp : first_pose) if (fp.first == p_.self_id) P.fixed[(size_t)fp.second] = 1;
        P.poses.resize((size_t)P.n_starts * init.size());
        for (int s = 0; s < P.n_starts; ++s) {
            double* x = P.poses.data() + (size_t)s * init.size();
            std::memcpy(x, init.data(), init.size() * sizeof(double));
            if (s == 0) continue;
            const double turn[4] = {0, 0, 0, pgo::normalize_angle(2.0 * 3.14159265358979323846 * s / P.n_starts)};
            for (size_t d = 0; d < first_pose.size(); ++d) {
                if (first_pose[d].first == p_.self_id) continue;
                const int lo = first_pose[d].second, hi = d + 1 < first_pose.size() ? first_pose[d + 1].second : P.n_poses;
                double pivot[4], inv[4], t1[4], t2[4];
                std::memcpy(pivot, init.data() + 4 * (size_t)lo, sizeof pivot);
                pgo::pose_inverse(pivot, inv);
                for (int v = lo; v < hi; ++v) {                      // pivot . turn . inverse(pivot) . pose
                    pgo::pose_mul(inv, init.data() + 4 * (size_t)v, t1);
                    pgo::pose_mul(turn, t1, t2);
                    pgo::pose_mul(pivot, t2, x + 4 * (size_t)v);
                }
            }
        }
        return P;
    }

private:
    struct Seen { int64_t keyframe_id = 0; double odom[4] = {0, 0, 0, 0}; };
    typedef std::deque<Seen> Track;
    Params p_;
    std::map<int, Track> tracks_;
};

}  // namespace omni
