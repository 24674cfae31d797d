// host_posegraph_capi.cpp -> lib/libomni_host_posegraph.so: the C entry points of the pose graph of the pipeline's window (KeyframePipeline::Config::pose_graph,
// keyframe_pipeline.hpp; host/pose_graph.hpp).  One library per switch, as before; the handle is the same (host_capi_types.hpp).
#include <cstring>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_posegraph.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
omni::KeyframePipeline& pipe(omni_pipeline* h, const char* who) {
    if (!h) throw std::invalid_argument(std::string(who) + ": null pipeline");
    return *h->p;
}
void put_problem(const omni::SwarmPoseGraph::Problem& P, int sizes[3], double* poses, uint8_t* fixed, int max_poses, omni_pgo_edge* edges, int max_edges) {
    sizes[0] = P.n_poses; sizes[1] = (int)P.edges.size(); sizes[2] = P.n_starts;
    if (poses && max_poses >= P.n_poses && !P.poses.empty()) std::memcpy(poses, P.poses.data(), P.poses.size() * sizeof(double));
    if (fixed && max_poses >= P.n_poses && !P.fixed.empty()) std::memcpy(fixed, P.fixed.data(), P.fixed.size());
    if (edges && max_edges >= (int)P.edges.size() && !P.edges.empty()) std::memcpy(edges, P.edges.data(), P.edges.size() * sizeof(omni_pgo_edge));
}
}  // namespace

extern "C" {

const char* omni_posegraph_host_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_pose_graph(omni_pipeline* h, int on, int window, int starts) {
    try { pipe(h, "omni_pipeline_set_pose_graph").set_pose_graph(on != 0, window, starts); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_pose_graph(omni_pipeline* h, int* on, int* window, int* starts) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_get_pose_graph");
        if (on) *on = p.pose_graph();
        if (window) *window = p.pose_graph_window();
        if (starts) *starts = p.pose_graph_starts();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_optimize(omni_pipeline* h, int* status) {
    try {
        const int st = pipe(h, "omni_pipeline_optimize").optimize();
        if (status) *status = st;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_estimated_poses(omni_pipeline* h, omni_pose_graph_frame* out, int max_frames, int* n_frames) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_estimated_poses");
        if (!n_frames || max_frames < 0 || (!out && max_frames > 0)) throw std::invalid_argument("omni_pipeline_estimated_poses: null argument or a negative count");
        const std::vector<omni::KeyframePipeline::EstimatedPose> est = p.estimated_poses();
        *n_frames = (int)est.size();
        for (int k = 0; k < max_frames && k < (int)est.size(); ++k) {
            const omni::KeyframePipeline::EstimatedPose& f = est[(size_t)k];
            out[k].drone = f.drone; out[k].pose_index = f.pose_index; out[k].keyframe_id = f.keyframe_id;
            for (int q = 0; q < 4; ++q) { out[k].odom[q] = f.odom[q]; out[k].init[q] = f.init[q]; out[k].pose[q] = f.pose[q]; }
        }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_pose_graph_drift(omni_pipeline* h, double out[4], int* valid) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_pose_graph_drift");
        if (!out || !valid) throw std::invalid_argument("omni_pipeline_pose_graph_drift: null argument");
        *valid = p.drift(out) ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_pose_graph_stats(omni_pipeline* h, int64_t out[11], double cost[2]) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_pose_graph_stats");
        if (!out) throw std::invalid_argument("omni_pipeline_pose_graph_stats: null argument");
        const omni::KeyframePipeline::PoseGraphStats st = p.pose_graph_stats();
        for (int i = 0; i < 11; ++i) out[i] = st.v[i];
        if (cost) { cost[0] = st.cost[0]; cost[1] = st.cost[1]; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_pose_graph_problem(omni_pipeline* h, int sizes[3], double* poses, uint8_t* fixed, int max_poses, omni_pgo_edge* edges, int max_edges,
                                     omni_pgo_params* params) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_pose_graph_problem");
        if (!sizes || max_poses < 0 || max_edges < 0) throw std::invalid_argument("omni_pipeline_pose_graph_problem: null argument or a negative count");
        put_problem(p.pose_graph_problem(), sizes, poses, fixed, max_poses, edges, max_edges);
        if (params) *params = p.pose_graph_params();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pose_graph_build_host(int self_id, int window, int starts, double pos_covariance_per_meter, double yaw_covariance_per_meter,
                               const omni_pose_graph_keyframe* keyframes, int n_keyframes, const omni_remote_edge* loops, int n_loops, omni_pose_graph_frame* frames_out,
                               int max_frames, int* n_frames, int sizes[3], double* poses, uint8_t* fixed, int max_poses, omni_pgo_edge* edges, int max_edges, int counts[5]) {
    try {
        if (n_keyframes < 0 || n_loops < 0 || (n_keyframes > 0 && !keyframes) || (n_loops > 0 && !loops) || !n_frames || !sizes || !counts || max_frames < 0 || max_poses < 0 ||
            max_edges < 0 || (!frames_out && max_frames > 0))
            throw std::invalid_argument("omni_pose_graph_build_host: null argument or a negative count");
        if (window < omni::SwarmPoseGraph::kMinWindow || window > omni::SwarmPoseGraph::kMaxWindow) throw std::invalid_argument("omni_pose_graph_build_host: window outside 2..256");
        if (starts < 1 || starts > OMNI_PGO_MAX_STARTS) throw std::invalid_argument("omni_pose_graph_build_host: starts outside 1..64");
        omni::SwarmPoseGraph::Params pr;
        pr.self_id = self_id; pr.window = window; pr.starts = starts; pr.pos_covariance_per_meter = pos_covariance_per_meter; pr.yaw_covariance_per_meter = yaw_covariance_per_meter;
        omni::SwarmPoseGraph g(pr);
        for (int k = 0; k < n_keyframes; ++k) g.note_frame(keyframes[k].drone, keyframes[k].keyframe_id, keyframes[k].pose);
        std::vector<omni::SwarmPoseGraph::Loop> ls;
        for (int k = 0; k < n_loops; ++k) {
            omni::SwarmPoseGraph::Loop l;
            l.id = loops[k].id; l.drone_a = loops[k].drone_id_a; l.drone_b = loops[k].drone_id_b; l.keyframe_a = loops[k].keyframe_id_a; l.keyframe_b = loops[k].keyframe_id_b;
            std::memcpy(l.rel, loops[k].relative_pose, sizeof l.rel); std::memcpy(l.pos_cov, loops[k].pos_cov, sizeof l.pos_cov); std::memcpy(l.ang_cov, loops[k].ang_cov, sizeof l.ang_cov);
            ls.push_back(l);
        }
        const omni::SwarmPoseGraph::Problem P = g.build(ls);
        *n_frames = (int)P.frames.size();
        for (int k = 0; k < max_frames && k < (int)P.frames.size(); ++k) {
            const omni::SwarmPoseGraph::Frame& f = P.frames[(size_t)k];
            frames_out[k].drone = f.drone; frames_out[k].pose_index = f.pose_index; frames_out[k].keyframe_id = f.keyframe_id;
            for (int q = 0; q < 4; ++q) { frames_out[k].odom[q] = f.odom[q]; frames_out[k].init[q] = f.init[q]; frames_out[k].pose[q] = f.init[q]; }
        }
        put_problem(P, sizes, poses, fixed, max_poses, edges, max_edges);
        counts[0] = P.ego_edges; counts[1] = P.loop_edges; counts[2] = P.loops_outside; counts[3] = P.unreachable_drones; counts[4] = P.merged;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
