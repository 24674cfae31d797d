// host_pcm_capi.cpp -> lib/libomni_host_pcm.so: the C entry points of the pairwise-consistency stage (KeyframePipeline::Config::pcm, keyframe_pipeline.hpp;
// host/loop_outlier_rejection.hpp).  One library per switch, as before; the handle is the same (host_capi_types.hpp).
#include <cstring>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_pcm.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
omni::KeyframePipeline& pipe(omni_pipeline* h, const char* who) {
    if (!h) throw std::invalid_argument(std::string(who) + ": null pipeline");
    return *h->p;
}
void put_pose(double* out, const omni::geom::Pose& p) { out[0] = p.pos.x; out[1] = p.pos.y; out[2] = p.pos.z; out[3] = p.att.w; out[4] = p.att.x; out[5] = p.att.y; out[6] = p.att.z; }
}  // namespace

extern "C" {

const char* omni_pcm_host_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_pcm(omni_pipeline* h, int on, double pcm_thres, int redundant, int capacity) {
    try { pipe(h, "omni_pipeline_set_pcm").set_pcm(on != 0, pcm_thres, redundant != 0, capacity); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_pcm(omni_pipeline* h, int* on, double* pcm_thres, int* redundant, int* capacity) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_get_pcm");
        if (on) *on = p.pcm();
        if (pcm_thres) *pcm_thres = p.pcm_thres();
        if (redundant) *redundant = p.pcm_redundant();
        if (capacity) *capacity = p.pcm_capacity();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_good_edges(omni_pipeline* h, omni_remote_edge* out, int max_edges, int* n_edges) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_good_edges");
        if (!n_edges || max_edges < 0 || (!out && max_edges > 0)) throw std::invalid_argument("omni_pipeline_good_edges: null argument or a negative count");
        const std::vector<omni::LoopEdge> edges = p.good_edges();
        *n_edges = (int)edges.size();
        for (int k = 0; k < max_edges && k < (int)edges.size(); ++k) {
            const omni::LoopEdge& e = edges[(size_t)k];
            omni_remote_edge& o = out[k];
            o.id = e.id; o.keyframe_id_a = e.keyframe_id_a; o.keyframe_id_b = e.keyframe_id_b; o.drone_id_a = e.drone_id_a; o.drone_id_b = e.drone_id_b;
            o.pnp_inlier_num = e.pnp_inlier_num; o.reserved = 0; o.ts_a = e.ts_a; o.ts_b = e.ts_b;
            put_pose(o.relative_pose, e.relative_pose); put_pose(o.self_pose_a, e.self_pose_a); put_pose(o.self_pose_b, e.self_pose_b);
            std::memcpy(o.pos_cov, e.pos_cov, sizeof o.pos_cov); std::memcpy(o.ang_cov, e.ang_cov, sizeof o.ang_cov);
        }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_pcm_stats(omni_pipeline* h, int64_t out[6]) {
    try {
        if (!out) throw std::invalid_argument("omni_pipeline_pcm_stats: null argument");
        pipe(h, "omni_pipeline_pcm_stats").pcm_stats(out);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_pcm_records(omni_pipeline* h, omni_pcm_edge* out, int max_edges, int* n_edges) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_pcm_records");
        if (!n_edges || max_edges < 0 || (!out && max_edges > 0)) throw std::invalid_argument("omni_pipeline_pcm_records: null argument or a negative count");
        const std::vector<omni_pcm_edge>& r = p.pcm_records();
        *n_edges = (int)r.size();
        for (int k = 0; k < max_edges && k < (int)r.size(); ++k) out[k] = r[(size_t)k];
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pcm_filter_host(const omni_pcm_edge* edges, int n, const int* batch, int n_batches, int self_id, int redundant, int capacity, const omni_pcm_params* params,
                         uint8_t* good_out, int64_t stats_out[6]) {
    try {
        if (n < 0 || (n > 0 && (!edges || !good_out)) || !params || (batch && n_batches < 0)) throw std::invalid_argument("omni_pcm_filter_host: null argument or a negative count");
        omni::LoopOutlierRejection::Params p;
        p.self_id = self_id; p.redundant = redundant != 0; p.capacity = capacity; p.pcm = *params;
        omni::LoopOutlierRejection lor(nullptr, p);
        int at = 0;
        for (int b = 0; b < (batch ? n_batches : 1); ++b) {
            const int m = batch ? batch[b] : n;
            if (m < 0 || at + m > n) throw std::invalid_argument("omni_pcm_filter_host: the batches do not fit the edges");
            lor.add(std::vector<omni_pcm_edge>(edges + at, edges + at + m));
            at += m;
        }
        for (int k = 0; k < n; ++k) good_out[k] = lor.good(edges[k]) ? 1 : 0;
        if (stats_out) for (int i = 0; i < 6; ++i) stats_out[i] = lor.stats().v[i];
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
