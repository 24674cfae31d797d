// host_remote_capi.cpp -> lib/libomni_host_remote.so: the C entry points of KeyframePipeline::Config::remote_in_stream (keyframe_pipeline.hpp, remote_queue.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_remote.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
omni::KeyframePipeline& pipe(omni_pipeline* h, const char* who) {
    if (!h) throw std::invalid_argument(std::string(who) + ": null pipeline");
    return *h->p;
}
}  // namespace

extern "C" {

const char* omni_remote_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_remote_in_stream(omni_pipeline* h, int on) {
    try { pipe(h, "omni_pipeline_set_remote_in_stream").set_remote_in_stream(on != 0); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_remote_in_stream(omni_pipeline* h, int* on) {
    try {
        if (!on) throw std::invalid_argument("omni_pipeline_get_remote_in_stream: null argument");
        *on = pipe(h, "omni_pipeline_get_remote_in_stream").remote_in_stream() ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int64_t omni_pipeline_remote_pending(omni_pipeline* h) { return h ? h->p->remote_pending() : -1; }

int omni_pipeline_remote_stats(omni_pipeline* h, int64_t out[4]) {
    try {
        if (!out) throw std::invalid_argument("omni_pipeline_remote_stats: null argument");
        pipe(h, "omni_pipeline_remote_stats").remote_stats(out);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_queue_copy_as_remote(omni_pipeline* h, int64_t src_msg_id, int drone_id, int64_t new_msg_id) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_queue_copy_as_remote");
        const auto& db = p.detector().fisheyeframe_database;
        const auto it = db.find(src_msg_id);
        if (it == db.end()) throw std::out_of_range("omni_pipeline_queue_copy_as_remote: key frame " + std::to_string(src_msg_id) + " is not in the database");
        if (db.find(new_msg_id) != db.end()) throw std::invalid_argument("omni_pipeline_queue_copy_as_remote: key frame " + std::to_string(new_msg_id) + " is in the database already");
        omni::FisheyeFrameDescriptor f = it->second;
        f.drone_id = drone_id; f.msg_id = new_msg_id; f.prevent_adding_db = false;
        for (auto& im : f.images) { im.drone_id = drone_id; im.frame_id = new_msg_id; }
        p.queue_remote_frame(std::move(f));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_remote_merge_plan(int64_t a, int64_t b, const int64_t* queue_p, int64_t n_queue, int32_t* remote_out, int64_t* index_out, int64_t cap, int64_t* n_out,
                           int64_t* n_taken) {
    try {
        if (!n_out || !n_taken) throw std::invalid_argument("omni_remote_merge_plan: null argument");
        int64_t taken = 0;
        const std::vector<omni::RemoteMergeSlot> plan = omni::remote_merge_plan(a, b, queue_p, n_queue, &taken);
        *n_out = (int64_t)plan.size(); *n_taken = taken;
        if ((int64_t)plan.size() > cap || (!plan.empty() && (!remote_out || !index_out))) throw std::length_error("omni_remote_merge_plan: " + std::to_string(plan.size()) + " slots do not fit");
        for (size_t s = 0; s < plan.size(); ++s) { remote_out[s] = plan[s].remote ? 1 : 0; index_out[s] = plan[s].index; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
