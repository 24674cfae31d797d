// host_pnp_capi.cpp -> lib/libomni_host_pnp.so: the C switch of KeyframePipeline::Config::device_pnp (keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_pnp.h"     // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_pnp_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_device_pnp(omni_pipeline* h, int on) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_device_pnp: null pipeline");
        h->p->set_device_pnp(on != 0);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_device_pnp(omni_pipeline* h, int* on, int* candidates_device, int* candidates_host) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_get_device_pnp: null pipeline");
        if (on) *on = h->p->device_pnp_config() ? 1 : 0;
        if (candidates_device) *candidates_device = h->p->pnp_candidates_device();
        if (candidates_host) *candidates_host = h->p->pnp_candidates_host();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_recv_copy_as_remote(omni_pipeline* h, int64_t src_msg_id, int drone_id, int64_t new_msg_id, int64_t* old_msg_id, int* loop) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_recv_copy_as_remote: null pipeline");
        const auto& db = h->p->detector().fisheyeframe_database;
        const auto it = db.find(src_msg_id);
        if (it == db.end()) throw std::out_of_range("omni_pipeline_recv_copy_as_remote: key frame " + std::to_string(src_msg_id) + " is not in the database");
        if (db.find(new_msg_id) != db.end()) throw std::invalid_argument("omni_pipeline_recv_copy_as_remote: key frame " + std::to_string(new_msg_id) + " is in the database already");
        omni::FisheyeFrameDescriptor f = it->second;
        f.drone_id = drone_id; f.msg_id = new_msg_id; f.prevent_adding_db = false;
        for (auto& im : f.images) { im.drone_id = drone_id; im.frame_id = new_msg_id; }
        const omni::LoopCandidate r = h->p->on_remote_frame(f);
        if (old_msg_id) *old_msg_id = r.found ? r.old_msg_id : -1;
        if (loop) *loop = r.loop ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
