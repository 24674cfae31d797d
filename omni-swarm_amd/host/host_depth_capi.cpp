// host_depth_capi.cpp -> lib/libomni_host_depth.so: the C switch of KeyframePipeline::Config::device_depth_landmarks (keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_depth.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_depth_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_device_depth_landmarks(omni_pipeline* h, int on) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_device_depth_landmarks: null pipeline");
        h->p->set_device_depth_landmarks(on != 0);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_device_depth_landmarks(omni_pipeline* h, int* on) {
    try {
        if (!h || !on) throw std::invalid_argument("omni_pipeline_get_device_depth_landmarks: null argument");
        *on = h->p->device_depth_landmarks_config() ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
