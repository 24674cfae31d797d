// host_landmarks_capi.cpp -> lib/libomni_host_landmarks.so: the C switch of KeyframePipeline::Config::device_landmarks (keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_landmarks.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_landmarks_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_device_landmarks(omni_pipeline* h, int on) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_device_landmarks: null pipeline");
        h->p->set_device_landmarks(on != 0);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
