// host_homography_capi.cpp -> lib/libomni_host_homography.so: the C switch of KeyframePipeline::Config::device_homography (keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_homography.h"     // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_homography_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_device_homography(omni_pipeline* h, int on) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_device_homography: null pipeline");
        h->p->set_device_homography(on != 0);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_device_homography(omni_pipeline* h, int* on, int* pairs_device, int* pairs_host) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_get_device_homography: null pipeline");
        if (on) *on = h->p->device_homography_config() ? 1 : 0;
        if (pairs_device) *pairs_device = h->p->homography_pairs_device();
        if (pairs_host) *pairs_host = h->p->homography_pairs_host();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
