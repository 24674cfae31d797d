// host_jpeg_capi.cpp -> lib/libomni_host_jpeg.so: the C switch of KeyframePipeline::Config::send_img / jpg_quality (keyframe_pipeline.hpp) and a reader of the
// images the messages then carry.  A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <cstring>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_jpeg.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_jpeg_host_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_send_img(omni_pipeline* h, int on, int quality) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_send_img: null pipeline");
        h->p->set_send_img(on != 0, quality);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_send_img(omni_pipeline* h, int* on, int* quality, int* active) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_get_send_img: null pipeline");
        if (on) *on = h->p->send_img_config() ? 1 : 0;
        if (quality) *quality = h->p->jpg_quality();
        if (active) *active = h->p->send_img() ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_jpeg_truncated(omni_pipeline* h, int64_t* count) {
    try {
        if (!h || !count) throw std::invalid_argument("omni_pipeline_jpeg_truncated: null argument");
        *count = h->p->jpeg_truncated();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_frame_image(omni_pipeline* h, int64_t msg_id, int direction, uint8_t* out, int64_t capacity, int64_t* size) {
    try {
        if (!h || !size) throw std::invalid_argument("omni_pipeline_frame_image: null argument");
        const auto& db = h->p->detector().fisheyeframe_database;
        const auto it = db.find(msg_id);
        if (it == db.end()) throw std::out_of_range("omni_pipeline_frame_image: key frame " + std::to_string(msg_id) + " is not in the database");
        if (direction < 0 || direction >= (int)it->second.images.size()) throw std::out_of_range("omni_pipeline_frame_image: no such direction");
        const std::vector<uint8_t>& im = it->second.images[(size_t)direction].image;
        *size = (int64_t)im.size();
        if (out && !im.empty() && (int64_t)im.size() <= capacity) std::memcpy(out, im.data(), im.size());
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
