// host_jpegdec_capi.cpp -> lib/libomni_host_jpegdec.so: the C switch of KeyframePipeline::Config::compressed_images (keyframe_pipeline.hpp) and the two intakes for
// key frames that come as JPEG files.  A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same
// (host_capi_types.hpp).
#include <string>
#include <vector>

#include "host_capi_types.hpp"
#include "swarm_loop_params.hpp"
#include "omni_host_jpegdec.h"   // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_jpegdec_host_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_compressed_images(omni_pipeline* h, int on) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_compressed_images: null pipeline");
        h->p->set_compressed_images(on != 0);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_compressed_images(omni_pipeline* h, int* on, int* active) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_get_compressed_images: null pipeline");
        if (on) *on = h->p->compressed_config() ? 1 : 0;
        if (active) *active = h->p->compressed() ? 1 : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_swarm_vins_is_compressed_images(const char* vins_yaml_text, int* present) {
    omni::SwarmLoopParams p;
    const bool found = vins_yaml_text && p.read_vins_settings(vins_yaml_text);
    if (present) *present = found ? 1 : 0;
    return p.is_compressed_images ? 1 : 0;
}

int omni_pipeline_apply_vins_settings(omni_pipeline* h, const char* vins_yaml_text) {
    try {
        if (!h || !vins_yaml_text) throw std::invalid_argument("omni_pipeline_apply_vins_settings: null argument");
        omni::SwarmLoopParams p;
        p.read_vins_settings(vins_yaml_text);
        h->p->set_compressed_images(p.is_compressed_images);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_jpeg_corrupt(omni_pipeline* h, int64_t* count) {
    try {
        if (!h || !count) throw std::invalid_argument("omni_pipeline_jpeg_corrupt: null argument");
        *count = h->p->jpeg_corrupt();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_push_keyframe_jpeg(omni_pipeline* h, const uint8_t* const* files, const int64_t* sizes, int64_t msg_id, double stamp, const double* pose7,
                                     int prevent_adding_db, const uint16_t* depth, int* hits) {
    try {
        if (!h || !files || !sizes) throw std::invalid_argument("omni_pipeline_push_keyframe_jpeg: null argument");
        omni::KeyframePipeline::KeyframeIn k;
        k.images = files; k.sizes = sizes; k.msg_id = msg_id; k.stamp = stamp; k.prevent_adding_db = prevent_adding_db != 0; k.depth = depth;
        if (pose7) { for (int i = 0; i < 3; ++i) k.pose_drone.position[i] = pose7[i]; for (int i = 0; i < 4; ++i) k.pose_drone.quat_wxyz[i] = pose7[3 + i]; }
        const int n = h->p->push_keyframe(k);
        if (hits) *hits += n;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_run_jpeg(omni_pipeline* h, int n_keyframes, int64_t first_msg_id, const uint8_t* const* files, const int64_t* sizes, int* hits) {
    try {
        if (!h || !files || !sizes || n_keyframes < 0) throw std::invalid_argument("omni_pipeline_run_jpeg: null argument");
        omni::KeyframePipeline& p = *h->p;
        if (!p.compressed()) throw std::invalid_argument("omni_pipeline_run_jpeg: compressed_images is off, or ignored in this pipeline's mode");
        using JF = omni::KeyframePipeline::JpegFile;
        const int MB = p.microbatch(), cams = p.stereo_rig() ? 2 : 1, full = n_keyframes / MB, rem = n_keyframes % MB;
        // blocks as run() reads them: per micro-batch [left files | right files]
        std::vector<std::vector<JF>> blocks((size_t)full + (rem ? 1 : 0));
        for (size_t e = 0; e < blocks.size(); ++e) {
            const int cnt = (int)e < full ? MB : rem;
            blocks[e].resize((size_t)cams * cnt);
            for (int c = 0; c < cams; ++c)
                for (int i = 0; i < cnt; ++i) {
                    const size_t at = (size_t)cams * ((size_t)e * MB + i) + c;
                    blocks[e][(size_t)c * cnt + i] = JF{files[at], sizes[at]};
                }
        }
        std::vector<const uint8_t*> pool;
        for (int e = 0; e < full; ++e) pool.push_back(reinterpret_cast<const uint8_t*>(blocks[(size_t)e].data()));
        const uint8_t* tail = rem ? reinterpret_cast<const uint8_t*>(blocks.back().data()) : nullptr;
        static const uint8_t* const kNone = nullptr;
        const int n = p.run(n_keyframes, first_msg_id, pool.empty() ? &kNone : pool.data(), pool.empty() ? 1 : (int)pool.size(), 0, tail, true);
        if (hits) *hits += n;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
