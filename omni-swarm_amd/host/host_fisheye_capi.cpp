// host_fisheye_capi.cpp -> lib/libomni_host_fisheye.so: the C entry points of the raw-fisheye mode of CameraConfig::STEREO_FISHEYE over omni::KeyframePipeline
// (keyframe_pipeline.hpp: Config::fisheye_src_width ...).  A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same
// (host_capi_types.hpp).
#include <algorithm>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_fisheye.h"     // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_fisheye_last_error(void) { return g_err.c_str(); }

omni_pipeline* omni_pipeline_create_stereo_fisheye_raw(int device, const char* sp_weights, const char* pca_comp_csv, const char* pca_mean_csv, const char* vlad_weights,
                                                       int width, int height, float thres, int max_num, int precision, int microbatch, int pipelines, int storage,
                                                       int self_id, double inner_product_thres, double init_mode_product_thres, int match_index_dist, int min_loop_num,
                                                       int min_direction_loop, int geometry, int src_width, int src_height, double fov_deg, const double* mei_up9,
                                                       const double* mei_down9, int first_view) {
    try {
        if (!sp_weights || !vlad_weights || !mei_up9 || !mei_down9) throw std::invalid_argument("omni_pipeline_create_stereo_fisheye_raw: null argument");
        if (src_width < 1 || src_height < 1) throw std::invalid_argument("omni_pipeline_create_stereo_fisheye_raw: the fisheye camera's frame size src_width x src_height is missing");
        omni::KeyframePipeline::Config c;
        c.device = device; c.sp_weights = sp_weights; c.pca_comp = pca_comp_csv ? pca_comp_csv : ""; c.pca_mean = pca_mean_csv ? pca_mean_csv : "";
        c.vlad_weights = vlad_weights; c.width = width; c.height = height; c.thres = thres; c.max_num = max_num; c.precision = precision;
        c.microbatch = microbatch; c.pipelines = pipelines; c.storage = storage; c.self_id = self_id;
        c.inner_product_thres = inner_product_thres; c.init_mode_product_thres = init_mode_product_thres; c.match_index_dist = match_index_dist;
        c.min_loop_num = min_loop_num; c.min_direction_loop = min_direction_loop; c.geometry = geometry != 0;
        c.cx = width / 2.0; c.cy = height / 2.0; c.fx = c.fy = width / 2.0;      // the side views' own pinhole model (focal length width / 2), as omni_pipeline_create
        c.camera_configuration = 1;
        c.fisheye_src_width = src_width; c.fisheye_src_height = src_height; c.fisheye_fov_deg = fov_deg; c.fisheye_first_view = first_view;
        std::copy(mei_up9, mei_up9 + 9, c.fisheye_mei_up); std::copy(mei_down9, mei_down9 + 9, c.fisheye_mei_down);
        return new omni_pipeline{new omni::KeyframePipeline(c)};
    } catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

int omni_pipeline_get_fisheye_raw(omni_pipeline* h, int* src_width, int* src_height) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_get_fisheye_raw: null pipeline");
        const bool on = h->p->fisheye_raw();
        if (src_width) *src_width = on ? h->p->in_width() : 0;
        if (src_height) *src_height = on ? h->p->in_height() : 0;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
