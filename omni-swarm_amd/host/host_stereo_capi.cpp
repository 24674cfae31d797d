// host_stereo_capi.cpp -> lib/libomni_host_stereo.so: the C entry points of CameraConfig::STEREO_PINHOLE over omni::KeyframePipeline (keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_stereo.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* omni_stereo_last_error(void) { return g_err.c_str(); }

omni_pipeline* omni_pipeline_create_stereo_pinhole(int device, const char* sp_weights, const char* pca_comp_csv, const char* pca_mean_csv, const char* vlad_weights,
                                                   int width, int height, float thres, int max_num, int precision, int microbatch, int pipelines, int storage,
                                                   int self_id, double inner_product_thres, double init_mode_product_thres, int match_index_dist, int min_loop_num,
                                                   int min_direction_loop, int geometry, double fx, double fy, double cx, double cy, int src_width, int src_height,
                                                   double triangle_thres, int accept_min_3d_pts) {
    try {
        omni::KeyframePipeline::Config c;
        c.device = device; c.sp_weights = sp_weights; c.pca_comp = pca_comp_csv ? pca_comp_csv : ""; c.pca_mean = pca_mean_csv ? pca_mean_csv : "";
        c.vlad_weights = vlad_weights; c.width = width; c.height = height; c.thres = thres; c.max_num = max_num; c.precision = precision;
        c.microbatch = microbatch; c.pipelines = pipelines; c.storage = storage; c.self_id = self_id;
        c.inner_product_thres = inner_product_thres; c.init_mode_product_thres = init_mode_product_thres; c.match_index_dist = match_index_dist;
        c.min_loop_num = min_loop_num; c.min_direction_loop = min_direction_loop; c.geometry = geometry != 0;
        c.camera_configuration = 0; c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.src_width = src_width; c.src_height = src_height;
        c.triangle_thres = triangle_thres; c.accept_min_3d_pts = accept_min_3d_pts;
        return new omni_pipeline{new omni::KeyframePipeline(c)};
    } catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

int omni_pipeline_set_stereo_extrinsics(omni_pipeline* h, const double* left7, const double* right7) {
    try {
        if (!h) throw std::invalid_argument("omni_pipeline_set_stereo_extrinsics: null pipeline");
        h->p->set_stereo_extrinsics(left7, right7);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
