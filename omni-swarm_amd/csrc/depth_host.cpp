// depth_plan.h for host callers: plain g++, no HIP header, no GPU, no context (omni_depth_landmarks_host)
#include "depth_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}

extern "C" int omni_depth_landmarks_host(const omni_depth_model* model, const omni_camera_model* camera, const double* poses7, int n_images, int max_num, const float* kps_xy,
                                         const int* n_kps, const uint16_t* depth, int depth_stride_elems, const uint8_t* have, float* norm2d_out, float* l3d_out,
                                         uint8_t* flag_out, int* count_out) {
    if (!model || !poses7 || !kps_xy || !n_kps || !depth || !norm2d_out || !l3d_out || !flag_out || !count_out) { omni::set_error("null argument"); return OMNI_ERR_INVALID; }
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    const char* why = omni::dp::check_model(*model);
    if (!why) why = omni::cam::check(cm);
    if (!why) why = omni::dp::check_sizes(*model, n_images, max_num, depth_stride_elems);
    if (why) {
        omni::set_error("%s (fx %g fy %g, %d x %d, near %g far %g; n_images %d, max_num %d, stride %d)", why, model->fx, model->fy, model->depth_width, model->depth_height,
                        model->depth_near, model->depth_far, n_images, max_num, depth_stride_elems);
        return OMNI_ERR_INVALID;
    }
    omni::dp::depth_landmarks_host(*model, cm, poses7, n_images, max_num, kps_xy, n_kps, depth, depth_stride_elems, have, norm2d_out, l3d_out, flag_out, count_out);
    return OMNI_OK;
}
