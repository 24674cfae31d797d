// omni_depth_landmarks_*: the depth landmarks of generate_gray_depth_image_descriptor (swarm_loop/src/loop_cam.cpp:260-304, the lifted key points of :558-566)
// on the GPU, f64.  The arithmetic is depth_plan.h's -- this file only spreads it over lanes:
//   one workgroup per image, 256 lanes; pose_cam = pose_drone * extrinsic once per workgroup (every lane computes the same few dozen operations: no LDS hand-over);
//   lanes stride over the max_num key-point slots: every slot of norm2d / landmarks_3d / landmarks_flag is written exactly once, by one lane -- the lift
//            (camera_plan.h's lens model: a constant number of undistortion rounds), the gate, one u16 read of the depth image, the transform;
//   count    count_3d = the landmarks set: a ballot + popcount per wave, the waves' sums through 4 words of LDS, one lane stores it.
// No atomics.  Built with contraction off (Makefile; the headers' pragma says the same): products and sums round one by one, as the host's.
#include "common.h"
#include "depth_plan.h"

namespace omni {

#define DP_THREADS 256

__global__ __launch_bounds__(DP_THREADS) void depth_landmarks_kernel(omni_depth_model m, omni_camera_model cm, const double* __restrict__ poses7, int n_images, int max_num,
                                                                     const float* __restrict__ kps_xy, const int* __restrict__ n_kps, const uint16_t* __restrict__ depth,
                                                                     int stride, const uint8_t* __restrict__ have, float* __restrict__ norm2d, float* __restrict__ l3d,
                                                                     uint8_t* __restrict__ flag, int* __restrict__ count) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_images) return;
    __shared__ int wave_sum[DP_THREADS / 64];
    const size_t at = (size_t)i * max_num;
    const int n_raw = n_kps[i], n = lm::clamp_count(n_raw, max_num);
    const bool live = dp::image_live(m, max_num, n_raw, !have || have[i]);
    dp::ImageGeom g;
    dp::image_geom(poses7 + 7 * (size_t)i, m.extrinsic, g);
    const uint16_t* dimg = depth + (size_t)i * stride * m.depth_height;
    int kept = 0;                                             // of this lane's WAVE (every lane of a wave holds the same number)
    for (int base = 0; base < max_num; base += DP_THREADS) {  // (uniform trip count: every lane of a wave reaches the ballot)
        const int k = base + lane;
        int set = 0;
        if (k < max_num) set = dp::slot(m, cm, g, live, n, kps_xy + at * 2, dimg, stride, k, norm2d + at * 2, l3d + at * 3, flag + at);
        kept += __popcll(__ballot(set));
    }
    if ((lane & 63) == 0) wave_sum[lane >> 6] = kept;
    __syncthreads();
    if (lane == 0) {
        int c = 0;
        for (int w = 0; w < DP_THREADS / 64; ++w) c += wave_sum[w];
        count[i] = c;
    }
}

int depth_landmarks_launch(hipStream_t stream, const omni_depth_model& m, const omni_camera_model& cm, const double* poses7_dev, int n_images, int max_num, const float* kps_xy,
                           const int* n_kps, const uint16_t* depth, int stride, const uint8_t* have, float* norm2d, float* l3d, uint8_t* flag, int* count) {
    hipLaunchKernelGGL(depth_landmarks_kernel, dim3(n_images), dim3(DP_THREADS), 0, stream, m, cm, poses7_dev, n_images, max_num, kps_xy, n_kps, depth, stride, have, norm2d, l3d,
                       flag, count);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

// depth_plan.h's dp::check_model as an error code (one wording for the device entry, the host entry and the unit)
int depth_check_model(const omni_depth_model* m) {
    const char* why = dp::check_model(*m);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "%s (fx %g fy %g, %d x %d, near %g far %g)", why, m->fx, m->fy, m->depth_width, m->depth_height, m->depth_near, m->depth_far);
    return OMNI_OK;
}

}  // namespace omni

extern "C" int omni_depth_landmarks_enqueue_dev(omni_ctx* ctx, const omni_depth_model* model, const omni_camera_model* camera, const double* poses7_dev, int n_images, int max_num,
                                                const float* kps_xy_dev, const int* n_kps_dev, const uint16_t* depth_dev, int depth_stride_elems, const uint8_t* have_dev,
                                                float* norm2d_out, float* l3d_out, uint8_t* flag_out, int* count_out) {
    OMNI_REQUIRE(ctx && model && poses7_dev && kps_xy_dev && n_kps_dev && depth_dev && norm2d_out && l3d_out && flag_out && count_out, OMNI_ERR_INVALID, "null argument");
    int rc;
    if ((rc = omni::depth_check_model(model))) return rc;
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    const char* why = omni::dp::check_sizes(*model, n_images, max_num, depth_stride_elems);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "%s (n_images %d, max_num %d, stride %d, depth_width %d)", why, n_images, max_num, depth_stride_elems, model->depth_width);
    omni::TraceRange trace_range("depth landmarks (lift + depth read)");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    return omni::depth_landmarks_launch(ctx->stream, *model, cm, poses7_dev, n_images, max_num, kps_xy_dev, n_kps_dev, depth_dev, depth_stride_elems, have_dev, norm2d_out, l3d_out,
                                        flag_out, count_out);
}
