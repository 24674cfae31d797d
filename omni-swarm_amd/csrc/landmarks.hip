// omni_landmarks_*: the lifting and the up/down triangulation of generate_stereo_image_descriptor (swarm_loop/src/loop_cam.cpp:397-444, triangulatePoint
// :73-106, the lifted key points of :558-566) on the GPU, f64.  The arithmetic is landmark_plan.h's -- this file only spreads it over lanes:
//   one workgroup per image pair (a direction of a key frame), 256 lanes;
//   phase 0  lanes over the key points of both images: the message's lifted floats (camera_plan.h's lens model: a constant number of undistortion rounds);
//            the pair's landmarks and flags zeroed;
//   phase 1  one match per lane: lift the two matched pixels in double (the same lens model), triangulate (4 x 4 cyclic Jacobi, A and V in registers), test, write;
//   count    count_3d = the kept matches: a ballot + popcount per wave, the waves' sums through 4 words of LDS, one lane stores it.
// The match lists are one-to-one (landmark_plan.h's precondition), so no two lanes write the same key point: no atomics.  Built with contraction off
// (Makefile; the header's pragma says the same): products and sums round one by one, as the host's.
#include "common.h"
#include "landmark_plan.h"

namespace omni {

#define LM_THREADS 256

__global__ __launch_bounds__(LM_THREADS) void landmarks_kernel(omni_stereo_model m, omni_camera_model cm, const double* __restrict__ poses7, int n_pairs, int max_num,
                                                               const float* __restrict__ kps_up, const float* __restrict__ kps_down,
                                                               const int* __restrict__ n_up_arr, const int* __restrict__ n_down_arr,
                                                               const int* __restrict__ match_up, const int* __restrict__ match_down,
                                                               const int* __restrict__ n_matches, float* __restrict__ norm_up, float* __restrict__ norm_down,
                                                               float* __restrict__ l3d_up, float* __restrict__ l3d_down, uint8_t* __restrict__ flag_up,
                                                               uint8_t* __restrict__ flag_down, int* __restrict__ count) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= n_pairs) return;
    __shared__ int wave_sum[LM_THREADS / 64];
    const size_t at = (size_t)p * max_num;
    const float *ku = kps_up + at * 2, *kd = kps_down + at * 2;
    float *l3u = l3d_up + at * 3, *l3d_ = l3d_down + at * 3;
    uint8_t *fu = flag_up + at, *fd = flag_down + at;
    const int n_up_raw = n_up_arr[p], n_down_raw = n_down_arr[p];
    lm::pair_phase0(m, cm, max_num, ku, n_up_raw, kd, n_down_raw, norm_up + at * 2, norm_down + at * 2, l3u, l3d_, fu, fd, lane, LM_THREADS);
    __syncthreads();                                          // the zeros of phase 0 are in place before any match writes over them
    const int nu = lm::clamp_count(n_up_raw, max_num), nd = lm::clamp_count(n_down_raw, max_num), nm = lm::pair_live_matches(m, max_num, n_up_raw, n_matches[p]);
    int kept = 0;                                             // of this lane's WAVE (every lane of a wave holds the same number)
    if (nm > 0) {
        const int dirs = m.dirs_per_keyframe, dir = p % dirs;
        lm::PairGeom g;
        lm::pair_geom(poses7 + 7 * (p / dirs), m.up_extrinsic[dir], m.down_extrinsic[dir], g);
        for (int base = 0; base < nm; base += LM_THREADS) {   // (uniform trip count: every lane of a wave reaches the ballot)
            const int i = base + lane;
            int keep = 0, tie = 0;
            if (i < nm) keep = lm::pair_match(m, cm, g, ku, nu, kd, nd, match_up[at + i], match_down[at + i], l3u, l3d_, fu, fd, &tie);
            kept += __popcll(__ballot(keep));
        }
    }
    if ((lane & 63) == 0) wave_sum[lane >> 6] = kept;
    __syncthreads();
    if (lane == 0) {
        int c = 0;
        for (int w = 0; w < LM_THREADS / 64; ++w) c += wave_sum[w];
        count[p] = c;
    }
}

// pair p: up image p of the *_up arrays, down image p of the *_down arrays (the unit's layout: the down images right behind the up images)
int landmarks_launch(hipStream_t stream, const omni_stereo_model& m, const omni_camera_model& cm, const double* poses7_dev, int n_pairs, int max_num, const float* kps_up, const float* kps_down,
                     const int* n_up, const int* n_down, const int* match_up, const int* match_down, const int* n_matches, float* norm_up, float* norm_down,
                     float* l3d_up, float* l3d_down, uint8_t* flag_up, uint8_t* flag_down, int* count) {
    hipLaunchKernelGGL(landmarks_kernel, dim3(n_pairs), dim3(LM_THREADS), 0, stream, m, cm, poses7_dev, n_pairs, max_num, kps_up, kps_down, n_up, n_down, match_up,
                       match_down, n_matches, norm_up, norm_down, l3d_up, l3d_down, flag_up, flag_down, count);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

int landmarks_check_model(const omni_stereo_model* m) {
    OMNI_REQUIRE(m->dirs_per_keyframe >= 1 && m->dirs_per_keyframe <= OMNI_STEREO_MAX_DIRS, OMNI_ERR_INVALID, "stereo model: %d directions per key frame, 1..%d",
                 m->dirs_per_keyframe, OMNI_STEREO_MAX_DIRS);
    OMNI_REQUIRE(m->fx != 0 && m->fy != 0 && m->fx == m->fx && m->fy == m->fy, OMNI_ERR_INVALID, "stereo model: focal lengths %g, %g", m->fx, m->fy);
    return OMNI_OK;
}

int landmarks_check_camera(const omni_camera_model* cm) {
    const char* why = cam::check(*cm);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "%s (type %d, k1 %g k2 %g p1 %g p2 %g xi %g)", why, cm->type, cm->k1, cm->k2, cm->p1, cm->p2, cm->xi);
    return OMNI_OK;
}

}  // namespace omni

extern "C" int omni_landmarks_enqueue_dev(omni_ctx* ctx, const omni_stereo_model* model, const double* poses7_dev, int n_pairs, int dirs_per_keyframe, int max_num,
                                          const float* kps_xy_dev, const int* n_kps_dev, const int* match_up_dev, const int* match_down_dev, const int* n_matches_dev,
                                          float* norm2d_out, float* l3d_out, uint8_t* flag_out, int* count_out) {
    return omni_landmarks_enqueue_dev_camera(ctx, model, nullptr, poses7_dev, n_pairs, dirs_per_keyframe, max_num, kps_xy_dev, n_kps_dev, match_up_dev, match_down_dev,
                                             n_matches_dev, norm2d_out, l3d_out, flag_out, count_out);
}

extern "C" int omni_landmarks_enqueue_dev_camera(omni_ctx* ctx, const omni_stereo_model* model, const omni_camera_model* camera, const double* poses7_dev, int n_pairs,
                                                 int dirs_per_keyframe, int max_num, const float* kps_xy_dev, const int* n_kps_dev, const int* match_up_dev,
                                                 const int* match_down_dev, const int* n_matches_dev, float* norm2d_out, float* l3d_out, uint8_t* flag_out, int* count_out) {
    OMNI_REQUIRE(ctx && model && poses7_dev && kps_xy_dev && n_kps_dev && match_up_dev && match_down_dev && n_matches_dev && norm2d_out && l3d_out && flag_out && count_out,
                 OMNI_ERR_INVALID, "null argument");
    int rc;
    if ((rc = omni::landmarks_check_model(model))) return rc;
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    OMNI_REQUIRE(dirs_per_keyframe == model->dirs_per_keyframe, OMNI_ERR_INVALID, "omni_landmarks_enqueue_dev: %d directions per key frame, the model has %d",
                 dirs_per_keyframe, model->dirs_per_keyframe);
    OMNI_REQUIRE(n_pairs >= 1 && n_pairs <= 65535 && n_pairs % dirs_per_keyframe == 0, OMNI_ERR_INVALID, "omni_landmarks_enqueue_dev: %d pairs of %d directions per key frame",
                 n_pairs, dirs_per_keyframe);
    OMNI_REQUIRE(max_num >= 1 && max_num <= 1024, OMNI_ERR_INVALID, "omni_landmarks_enqueue_dev: max_num=%d outside [1, 1024]", max_num);
    omni::TraceRange trace_range("stereo landmarks (lift + triangulate)");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    const size_t half = (size_t)n_pairs * max_num;
    return omni::landmarks_launch(ctx->stream, *model, cm, poses7_dev, n_pairs, max_num, kps_xy_dev, kps_xy_dev + half * 2, n_kps_dev, n_kps_dev + n_pairs, match_up_dev,
                                  match_down_dev, n_matches_dev, norm2d_out, norm2d_out + half * 2, l3d_out, l3d_out + half * 3, flag_out, flag_out + half, count_out);
}

// camera_plan.h on the host: no GPU, no context
extern "C" int omni_camera_lift_host(const omni_camera_model* camera, const double* intrinsics4, const float* xy, int n, double* out_xy_f64) {
    OMNI_REQUIRE(intrinsics4 && n >= 0 && (n == 0 || (xy && out_xy_f64)), OMNI_ERR_INVALID, "omni_camera_lift_host: null argument or n < 0");
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    int rc;
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    OMNI_REQUIRE(intrinsics4[0] != 0 && intrinsics4[1] != 0 && intrinsics4[0] == intrinsics4[0] && intrinsics4[1] == intrinsics4[1], OMNI_ERR_INVALID,
                 "omni_camera_lift_host: focal lengths %g, %g", intrinsics4[0], intrinsics4[1]);
    for (int i = 0; i < n; ++i) omni::cam::lift(cm, intrinsics4[0], intrinsics4[1], intrinsics4[2], intrinsics4[3], xy[2 * i], xy[2 * i + 1], out_xy_f64 + 2 * (size_t)i);
    return OMNI_OK;
}

extern "C" int omni_camera_project_host(const omni_camera_model* camera, const double* intrinsics4, const double* xyz, int n, double* out_xy_f64) {
    OMNI_REQUIRE(intrinsics4 && n >= 0 && (n == 0 || (xyz && out_xy_f64)), OMNI_ERR_INVALID, "omni_camera_project_host: null argument or n < 0");
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    int rc;
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    for (int i = 0; i < n; ++i) omni::cam::project(cm, intrinsics4[0], intrinsics4[1], intrinsics4[2], intrinsics4[3], xyz + 3 * (size_t)i, out_xy_f64 + 2 * (size_t)i);
    return OMNI_OK;
}
