/* omni_host_stereo.h -- C entry points of libomni_host_stereo.so (omni-swarm_amd/host/host_stereo_capi.cpp): CameraConfig::STEREO_PINHOLE (loop_defines.h:110-115,
 * swarm_loop.cpp:275-286; generate_stereo_image_descriptor for one direction, loop_cam.cpp:189-196) on the key-frame pipeline of omni_host.h.  The handle is
 * omni_host.h's omni_pipeline: everything there (run, push_keyframe, flush, get_edges, destroy ...) works on a pipeline made here.  Returns as in omni_host.h:
 * 0 on success; after a failure omni_stereo_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_STEREO_H
#define OMNI_HOST_STEREO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_stereo_last_error(void);

/* The arguments of omni_pipeline_create, then the pinhole model fx fy cx cy of the NETWORK-size (width x height) image -- key points stay in network-image
 * coordinates and are lifted as they are (loop_cam.cpp:558-569) --, the camera's frame size (src_width x src_height: frames are resized to width x height
 * inside every unit, on the GPU; 0 x 0: they arrive at the networks' size) and the stereo thresholds (loop_cam.cpp:385-444).  A key frame is a left and a
 * right frame: omni_pipeline_push_keyframe takes images[0] = left, images[1] = right at the camera's size; a block of omni_pipeline_run holds the
 * micro-batch's left frames followed by its right frames, rows packed.  MobileNetVLAD runs on the left frame only, no rows are blanked, there is one
 * direction (MAX_DIRS = 1; the query direction is 0, loop_detector.cpp:252-258).  NULL on failure. */
omni_pipeline* omni_pipeline_create_stereo_pinhole(int device, const char* sp_weights, const char* pca_comp_csv, const char* pca_mean_csv, const char* vlad_weights,
                                                   int width, int height, float thres, int max_num, int precision, int microbatch, int pipelines, int storage,
                                                   int self_id, double inner_product_thres, double init_mode_product_thres, int match_index_dist, int min_loop_num,
                                                   int min_direction_loop, int geometry, double fx, double fy, double cx, double cy, int src_width, int src_height,
                                                   double triangle_thres, int accept_min_3d_pts);

/* body -> camera of the left and the right camera (xyz + quaternion wxyz; body_T_cam0 / body_T_cam1, swarm_loop.cpp:294-306) instead of the defaults (a
 * forward-looking left camera at the body origin, the right camera 0.10 m to its right).  Refused after the first key frame, and on a pipeline of another
 * camera configuration. */
int omni_pipeline_set_stereo_extrinsics(omni_pipeline* h, const double* left7, const double* right7);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_STEREO_H */
