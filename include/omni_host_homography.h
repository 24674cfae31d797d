/* omni_host_homography.h -- C entry points of libomni_host_homography.so (omni-swarm_amd/host/host_homography_capi.cpp): where the key-frame pipeline of
 * omni_host.h runs the homography RANSAC of its loop candidates (compute_correspond_features' cv::findHomography(old_2d, new_2d, RANSAC, 3, mask),
 * loop_detector.cpp:589-598).  The handle is omni_host.h's omni_pipeline, whoever made it.  Returns as in omni_host.h: 0 on success; after a failure
 * omni_homography_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_HOMOGRAPHY_H
#define OMNI_HOST_HOMOGRAPHY_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_homography_last_error(void);

/* on != 0: on the GPU, in the round trip that matches the candidates' direction pairs (the same arithmetic, bit for bit: csrc/ransac_plan.h); a pair the device
 * hands back (degenerate points) still runs on the host.  on == 0: on the host's geometry threads.  Only a pipeline made with geometry != 0 verifies loops at
 * all; elsewhere the call succeeds and changes nothing.  Allowed between any two calls on the pipeline: the next micro-batch's candidates follow it. */
int omni_pipeline_set_device_homography(omni_pipeline* h, int on);
/* *on: the switch as set; *pairs_device: direction pairs whose mask came from the GPU so far; *pairs_host: pairs that ran on the host although the switch was
 * on (handed back by the device).  Any of the three may be NULL. */
int omni_pipeline_get_device_homography(omni_pipeline* h, int* on, int* pairs_device, int* pairs_host);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_HOMOGRAPHY_H */
