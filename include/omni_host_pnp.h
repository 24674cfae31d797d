/* omni_host_pnp.h -- C entry points of libomni_host_pnp.so (omni-swarm_amd/host/host_pnp_capi.cpp): where the key-frame pipeline of omni_host.h runs the RANSAC
 * half of its loop candidates' relative pose (compute_relative_pose's cv::solvePnPRansac, loop_detector.cpp:390-391).  The handle is omni_host.h's
 * omni_pipeline, whoever made it.  Returns as in omni_host.h: 0 on success; after a failure omni_pnp_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_PNP_H
#define OMNI_HOST_PNP_H
#ifdef __cplusplus
extern "C" {
#endif

#include <stdint.h>

typedef struct omni_pipeline omni_pipeline;

const char* omni_pnp_last_error(void);

/* on != 0: every candidate's EPnP RANSAC on the GPU, one call from its geometry task (the same arithmetic, bit for bit: csrc/pnp_plan.h); the refit stays on the
 * host, and a candidate the device hands back still runs there whole.  on == 0 (the default): on the host's geometry threads.  Only a pipeline made with
 * geometry != 0 verifies loops at all; elsewhere the call succeeds and changes nothing.  Allowed between any two calls on the pipeline: the next micro-batch's
 * candidates follow it. */
int omni_pipeline_set_device_pnp(omni_pipeline* h, int on);
/* *on: the switch as set; *candidates_device: candidates whose RANSAC ran on the GPU so far; *candidates_host: candidates that ran on the host although the
 * switch was on (handed back by the device, or more points than it takes).  Any of the three may be NULL. */
int omni_pipeline_get_device_pnp(omni_pipeline* h, int* on, int* candidates_device, int* candidates_host);


/* The path of a key frame that ANOTHER drone sent (KeyframePipeline::on_remote_frame: verified on the spot, in init_mode -- 1 000 PnP iterations -- while few
 * loops connect the two drones), for callers without the network layer: a copy of the database's key frame src_msg_id is handed to the detector as key frame
 * new_msg_id of drone drone_id (not this drone's id; new_msg_id not in the database yet).  After a flush(), between two calls on the pipeline.
 * *old_msg_id: the database frame it was matched with, -1 for none; *loop: 1 when the candidate became an edge.  Either may be NULL. */
int omni_pipeline_recv_copy_as_remote(omni_pipeline* h, int64_t src_msg_id, int drone_id, int64_t new_msg_id, int64_t* old_msg_id, int* loop);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_PNP_H */
