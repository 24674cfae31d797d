/* omni_host_posegraph.h -- C entry points of libomni_host_posegraph.so (omni-swarm_amd/host/host_posegraph_capi.cpp): the 4-DoF pose graph of the key-frame
 * pipeline's window (KeyframePipeline::Config::pose_graph; host/pose_graph.hpp builds the problem, csrc/pgo.hip solves it; the loop + ego-motion part of
 * swarm_localization_solver.cpp:1064-1213, :1668-1712).  omni_pipeline_optimize solves the last `window` key frames per drone with the edges
 * omni_pipeline_good_edges returns; the stage only adds outputs: with it on, hits, candidates, edges, counters, rows and good edges are what they are with it off.
 * Parity with the reference is UNPINNED (Ceres, Eigen and swarm_msgs are not vendored): csrc/pgo_plan.h is the specification.  Returns as in omni_host.h: 0 on
 * success; after a failure omni_posegraph_host_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_POSEGRAPH_H
#define OMNI_HOST_POSEGRAPH_H
#include <stdint.h>

#include "omni_hip.h"
#include "omni_host_wire_messages.h"      /* omni_remote_edge: every field of an edge */
#ifdef __cplusplus
extern "C" {
#endif

/* a window key frame: its pose of the problem, its odometry pose, its initial value (start 0) and its estimate, each x y z yaw */
typedef struct omni_pose_graph_frame {
    int32_t drone, pose_index;
    int64_t keyframe_id;
    double  odom[4], init[4], pose[4];
} omni_pose_graph_frame;
/* a key frame as the pipeline saw it: pose = xyz + quaternion wxyz */
typedef struct omni_pose_graph_keyframe {
    int32_t drone, reserved;
    int64_t keyframe_id;
    double  pose[7];
} omni_pose_graph_keyframe;

const char* omni_posegraph_host_last_error(void);

/* Off by default.  window: key frames per drone, 2..256 (the reference's max_keyframe_num: 50); starts: initial pose sets, 1..64.  Refused: after the first key
 * frame; on a sharded database; on a pipeline without a geometry stage. */
int omni_pipeline_set_pose_graph(omni_pipeline* h, int on, int window, int starts);
int omni_pipeline_get_pose_graph(omni_pipeline* h, int* on, int* window, int* starts);
/* Solves the current window on the GPU (blocking, on a context of its own).  *status (may be NULL): OMNI_PGO_* of the start that was kept. */
int omni_pipeline_optimize(omni_pipeline* h, int* status);
/* every window key frame of the last optimize, drones ascending, oldest first: up to max_frames of them to out (may be NULL with max_frames 0), *n_frames receives
 * how many there are */
int omni_pipeline_estimated_poses(omni_pipeline* h, omni_pose_graph_frame* out, int max_frames, int* n_frames);
/* this drone's newest estimated pose . inverse(its odometry pose), x y z yaw; *valid = 0 when the last optimize held no key frame of this drone */
int omni_pipeline_pose_graph_drift(omni_pipeline* h, double out[4], int* valid);
/* of the last optimize: [0] optimize calls so far, [1] poses, [2] ego-motion edges, [3] loop edges, [4] loop edges outside the window, [5] drones no edge reaches,
 * [6] key frames merged into their predecessor's pose, [7] the start kept (-1: none ended finite), [8] its status, [9] its outer iterations, [10] its
 * conjugate-gradient steps; cost (may be NULL): its initial and final cost */
int omni_pipeline_pose_graph_stats(omni_pipeline* h, int64_t out[11], double cost[2]);
/* The exact problem the last optimize solved.  sizes[3] = {n_poses, n_edges, n_starts} is always written; poses [n_starts][n_poses][4], fixed [n_poses], edges
 * [n_edges] and *params are written where the pointer is not NULL and the capacity given (max_poses, max_edges: what ONE start and the edge array hold) suffices. */
int omni_pipeline_pose_graph_problem(omni_pipeline* h, int sizes[3], double* poses, uint8_t* fixed, int max_poses, omni_pgo_edge* edges, int max_edges,
                                     omni_pgo_params* params);
/* SwarmPoseGraph without a pipeline and without a GPU: the key frames in the order they were seen, the loop edges in order.  frames_out (up to max_frames; pose =
 * init), the problem as above, counts[5] = {ego-motion edges, loop edges, loop edges outside, unreachable drones, merged key frames}; *n_frames always written. */
int omni_pose_graph_build_host(int self_id, int window, int starts, double pos_covariance_per_meter, double yaw_covariance_per_meter,
                               const omni_pose_graph_keyframe* keyframes, int n_keyframes, const omni_remote_edge* loops, int n_loops, omni_pose_graph_frame* frames_out,
                               int max_frames, int* n_frames, int sizes[3], double* poses, uint8_t* fixed, int max_poses, omni_pgo_edge* edges, int max_edges, int counts[5]);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_POSEGRAPH_H */
