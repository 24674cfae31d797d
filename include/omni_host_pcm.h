/* omni_host_pcm.h -- C entry points of libomni_host_pcm.so (omni-swarm_amd/host/host_pcm_capi.cpp): pairwise-consistency outlier rejection of the pipeline's loop
 * edges (KeyframePipeline::Config::pcm; host/loop_outlier_rejection.hpp; SwarmLocalOutlierRejection::OutlierRejectionLoopEdges, swarm_localization/src/
 * swarm_outlier_rejection/swarm_outlier_rejection.cpp:98-298).  Every edge that enters omni_pipeline_get_edges or omni_pipeline_get_remote_edges is compared with every
 * earlier edge of its drone pair on the GPU (csrc/pcm.hip), the clique heuristic picks the pair's inlier set on the host, and omni_pipeline_good_edges lists what is
 * left.  The stage only adds an output: with it on, edges, candidates, counters and rows are what they are with it off.  Parity with the reference is UNPINNED
 * (swarm_msgs is not vendored): csrc/pcm_plan.h is the specification.  The LOOP_INLIERS message is not sent.  Returns as in omni_host.h: 0 on success; after a
 * failure omni_pcm_host_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_PCM_H
#define OMNI_HOST_PCM_H
#include <stdint.h>

#include "omni_hip.h"
#include "omni_host_wire_messages.h"      /* omni_remote_edge: every field of an edge */
#ifdef __cplusplus
extern "C" {
#endif

const char* omni_pcm_host_last_error(void);

/* Off by default.  pcm_thres > 0 (the reference's default: 0.6); redundant: every drone pair is evaluated, not only those with this drone at one end; capacity: edges
 * per drone pair, a multiple of 64 in 64..32768.  Refused: after the first key frame; on a sharded database; on a pipeline without a geometry stage. */
int omni_pipeline_set_pcm(omni_pipeline* h, int on, double pcm_thres, int redundant, int capacity);
int omni_pipeline_get_pcm(omni_pipeline* h, int* on, double* pcm_thres, int* redundant, int* capacity);
/* the pipeline's own edges, then the edges other drones sent, without those the stage rejected: up to max_edges of them to out (may be NULL with max_edges 0),
 * *n_edges receives how many there are.  An edge one of whose frames the pipeline never saw is outside the graph and passes.  With the stage off: every edge. */
int omni_pipeline_good_edges(omni_pipeline* h, omni_remote_edge* out, int max_edges, int* n_edges);
/* [0] edges entered, [1] pairs of edges evaluated, [2] consistent pairs, [3] clique runs, [4] edges left out because one of their frames was never seen, [5] edges
 * that met a full handle */
int omni_pipeline_pcm_stats(omni_pipeline* h, int64_t out[6]);
/* the records the stage entered so far, in the order they entered (path lengths included): what a recomputation on the host takes */
int omni_pipeline_pcm_records(omni_pipeline* h, omni_pcm_edge* out, int max_edges, int* n_edges);
/* LoopOutlierRejection with its rows from omni_pcm_rows_host (no GPU, no pipeline): the n edges enter in calls of batch[0], batch[1], .. edges (n_batches calls;
 * batch == NULL: one call); good_out [n]: whether edge k passes afterwards; stats_out (may be NULL) as above. */
int omni_pcm_filter_host(const omni_pcm_edge* edges, int n, const int* batch, int n_batches, int self_id, int redundant, int capacity, const omni_pcm_params* params,
                         uint8_t* good_out, int64_t stats_out[6]);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_PCM_H */
