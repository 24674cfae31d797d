/* omni_host_wire.h -- C entry points of libomni_host_wire.so (omni-swarm_amd/host/host_wire_capi.cpp): the LoopNet wire of the key-frame pipeline of omni_host.h
 * (swarm_loop/src/loop_net.cpp; host/loop_net_wire.hpp), in both directions.  Out: every finished local key frame leaves as LoopNet's packets -- one VIOKF_HEADER
 * packet per image with key points and one VIOKF_LANDMARKS packet per sent landmark -- kept in order until omni_pipeline_take_packets hands them out.  In: packets of
 * other drones enter through omni_pipeline_recv_packet / omni_pipeline_scan_recv; every frame the wire completes goes through the pipeline's serial flow (flush, then
 * the detector's on_image_recv and the geometry stage), its candidate into omni_pipeline_get_candidates and an accepted loop into omni_pipeline_get_edges.  The
 * encoding is this library's own (two builds of it interoperate); byte-level interoperation with a reference drone needs the un-vendored .lcm definitions and is
 * UNPINNED.  The handle is omni_host.h's omni_pipeline, whoever made it.  Returns as in omni_host.h: 0 on success; after a failure omni_wire_host_last_error() holds
 * the message (per calling thread). */
#ifndef OMNI_HOST_WIRE_H
#define OMNI_HOST_WIRE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_wire_host_last_error(void);

#define OMNI_WIRE_CHANNEL_HEADER 0        /* "VIOKF_HEADER" */
#define OMNI_WIRE_CHANNEL_LANDMARKS 1     /* "VIOKF_LANDMARKS" */
/* (channels 2 and 3, SWARM_LOOP_IMG_DES and SWARM_LOOP_CONN, are off by default and belong to omni_host_wire_messages.h) */

/* wire != 0: the pipeline owns a LoopNetWire and keeps every finished key frame's packets.  device_wire != 0: the packets are packed inside the key-frame unit on the
 * GPU (csrc/wire_pack.hip) and only copied and numbered on the calling thread; 0: LoopNetWire::broadcast_fisheye_desc runs there.  The same bytes either way.
 * send_all_features: LoopNet's SEND_ALL_FEATURES.  All off by default.  Refused: after the first key frame; on a sharded database, which builds no messages;
 * device_wire without wire; device_wire without the landmarks being made on the device (device_landmarks for the stereo configurations, device_depth_landmarks
 * for PINHOLE_DEPTH, the geometry stage on). */
int omni_pipeline_set_wire(omni_pipeline* h, int wire, int device_wire, int send_all_features);
int omni_pipeline_get_wire(omni_pipeline* h, int* wire, int* device_wire, int* send_all_features);
/* key frames whose packets are waiting to be taken; -1 for a null pipeline */
int64_t omni_pipeline_wire_pending(omni_pipeline* h);
/* The oldest key frame's packets.  *n_bytes and *n_packets always receive what it holds.  With bytes == NULL nothing else happens (the size query).  Otherwise the
 * block goes to bytes (bytes_cap >= *n_bytes) and packet k's offset in it, size and channel (OMNI_WIRE_CHANNEL_*) to offsets[k], sizes[k], channels[k]
 * (max_packets >= *n_packets), *msg_id receives the key frame's id, and the key frame is popped.  Fails when nothing is pending or a buffer is too small (nothing
 * is popped then).  Between two calls of run / push_keyframe / poll / flush only. */
int omni_pipeline_take_packets(omni_pipeline* h, int64_t* msg_id, uint8_t* bytes, int64_t bytes_cap, int64_t* n_bytes, int64_t* offsets, int* sizes, int* channels,
                               int max_packets, int* n_packets);
/* the receiving side: recv_period (seconds; loop_net.h:33, default 0.5), MIN_DIRECTION_LOOP (default: the pipeline's min_direction_loop), group_by_frame_id (0, the
 * default: the reference's key, every image opens a frame of its own; 1: the directions of a key frame meet again) */
int omni_pipeline_set_wire_recv(omni_pipeline* h, double recv_period, int min_direction_loop, int group_by_frame_id);
/* one packet of the transport, `channel` its LCM channel name, `now` the receiver's clock in seconds; *accepted (may be NULL): 0 when the packet does not parse or
 * has another shape.  The pipeline's own packets are ignored.  Frames the packet completes go through the detector before the call returns.  Between two calls of
 * run / push_keyframe / poll / flush only. */
int omni_pipeline_recv_packet(omni_pipeline* h, const char* channel, const uint8_t* data, int64_t n, double now, int* accepted);
/* LoopNet::scan_recv_packets: images and frames whose time has run out are completed; call it periodically */
int omni_pipeline_scan_recv(omni_pipeline* h, double now);
/* frames the wire has completed and handed to the detector so far; -1 for a null pipeline */
int64_t omni_pipeline_remote_frames(omni_pipeline* h);
/* the calling thread's milliseconds spent on the outgoing wire inside the pipeline so far (reset != 0: and start again) */
int omni_pipeline_wire_host_ms(omni_pipeline* h, double* ms, int reset);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_WIRE_H */
