// host_wire_capi.cpp -> lib/libomni_host_wire.so: the C entry points of the pipeline's LoopNet wire (KeyframePipeline::Config::wire / device_wire, keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <cstring>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_wire.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
omni::KeyframePipeline& pipe(omni_pipeline* h, const char* who) {
    if (!h) throw std::invalid_argument(std::string(who) + ": null pipeline");
    return *h->p;
}
}  // namespace

extern "C" {

const char* omni_wire_host_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_wire(omni_pipeline* h, int wire, int device_wire, int send_all_features) {
    try { pipe(h, "omni_pipeline_set_wire").set_wire(wire != 0, device_wire != 0, send_all_features != 0); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_wire(omni_pipeline* h, int* wire, int* device_wire, int* send_all_features) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_get_wire");
        if (wire) *wire = p.wire();
        if (device_wire) *device_wire = p.device_wire();
        if (send_all_features) *send_all_features = p.send_all_features();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int64_t omni_pipeline_wire_pending(omni_pipeline* h) { return h ? (int64_t)h->p->wire_pending() : -1; }

int omni_pipeline_take_packets(omni_pipeline* h, int64_t* msg_id, uint8_t* bytes, int64_t bytes_cap, int64_t* n_bytes, int64_t* offsets, int* sizes, int* channels,
                               int max_packets, int* n_packets) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_take_packets");
        if (!n_bytes || !n_packets) throw std::invalid_argument("omni_pipeline_take_packets: null argument");
        const omni::KeyframePipeline::SentFrame* s = p.oldest_packets();
        if (!s) throw std::runtime_error("omni_pipeline_take_packets: no key frame's packets are pending");
        *n_bytes = (int64_t)s->bytes.size(); *n_packets = (int)s->size.size();
        if (!bytes) return 0;
        if (!msg_id || !offsets || !sizes || !channels) throw std::invalid_argument("omni_pipeline_take_packets: null argument");
        if (bytes_cap < *n_bytes || max_packets < *n_packets)
            throw std::length_error("omni_pipeline_take_packets: " + std::to_string(*n_packets) + " packets of " + std::to_string(*n_bytes) + " bytes do not fit the buffers");
        const omni::KeyframePipeline::SentFrame f = p.take_packets();
        *msg_id = f.msg_id;
        if (!f.bytes.empty()) std::memcpy(bytes, f.bytes.data(), f.bytes.size());
        for (size_t k = 0; k < f.size.size(); ++k) { offsets[k] = f.off[k]; sizes[k] = f.size[k]; channels[k] = f.channel[k]; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_set_wire_recv(omni_pipeline* h, double recv_period, int min_direction_loop, int group_by_frame_id) {
    try { pipe(h, "omni_pipeline_set_wire_recv").set_wire_recv(recv_period, min_direction_loop, group_by_frame_id != 0); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_recv_packet(omni_pipeline* h, const char* channel, const uint8_t* data, int64_t n, double now, int* accepted) {
    try {
        if (n < 0) throw std::invalid_argument("omni_pipeline_recv_packet: a negative size");
        const bool ok = pipe(h, "omni_pipeline_recv_packet").recv_packet(channel, data, (size_t)n, now);
        if (accepted) *accepted = ok;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_scan_recv(omni_pipeline* h, double now) {
    try { pipe(h, "omni_pipeline_scan_recv").scan_recv(now); return 0; } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int64_t omni_pipeline_remote_frames(omni_pipeline* h) { return h ? h->p->remote_frames() : -1; }

int omni_pipeline_wire_host_ms(omni_pipeline* h, double* ms, int reset) {
    try {
        if (!ms) throw std::invalid_argument("omni_pipeline_wire_host_ms: null argument");
        *ms = pipe(h, "omni_pipeline_wire_host_ms").wire_host_ms(reset != 0);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
