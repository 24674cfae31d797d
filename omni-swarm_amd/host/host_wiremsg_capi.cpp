// host_wiremsg_capi.cpp -> lib/libomni_host_wiremsg.so: the C entry points of the wire's other two message kinds (KeyframePipeline::Config::wire_img_desc /
// wire_loop_conn, keyframe_pipeline.hpp).  A library of its own next to libomni_host_wire.so, whose set of entry points is fixed; the handle is the same
// (host_capi_types.hpp).
#include <cstring>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_wire_messages.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;
omni::KeyframePipeline& pipe(omni_pipeline* h, const char* who) {
    if (!h) throw std::invalid_argument(std::string(who) + ": null pipeline");
    return *h->p;
}
void put_pose(double* out, const omni::geom::Pose& p) { out[0] = p.pos.x; out[1] = p.pos.y; out[2] = p.pos.z; out[3] = p.att.w; out[4] = p.att.x; out[5] = p.att.y; out[6] = p.att.z; }
static_assert(OMNI_WIRE_IMG_OFF == omni::KeyframePipeline::WIRE_IMG_OFF && OMNI_WIRE_IMG_IMAGE == omni::KeyframePipeline::WIRE_IMG_IMAGE &&
              OMNI_WIRE_IMG_WHOLE == omni::KeyframePipeline::WIRE_IMG_WHOLE && OMNI_WIRE_IMG_PC_REPLAY == omni::KeyframePipeline::WIRE_IMG_PC_REPLAY &&
              OMNI_WIRE_REMOTE_IMAGES_MAX == omni::KeyframePipeline::REMOTE_IMAGES_MAX, "the header's constants are the pipeline's");
}  // namespace

extern "C" {

const char* omni_wiremsg_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_wire_messages(omni_pipeline* h, int wire_img_desc, int wire_loop_conn) {
    try { pipe(h, "omni_pipeline_set_wire_messages").set_wire_messages(wire_img_desc, wire_loop_conn != 0); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_wire_messages(omni_pipeline* h, int* wire_img_desc, int* wire_loop_conn, int* accept_img_desc) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_get_wire_messages");
        if (wire_img_desc) *wire_img_desc = p.wire_img_desc();
        if (wire_loop_conn) *wire_loop_conn = p.wire_loop_conn();
        if (accept_img_desc) *accept_img_desc = p.wire_accept_img_desc();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_set_wire_accept_img_desc(omni_pipeline* h, int on) {
    try { pipe(h, "omni_pipeline_set_wire_accept_img_desc").set_wire_accept_img_desc(on != 0); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int omni_pipeline_get_remote_edges(omni_pipeline* h, omni_remote_edge* out, int max_edges, int* n_edges) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_get_remote_edges");
        if (!n_edges || max_edges < 0 || (!out && max_edges > 0)) throw std::invalid_argument("omni_pipeline_get_remote_edges: null argument or a negative count");
        const std::vector<omni::LoopEdge>& edges = p.remote_edges();
        *n_edges = (int)edges.size();
        for (int k = 0; k < max_edges && k < (int)edges.size(); ++k) {
            const omni::LoopEdge& e = edges[(size_t)k];
            omni_remote_edge& o = out[k];
            o.id = e.id; o.keyframe_id_a = e.keyframe_id_a; o.keyframe_id_b = e.keyframe_id_b; o.drone_id_a = e.drone_id_a; o.drone_id_b = e.drone_id_b;
            o.pnp_inlier_num = e.pnp_inlier_num; o.reserved = 0; o.ts_a = e.ts_a; o.ts_b = e.ts_b;
            put_pose(o.relative_pose, e.relative_pose); put_pose(o.self_pose_a, e.self_pose_a); put_pose(o.self_pose_b, e.self_pose_b);
            std::memcpy(o.pos_cov, e.pos_cov, sizeof o.pos_cov); std::memcpy(o.ang_cov, e.ang_cov, sizeof o.ang_cov);
        }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

int64_t omni_pipeline_remote_image_pending(omni_pipeline* h, int64_t* dropped) {
    if (!h) return -1;
    if (dropped) *dropped = h->p->remote_images_dropped();
    return (int64_t)h->p->remote_images_pending();
}

int omni_pipeline_take_remote_image(omni_pipeline* h, uint8_t* bytes, int64_t bytes_cap, int64_t* n_bytes, int* drone_id, int64_t* frame_id, int* direction, int* width,
                                    int* height) {
    try {
        omni::KeyframePipeline& p = pipe(h, "omni_pipeline_take_remote_image");
        if (!n_bytes) throw std::invalid_argument("omni_pipeline_take_remote_image: null argument");
        const omni::KeyframePipeline::RemoteImage* r = p.oldest_remote_image();
        if (!r) throw std::runtime_error("omni_pipeline_take_remote_image: no image is pending");
        *n_bytes = (int64_t)r->bytes.size();
        if (!bytes) return 0;
        if (!drone_id || !frame_id || !direction || !width || !height) throw std::invalid_argument("omni_pipeline_take_remote_image: null argument");
        if (bytes_cap < *n_bytes) throw std::length_error("omni_pipeline_take_remote_image: " + std::to_string(*n_bytes) + " bytes do not fit the buffer");
        const omni::KeyframePipeline::RemoteImage im = p.take_remote_image();
        std::memcpy(bytes, im.bytes.data(), im.bytes.size());
        *drone_id = im.drone_id; *frame_id = im.frame_id; *direction = im.direction; *width = im.width; *height = im.height;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
