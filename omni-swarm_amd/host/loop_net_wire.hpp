// loop_net_wire.hpp -- the wire side of LoopNet (swarm_loop/src/loop_net.cpp), transport-agnostic: how one key frame leaves a drone as
// packets and how packets from other drones become FisheyeFrameDescriptor messages for LoopDetector::on_image_recv.
//
//   LoopNetWire::broadcast_fisheye_desc / broadcast_img_desc   loop_net.cpp:19-120   one "VIOKF_HEADER" packet per image + one "VIOKF_LANDMARKS"
//                                                                                    packet per landmark with a 3-D point (or all, SEND_ALL_FEATURES)
//   LoopNetWire::on_packet -> header / landmark reassembly     loop_net.cpp:187-229, 300-324
//   LoopNetWire::scan_recv_packets                             loop_net.cpp:231-298  image complete or recv_period elapsed -> image; >= MIN_DIRECTION_LOOP
//                                                                                    images or 2 x recv_period elapsed -> frame_desc_callback
//   LoopNetWire::image_desc_callback                           loop_net.cpp:143-174  frames keyed by the image's msg_id (sic), null images for the
//                                                                                    directions not (yet) received (generate_null_img_desc)
//
// The reference publishes LCM messages generated from swarm_msgs' .lcm files, which are un-vendored: the exact field order and the 8-byte LCM
// type fingerprints cannot be reproduced here.  The encoding below follows LCM's rules (fingerprint first, big-endian scalars, every
// variable-length array preceded by its own length member) over the fields loop_net.cpp reads and writes, with fingerprints of our own:
// two builds of THIS library interoperate; byte-level interop with a reference drone needs the .lcm definitions.
// Pinned: tests/cpp/wire_pin.cpp compiles the reference's own LoopNet (class + loop_net.cpp, extracted at build time) against stand-in ROS /
// LCM / swarm_msgs types and runs it next to this class: same messages out of broadcast_fisheye_desc, same frames out of frame_desc_callback
// under complete, lossy and shuffled delivery.
// Deviations (both asserted by that test): message ids come from a per-object counter mixed with the drone id instead of rand() + nsec
// (loop_net.cpp:28,81): deterministic; a header always activates its image, also when a landmark packet overtook it (see on_header).
//
// The other two message kinds of loop_net.cpp:9-10, under the same rules and with the same caveat (fingerprints of our own, "OMNIIMG1" and "OMNILCN1": byte-level
// interoperation with a reference drone is UNPINNED, the .lcm files are not vendored):
//   SWARM_LOOP_IMG_DES   the whole ImageDescriptor_t: behind an image's landmark packets under send_img (without the 64-d descriptors) or send_whole_img_desc
//                        (with them), alone and whole under is_pc_replay (loop_net.cpp:37-41, 103-116).  ALL landmark_num landmarks, as the reference sends them.
//                        A fixed head with every scalar and every length member, then the float arrays, then the two byte arrays (csrc/wire_plan.h restates it for
//                        the GPU, which stores whole dwords).
//   SWARM_LOOP_CONN      every accepted LoopEdge (loop_net.cpp:122-127, 174-184), a packet of fixed size; doubles travel as their 64 bits.
// One more deviation: the reference hands every received SWARM_LOOP_IMG_DES to image_desc_callback (:129-140), so the receiver of a send_img drone gets each
// image twice, the second time without descriptors.  Here a received whole-descriptor packet always reaches image_callback; it enters the frame flow only with
// accept_img_desc set (what a replay ground station sets) AND when it carries its descriptors.
#pragma once
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <set>

#include "loop_geometry.hpp"
#include "omni_swarm.hpp"

namespace omni {
namespace wire {

struct Writer {
    std::vector<uint8_t> b;
    void u8(uint8_t v) { b.push_back(v); }
    void i32(int32_t v) { for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)((uint32_t)v >> s)); }
    void i64(int64_t v) { for (int s = 56; s >= 0; s -= 8) b.push_back((uint8_t)((uint64_t)v >> s)); }
    void f32(float v) { uint32_t u; std::memcpy(&u, &v, 4); i32((int32_t)u); }
    void f64(double v) { uint64_t u; std::memcpy(&u, &v, 8); i64((int64_t)u); }
    void pose(const PoseMsg& p) { for (double v : p.position) f64(v); for (double v : p.quat_wxyz) f64(v); }
};
struct Reader {
    const uint8_t* p; size_t n, o = 0; bool ok = true;
    Reader(const uint8_t* data, size_t len) : p(data), n(len) {}
    bool need(size_t k) { if (o + k > n) { ok = false; return false; } return true; }
    uint8_t u8() { return need(1) ? p[o++] : 0; }
    int32_t i32() { if (!need(4)) return 0; uint32_t v = 0; for (int i = 0; i < 4; ++i) v = (v << 8) | p[o++]; return (int32_t)v; }
    int64_t i64() { if (!need(8)) return 0; uint64_t v = 0; for (int i = 0; i < 8; ++i) v = (v << 8) | p[o++]; return (int64_t)v; }
    float f32() { uint32_t u = (uint32_t)i32(); float v; std::memcpy(&v, &u, 4); return v; }
    double f64() { uint64_t u = (uint64_t)i64(); double v; std::memcpy(&v, &u, 8); return v; }
    PoseMsg pose() { PoseMsg m; for (double& v : m.position) v = f64(); for (double& v : m.quat_wxyz) v = f64(); return m; }
};

constexpr int64_t FP_HEADER = 0x4f4d4e4948445231ll;      // "OMNIHDR1"
constexpr int64_t FP_LANDMARK = 0x4f4d4e494c4d4b31ll;    // "OMNILMK1"
constexpr const char* CH_HEADER = "VIOKF_HEADER";        // loop_net.cpp:12
constexpr const char* CH_LANDMARKS = "VIOKF_LANDMARKS";  // loop_net.cpp:13

struct ImageDescriptorHeader {                           // ImageDescriptorHeader_t as loop_net.cpp:51-63 fills it
    double timestamp = 0; int drone_id = 0, feature_num = 0, direction = 0; bool prevent_adding_db = false;
    int64_t msg_id = 0, frame_id = 0;
    std::vector<float> image_desc; PoseMsg pose_drone, camera_extrinsic;
};
struct LandmarkDescriptor {                              // LandmarkDescriptor_t as loop_net.cpp:70-85 fills it
    int landmark_id = 0, drone_id = 0, landmark_flag = 0;
    Point2f landmark_2d_norm{0, 0}, landmark_2d{0, 0}; Point3f landmark_3d;
    std::vector<float> feature_descriptor; int64_t msg_id = 0, header_id = 0;
};

inline std::vector<uint8_t> encode(const ImageDescriptorHeader& h) {
    Writer w;
    w.i64(FP_HEADER); w.f64(h.timestamp); w.i32(h.drone_id); w.i64(h.msg_id); w.i64(h.frame_id); w.i32(h.feature_num); w.i32(h.direction);
    w.u8(h.prevent_adding_db ? 1 : 0); w.pose(h.pose_drone); w.pose(h.camera_extrinsic);
    w.i32((int32_t)h.image_desc.size());
    for (float v : h.image_desc) w.f32(v);
    return std::move(w.b);
}
inline bool decode(const uint8_t* p, size_t n, ImageDescriptorHeader& h) {
    Reader r(p, n);
    if (r.i64() != FP_HEADER) return false;
    h.timestamp = r.f64(); h.drone_id = r.i32(); h.msg_id = r.i64(); h.frame_id = r.i64(); h.feature_num = r.i32(); h.direction = r.i32();
    h.prevent_adding_db = r.u8() != 0; h.pose_drone = r.pose(); h.camera_extrinsic = r.pose();
    const int32_t k = r.i32();
    if (!r.ok || k < 0 || (size_t)k * 4 > n) return false;
    h.image_desc.resize(k);
    for (auto& v : h.image_desc) v = r.f32();
    return r.ok && r.o == n;
}
inline std::vector<uint8_t> encode(const LandmarkDescriptor& l) {
    Writer w;
    w.i64(FP_LANDMARK); w.i64(l.msg_id); w.i64(l.header_id); w.i32(l.drone_id); w.i32(l.landmark_id); w.i32(l.landmark_flag);
    w.f32(l.landmark_2d_norm.x); w.f32(l.landmark_2d_norm.y); w.f32(l.landmark_2d.x); w.f32(l.landmark_2d.y);
    w.f32(l.landmark_3d.x); w.f32(l.landmark_3d.y); w.f32(l.landmark_3d.z);
    w.i32((int32_t)l.feature_descriptor.size());
    for (float v : l.feature_descriptor) w.f32(v);
    return std::move(w.b);
}
inline bool decode(const uint8_t* p, size_t n, LandmarkDescriptor& l) {
    Reader r(p, n);
    if (r.i64() != FP_LANDMARK) return false;
    l.msg_id = r.i64(); l.header_id = r.i64(); l.drone_id = r.i32(); l.landmark_id = r.i32(); l.landmark_flag = r.i32();
    l.landmark_2d_norm.x = r.f32(); l.landmark_2d_norm.y = r.f32(); l.landmark_2d.x = r.f32(); l.landmark_2d.y = r.f32();
    l.landmark_3d.x = r.f32(); l.landmark_3d.y = r.f32(); l.landmark_3d.z = r.f32();
    const int32_t k = r.i32();
    if (!r.ok || k < 0 || (size_t)k * 4 > n) return false;
    l.feature_descriptor.resize(k);
    for (auto& v : l.feature_descriptor) v = r.f32();
    return r.ok && r.o == n;
}

constexpr int64_t FP_IMAGE = 0x4f4d4e49494d4731ll;       // "OMNIIMG1"
constexpr int64_t FP_LOOP_CONN = 0x4f4d4e494c434e31ll;   // "OMNILCN1"
constexpr const char* CH_IMG_DES = "SWARM_LOOP_IMG_DES"; // loop_net.cpp:9
constexpr const char* CH_LOOP_CONN = "SWARM_LOOP_CONN";  // loop_net.cpp:10
constexpr size_t IMAGE_HEAD_BYTES = 177;                 // the whole descriptor's fixed head: every scalar and every length member
constexpr size_t LOOP_CONN_BYTES = 276;                  // 8 + 3 x 8 + 3 x 4 + 2 x 8 + 3 x 56 + 6 x 8

// The whole ImageDescriptor.  Head: fingerprint, timestamp, drone_id, msg_id, frame_id, landmark_num, direction, prevent_adding_db, pose_drone, camera_extrinsic,
// image_width, image_height, image_desc_size, feature_descriptor_size, image_size; then image_desc, feature_descriptor, landmarks_2d_norm, landmarks_2d,
// landmarks_3d (the three of landmark_num entries each); then landmarks_flag and image.  with_features false: feature_descriptor_size 0 (loop_net.cpp:105-107).
// An array shorter than landmark_num announces is completed with zeros (as broadcast_img_desc reads flags and 3-D points).
inline std::vector<uint8_t> encode(const ImageDescriptor& m, bool with_features) {
    Writer w;
    const int n = m.landmark_num < 0 ? 0 : m.landmark_num;
    const size_t fds = with_features ? (size_t)n * 64 : 0;
    w.i64(FP_IMAGE); w.f64(m.timestamp); w.i32(m.drone_id); w.i64(m.msg_id); w.i64(m.frame_id); w.i32(n); w.i32(m.direction);
    w.u8(m.prevent_adding_db ? 1 : 0); w.pose(m.pose_drone); w.pose(m.camera_extrinsic);
    w.i32(m.image_width); w.i32(m.image_height); w.i32((int32_t)m.image_desc.size()); w.i32((int32_t)fds); w.i32((int32_t)m.image.size());
    for (float v : m.image_desc) w.f32(v);
    for (size_t i = 0; i < fds; ++i) w.f32(i < m.feature_descriptor.size() ? m.feature_descriptor[i] : 0.f);
    for (int i = 0; i < n; ++i) { const Point2f p = i < (int)m.landmarks_2d_norm.size() ? m.landmarks_2d_norm[i] : Point2f{0, 0}; w.f32(p.x); w.f32(p.y); }
    for (int i = 0; i < n; ++i) { const Point2f p = i < (int)m.landmarks_2d.size() ? m.landmarks_2d[i] : Point2f{0, 0}; w.f32(p.x); w.f32(p.y); }
    for (int i = 0; i < n; ++i) { const Point3f p = i < (int)m.landmarks_3d.size() ? m.landmarks_3d[i] : Point3f{}; w.f32(p.x); w.f32(p.y); w.f32(p.z); }
    for (int i = 0; i < n; ++i) w.u8(i < (int)m.landmarks_flag.size() ? m.landmarks_flag[i] : 0);
    w.b.insert(w.b.end(), m.image.begin(), m.image.end());
    return std::move(w.b);
}
// The four length members must account for the packet's size exactly; that is checked before anything is resized.
inline bool decode(const uint8_t* p, size_t n, ImageDescriptor& m) {
    Reader r(p, n);
    if (r.i64() != FP_IMAGE) return false;
    m.timestamp = r.f64(); m.drone_id = r.i32(); m.msg_id = r.i64(); m.frame_id = r.i64(); m.landmark_num = r.i32(); m.direction = r.i32();
    m.prevent_adding_db = r.u8() != 0; m.pose_drone = r.pose(); m.camera_extrinsic = r.pose();
    m.image_width = r.i32(); m.image_height = r.i32();
    const int32_t ids = r.i32(), fds = r.i32(), isz = r.i32(), k = m.landmark_num;
    if (!r.ok || k < 0 || ids < 0 || fds < 0 || isz < 0) return false;
    if ((uint64_t)IMAGE_HEAD_BYTES + 4ull * ((uint64_t)ids + (uint64_t)fds + 7ull * (uint64_t)k) + (uint64_t)k + (uint64_t)isz != (uint64_t)n) return false;
    m.image_desc.resize(ids); m.feature_descriptor.resize(fds); m.landmarks_2d_norm.resize(k); m.landmarks_2d.resize(k); m.landmarks_3d.resize(k);
    for (auto& v : m.image_desc) v = r.f32();
    for (auto& v : m.feature_descriptor) v = r.f32();
    for (auto& v : m.landmarks_2d_norm) { v.x = r.f32(); v.y = r.f32(); }
    for (auto& v : m.landmarks_2d) { v.x = r.f32(); v.y = r.f32(); }
    for (auto& v : m.landmarks_3d) { v.x = r.f32(); v.y = r.f32(); v.z = r.f32(); }
    if (!r.need((size_t)k + (size_t)isz)) return false;
    m.landmarks_flag.assign(p + r.o, p + r.o + k); r.o += k;
    m.image.assign(p + r.o, p + r.o + isz); r.o += isz;
    return r.ok && r.o == n;
}

inline void put_pose(Writer& w, const geom::Pose& q) { w.f64(q.pos.x); w.f64(q.pos.y); w.f64(q.pos.z); w.f64(q.att.w); w.f64(q.att.x); w.f64(q.att.y); w.f64(q.att.z); }
inline void get_pose(Reader& r, geom::Pose& q) { q.pos.x = r.f64(); q.pos.y = r.f64(); q.pos.z = r.f64(); q.att.w = r.f64(); q.att.x = r.f64(); q.att.y = r.f64(); q.att.z = r.f64(); }
// every field of omni::LoopEdge (loop_geometry.hpp), LOOP_CONN_BYTES in all
inline std::vector<uint8_t> encode(const LoopEdge& e) {
    Writer w;
    w.i64(FP_LOOP_CONN); w.i64(e.id); w.i64(e.keyframe_id_a); w.i64(e.keyframe_id_b); w.i32(e.drone_id_a); w.i32(e.drone_id_b); w.i32(e.pnp_inlier_num);
    w.f64(e.ts_a); w.f64(e.ts_b); put_pose(w, e.relative_pose); put_pose(w, e.self_pose_a); put_pose(w, e.self_pose_b);
    for (double v : e.pos_cov) w.f64(v);
    for (double v : e.ang_cov) w.f64(v);
    return std::move(w.b);
}
inline bool decode(const uint8_t* p, size_t n, LoopEdge& e) {
    if (n != LOOP_CONN_BYTES) return false;
    Reader r(p, n);
    if (r.i64() != FP_LOOP_CONN) return false;
    e.id = r.i64(); e.keyframe_id_a = r.i64(); e.keyframe_id_b = r.i64(); e.drone_id_a = r.i32(); e.drone_id_b = r.i32(); e.pnp_inlier_num = r.i32();
    e.ts_a = r.f64(); e.ts_b = r.f64(); get_pose(r, e.relative_pose); get_pose(r, e.self_pose_a); get_pose(r, e.self_pose_b);
    for (double& v : e.pos_cov) v = r.f64();
    for (double& v : e.ang_cov) v = r.f64();
    return r.ok && r.o == n;
}

}  // namespace wire

class LoopNetWire {
public:
    static constexpr int FEATURE_DESC_SIZE = 64;         // loop_defines.h:67
    static constexpr size_t IMAGE_DESC_SIZE = 4096;      // MobileNetVLAD's output (loop_defines.h)
    static constexpr int MAX_FEATURES = 4096;            // sanity bound on a header's feature_num (the reference sends <= 200)
    static constexpr int MAX_IMAGE_BYTES = 1 << 22;      // sanity bound on a whole descriptor's image_size (a q 75 JPEG of a 640 x 480 view is ~60 kB)
    double orphan_timeout = 10.0;                        // landmarks whose header never arrives are forgotten after this many seconds
    double recv_period = 0.5;                            // loop_net.h:33
    int MIN_DIRECTION_LOOP = 3;
    bool SEND_ALL_FEATURES = false;
    // false = the reference's key (frame_hash = image.msg_id, loop_net.cpp:144: every image opens a frame of its own, so a received fisheye
    // frame never holds more than one direction); true = key by (drone, frame_id) so that the 4 directions of a key frame meet again
    bool group_by_frame_id = false;
    // LoopNet(_lcm_uri, send_img, send_whole_img_desc, recv_msg_duration) and IS_PC_REPLAY (loop_net.h, loop_net.cpp:37,103): which images also leave as a whole
    // descriptor.  accept_img_desc: received whole descriptors that carry their 64-d descriptors enter the frame flow (see the deviation above); off by default
    bool send_img = false, send_whole_img_desc = false, is_pc_replay = false, accept_img_desc = false;
    // transport: publish(channel, bytes) is called for every outgoing packet; feed incoming packets to on_packet()
    std::function<void(const char* channel, const std::vector<uint8_t>& bytes)> publish;
    std::function<void(const FisheyeFrameDescriptor&)> frame_desc_callback;      // -> LoopDetector::on_image_recv
    std::function<void(int drone_id, float rate)> msg_recv_rate_callback = [](int, float) {};
    std::function<void(const LoopEdge&)> loopconn_callback;                      // every received edge that is not our own (loop_net.cpp:174-184)
    std::function<void(const ImageDescriptor&)> image_callback;                  // every received whole descriptor that is not our own (:129-140)
    explicit LoopNetWire(int self_id) : self_id_(self_id) {}

    // :19-26
    void broadcast_fisheye_desc(FisheyeFrameDescriptor& f) { for (auto& img : f.images) if (img.landmark_num > 0) broadcast_img_desc(img); }

    // :28-118: the replay early return, the header + landmark packets, then the whole descriptor behind them under send_img / send_whole_img_desc
    int broadcast_img_desc(ImageDescriptor& img) {
        img.msg_id = next_id();
        sent_message.insert(img.msg_id);
        if (is_pc_replay) { const auto b = wire::encode(img, true); publish(wire::CH_IMG_DES, b); return (int)b.size(); }      // :37-41
        int feature_num = 0;
        for (int i = 0; i < img.landmark_num; ++i) if (i < (int)img.landmarks_flag.size() && img.landmarks_flag[i] > 0) ++feature_num;
        wire::ImageDescriptorHeader h;
        h.timestamp = img.timestamp; h.drone_id = img.drone_id; h.image_desc = img.image_desc; h.pose_drone = img.pose_drone;
        h.camera_extrinsic = img.camera_extrinsic; h.prevent_adding_db = img.prevent_adding_db; h.msg_id = img.msg_id; h.frame_id = img.frame_id;
        // the landmarks WITH a 3-D point, also under SEND_ALL_FEATURES (loop_net.cpp:62): the receiver then closes the image after that many
        // packets and drops the rest -- the reference's behaviour, kept so that its drones and ours read each other's headers the same way
        h.feature_num = feature_num; h.direction = img.direction;
        size_t bytes = 0;
        { auto b = wire::encode(h); bytes += b.size(); publish(wire::CH_HEADER, b); }
        for (int i = 0; i < img.landmark_num; ++i) {
            const int flag = i < (int)img.landmarks_flag.size() ? img.landmarks_flag[i] : 0;
            if (!(flag > 0 || SEND_ALL_FEATURES)) continue;
            wire::LandmarkDescriptor lm;
            lm.landmark_id = i; lm.landmark_2d_norm = img.landmarks_2d_norm[i]; lm.landmark_2d = img.landmarks_2d[i];
            lm.landmark_3d = i < (int)img.landmarks_3d.size() ? img.landmarks_3d[i] : Point3f{}; lm.landmark_flag = flag; lm.drone_id = img.drone_id;
            lm.feature_descriptor.assign(img.feature_descriptor.begin() + (size_t)i * FEATURE_DESC_SIZE, img.feature_descriptor.begin() + (size_t)(i + 1) * FEATURE_DESC_SIZE);
            lm.msg_id = next_id(); lm.header_id = img.msg_id;
            auto b = wire::encode(lm); bytes += b.size(); publish(wire::CH_LANDMARKS, b);
        }
        if (send_img || send_whole_img_desc) { const auto b = wire::encode(img, send_whole_img_desc); bytes += b.size(); publish(wire::CH_IMG_DES, b); }   // :103-116
        return (int)bytes;
    }

    // :122-127
    void broadcast_loop_connection(const LoopEdge& e) { sent_message.insert(e.id); publish(wire::CH_LOOP_CONN, wire::encode(e)); }

    // lcm.subscribe handlers (:9-13): returns false for packets that do not parse
    // Array lengths come from the network: a landmark must carry exactly FEATURE_DESC_SIZE floats and a header a 4096-float global descriptor
    // (or none) -- LoopDetector reads that many from image_desc / feature_descriptor without looking at the vector's size -- and the direction
    // must index the 4 images of a frame.  Packets of any other shape (another version, corruption that kept the framing) are dropped.
    bool on_packet(const char* channel, const uint8_t* data, size_t n, double now) {
        if (std::strcmp(channel, wire::CH_HEADER) == 0) {
            wire::ImageDescriptorHeader h;
            if (!wire::decode(data, n, h)) return false;
            if (!(h.image_desc.size() == IMAGE_DESC_SIZE || h.image_desc.empty()) || h.feature_num < 0 || h.feature_num > MAX_FEATURES || h.direction < 0 || h.direction >= 4) return false;
            on_header(h, now);
            return true;
        }
        if (std::strcmp(channel, wire::CH_LANDMARKS) == 0) {
            wire::LandmarkDescriptor l;
            if (!wire::decode(data, n, l)) return false;
            if (l.feature_descriptor.size() != (size_t)FEATURE_DESC_SIZE) return false;
            on_landmark(l, now);
            return true;
        }
        // the whole descriptor: LoopDetector reads 4096 / 64 floats per image / landmark here too, so the two float arrays are of those sizes or absent
        if (std::strcmp(channel, wire::CH_IMG_DES) == 0) {
            ImageDescriptor m;
            if (!wire::decode(data, n, m)) return false;
            if (!(m.image_desc.size() == IMAGE_DESC_SIZE || m.image_desc.empty()) || m.landmark_num > MAX_FEATURES || m.direction < 0 || m.direction >= 4 ||
                !(m.feature_descriptor.empty() || m.feature_descriptor.size() == (size_t)FEATURE_DESC_SIZE * m.landmark_num) || m.image.size() > (size_t)MAX_IMAGE_BYTES)
                return false;
            on_whole_image(m, now);
            return true;
        }
        if (std::strcmp(channel, wire::CH_LOOP_CONN) == 0) {
            LoopEdge e;
            if (!wire::decode(data, n, e)) return false;
            if (!sent_message.count(e.id) && loopconn_callback) loopconn_callback(e);                 // :178-183
            return true;
        }
        return false;
    }

    // :231-298; call it periodically too (the reference runs it from every landmark packet, :323)
    void scan_recv_packets(double tnow) {
        std::vector<int64_t> finish_recv;
        for (int64_t id : active_receving_msg) {
            ImageDescriptor& im = received_images[id];
            if (tnow - msg_header_recv_time[id] > recv_period || im.landmark_num == (int)im.landmarks_2d.size()) {
                const float rate = im.landmark_num > 0 ? (float)im.landmarks_2d.size() / (float)im.landmark_num : 1.f;
                im.landmark_num = (int)im.landmarks_2d.size();
                finish_recv.push_back(id);
                msg_recv_rate_callback(im.drone_id, rate);
            }
        }
        for (int64_t id : finish_recv) { blacklist.insert(id); active_receving_msg.erase(id); }
        for (int64_t id : finish_recv) {
            ImageDescriptor& im = received_images[id];
            im.landmark_num = (int)im.landmarks_2d.size();
            if (!im.landmarks_2d.empty()) image_desc_callback(im);
            received_images.erase(id);
            msg_header_recv_time.erase(id);
            orphan_first_seen.erase(id);
        }
        // entries created by landmarks whose header never came (lost, rejected, or sent by somebody else's bug) must not pile up
        for (auto it = orphan_first_seen.begin(); it != orphan_first_seen.end();) {
            if (msg_header_recv_time.count(it->first)) { it = orphan_first_seen.erase(it); continue; }      // the header arrived meanwhile
            if (tnow - it->second > orphan_timeout) { received_images.erase(it->first); blacklist.insert(it->first); it = orphan_first_seen.erase(it); continue; }
            ++it;
        }
        std::vector<int64_t> finish_frames;
        for (int64_t hash : active_receving_frames) {
            int count = 0;
            for (auto& im : received_frames[hash].images) if (im.landmark_num > 0) ++count;
            if (tnow - frame_header_recv_time[hash] > 2.0 * recv_period || count >= MIN_DIRECTION_LOOP) finish_frames.push_back(hash);
        }
        for (int64_t hash : finish_frames) {
            FisheyeFrameDescriptor& f = received_frames[hash];
            active_receving_frames.erase(hash);
            f.landmark_num = 0;
            for (auto& im : f.images) f.landmark_num += im.landmark_num;
            if (frame_desc_callback) frame_desc_callback(f);
            received_frames.erase(hash);
            frame_header_recv_time.erase(hash);
        }
    }

    // ids for packets that were encoded elsewhere (the key-frame unit's pack stage, csrc/wire_plan.h, leaves them zero): the next id of this object's sequence,
    // a header's entered into sent_message as broadcast_img_desc does
    int64_t reserve_id(bool header) { const int64_t id = next_id(); if (header) sent_message.insert(id); return id; }
    bool msg_blocked(int64_t id) const { return blacklist.count(id) || sent_message.count(id); }     // loop_net.h:85-87
    int pending_images() const { return (int)received_images.size(); }

private:
    // :187-229
    void on_header(const wire::ImageDescriptorHeader& m, double now) {
        if (msg_blocked(m.msg_id)) return;
        msg_header_recv_time[m.msg_id] = now;
        // the reference marks the image active only when the header CREATES the entry (:197-201): a landmark packet that overtakes its header
        // (on_landmark creates the entry, :308-311) leaves the image inactive for ever.  Fixed here: the header always activates it.
        active_receving_msg.insert(m.msg_id);
        ImageDescriptor& t = received_images[m.msg_id];
        t.timestamp = m.timestamp; t.drone_id = m.drone_id; t.image_desc = m.image_desc; t.pose_drone = m.pose_drone; t.camera_extrinsic = m.camera_extrinsic;
        t.landmark_num = m.feature_num; t.frame_id = m.frame_id; t.msg_id = m.msg_id; t.prevent_adding_db = m.prevent_adding_db; t.direction = m.direction;
    }
    // :129-140, with the deviation stated at the top.  A whole descriptor that enters the frame flow supersedes what the header + landmark packets of the same
    // image have assembled so far, and an image those packets already delivered is not delivered again (its id is black-listed).
    void on_whole_image(const ImageDescriptor& m, double now) {
        if (sent_message.count(m.msg_id)) return;
        if (image_callback) image_callback(m);
        if (!accept_img_desc || m.landmark_num <= 0 || m.feature_descriptor.empty() || blacklist.count(m.msg_id)) return;
        active_receving_msg.erase(m.msg_id); received_images.erase(m.msg_id); orphan_first_seen.erase(m.msg_id);
        blacklist.insert(m.msg_id);
        msg_header_recv_time[m.msg_id] = now;
        image_desc_callback(m);
        msg_header_recv_time.erase(m.msg_id);
        scan_recv_packets(now);
    }
    // :300-324
    void on_landmark(const wire::LandmarkDescriptor& m, double now) {
        if (msg_blocked(m.header_id)) return;
        if (!received_images.count(m.header_id)) orphan_first_seen.emplace(m.header_id, now);
        ImageDescriptor& t = received_images[m.header_id];          // a landmark may overtake its header: the entry is created here (:308-311)
        t.landmarks_2d_norm.push_back(m.landmark_2d_norm); t.landmarks_2d.push_back(m.landmark_2d); t.landmarks_3d.push_back(m.landmark_3d);
        t.landmarks_flag.push_back((uint8_t)m.landmark_flag);
        t.feature_descriptor.insert(t.feature_descriptor.end(), m.feature_descriptor.begin(), m.feature_descriptor.begin() + FEATURE_DESC_SIZE);
        scan_recv_packets(now);
    }
    // :143-174
    void image_desc_callback(const ImageDescriptor& image) {
        const int64_t frame_hash = group_by_frame_id ? (((int64_t)image.drone_id << 48) ^ image.frame_id) : image.msg_id;      // (sic) see group_by_frame_id
        auto it = received_frames.find(frame_hash);
        if (it == received_frames.end()) {
            FisheyeFrameDescriptor f;
            f.image_num = 4; f.timestamp = image.timestamp;
            for (int i = 0; i < f.image_num; ++i) {
                if (i != image.direction) { ImageDescriptor null_img; null_img.landmark_num = 0; f.images.push_back(null_img); }   // generate_null_img_desc
                else f.images.push_back(image);
            }
            f.msg_id = image.frame_id; f.pose_drone = image.pose_drone; f.landmark_num = 0; f.drone_id = image.drone_id;
            received_frames[frame_hash] = f;
            frame_header_recv_time[frame_hash] = msg_header_recv_time[image.msg_id];
            active_receving_frames.insert(frame_hash);
        } else if (image.direction >= 0 && image.direction < (int)it->second.images.size()) {
            it->second.images[image.direction] = image;
        }
    }
    int64_t next_id() { return ((int64_t)self_id_ << 40) | (++counter_); }

    int self_id_;
    int64_t counter_ = 0;
    std::set<int64_t> sent_message, blacklist, active_receving_msg, active_receving_frames;
    std::map<int64_t, ImageDescriptor> received_images;
    std::map<int64_t, FisheyeFrameDescriptor> received_frames;
    std::map<int64_t, double> msg_header_recv_time, frame_header_recv_time, orphan_first_seen;
};

}  // namespace omni
