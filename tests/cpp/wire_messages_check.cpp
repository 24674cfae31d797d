// Exercises the other two message kinds of host/loop_net_wire.hpp, SWARM_LOOP_CONN (LoopEdge) and SWARM_LOOP_IMG_DES (the whole ImageDescriptor): round trips,
// packets dumped as hex for an independent reader, every truncation and every inconsistent length member dropped, the replay early return, a drone ignoring its own
// packets and edges, and the accept_img_desc rule.  Prints one tagged line per check; tests/test_wire_messages_cpu.py reads them.  argv[1] = seed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../omni-swarm_amd/host/loop_net_wire.hpp"

using namespace omni;

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
static double from_bits(uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; }
static bool same(const geom::Pose& a, const geom::Pose& b) {
    return bits(a.pos.x) == bits(b.pos.x) && bits(a.pos.y) == bits(b.pos.y) && bits(a.pos.z) == bits(b.pos.z) && bits(a.att.w) == bits(b.att.w) && bits(a.att.x) == bits(b.att.x) &&
           bits(a.att.y) == bits(b.att.y) && bits(a.att.z) == bits(b.att.z);
}
static bool same(const LoopEdge& a, const LoopEdge& b) {
    bool ok = a.id == b.id && a.keyframe_id_a == b.keyframe_id_a && a.keyframe_id_b == b.keyframe_id_b && a.drone_id_a == b.drone_id_a && a.drone_id_b == b.drone_id_b &&
              a.pnp_inlier_num == b.pnp_inlier_num && bits(a.ts_a) == bits(b.ts_a) && bits(a.ts_b) == bits(b.ts_b) && same(a.relative_pose, b.relative_pose) &&
              same(a.self_pose_a, b.self_pose_a) && same(a.self_pose_b, b.self_pose_b);
    for (int k = 0; k < 3; ++k) ok = ok && bits(a.pos_cov[k]) == bits(b.pos_cov[k]) && bits(a.ang_cov[k]) == bits(b.ang_cov[k]);
    return ok;
}
static bool same(const PoseMsg& a, const PoseMsg& b) { return std::memcmp(a.position, b.position, 24) == 0 && std::memcmp(a.quat_wxyz, b.quat_wxyz, 32) == 0; }
template <class T> static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
static bool same(const ImageDescriptor& a, const ImageDescriptor& b, bool with_features) {
    return a.drone_id == b.drone_id && a.landmark_num == b.landmark_num && a.direction == b.direction && a.msg_id == b.msg_id && a.frame_id == b.frame_id &&
           bits(a.timestamp) == bits(b.timestamp) && a.prevent_adding_db == b.prevent_adding_db && same_bytes(a.image_desc, b.image_desc) &&
           (with_features ? same_bytes(a.feature_descriptor, b.feature_descriptor) : b.feature_descriptor.empty()) && same_bytes(a.landmarks_2d, b.landmarks_2d) &&
           same_bytes(a.landmarks_2d_norm, b.landmarks_2d_norm) && same_bytes(a.landmarks_3d, b.landmarks_3d) && same_bytes(a.landmarks_flag, b.landmarks_flag) &&
           same(a.pose_drone, b.pose_drone) && same(a.camera_extrinsic, b.camera_extrinsic) && a.image_width == b.image_width && a.image_height == b.image_height &&
           same_bytes(a.image, b.image);
}
static void hex(const char* tag, const std::vector<uint8_t>& b) { std::printf("%s ", tag); for (uint8_t v : b) std::printf("%02x", v); std::printf("\n"); }
static void put32(std::vector<uint8_t>& b, size_t at, int32_t v) { for (int j = 0; j < 4; ++j) b[at + j] = (uint8_t)((uint32_t)v >> (24 - 8 * j)); }

static std::mt19937 rng;
static LoopEdge random_edge(int64_t id, bool odd) {
    std::uniform_real_distribution<double> D(-10., 10.);
    LoopEdge e;
    e.id = id; e.keyframe_id_a = ((int64_t)rng() << 24) ^ rng(); e.keyframe_id_b = -(int64_t)rng(); e.drone_id_a = 1 + rng() % 5; e.drone_id_b = -(int)(rng() % 5);
    e.pnp_inlier_num = rng() % 200; e.ts_a = 1.6e9 + D(rng); e.ts_b = 1.6e9 + D(rng);
    for (geom::Pose* p : {&e.relative_pose, &e.self_pose_a, &e.self_pose_b}) { p->pos = {D(rng), D(rng), D(rng)}; p->att = {D(rng), D(rng), D(rng), D(rng)}; }
    for (int k = 0; k < 3; ++k) { e.pos_cov[k] = D(rng); e.ang_cov[k] = D(rng); }
    if (odd) { e.ts_a = from_bits(0x7ff8000000abcdefull); e.relative_pose.att.z = from_bits(0x8000000000000000ull); e.pos_cov[1] = from_bits(0x7ff0000000000000ull); e.ang_cov[2] = from_bits(1); }
    return e;
}
// direction d of a key frame of drone 2: n landmarks, landmark i at pixel (10 i + d, 3 i), flag i % 3, an image of `img` bytes
static ImageDescriptor make_image(int d, int n, size_t img, bool odd = false) {
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    ImageDescriptor im;
    im.drone_id = 2; im.direction = d; im.frame_id = 4242; im.timestamp = 12.5 + d; im.landmark_num = n; im.prevent_adding_db = d == 1; im.image_width = 640 + d; im.image_height = 480;
    im.pose_drone.position[0] = 1.5; im.pose_drone.quat_wxyz[0] = 0.8; im.pose_drone.quat_wxyz[3] = 0.6; im.camera_extrinsic.position[2] = 0.05 * d;
    im.image_desc.resize(4096);
    for (auto& v : im.image_desc) v = U(rng);
    for (int i = 0; i < n; ++i) {
        im.landmarks_2d.push_back({(float)(10 * i + d), (float)(3 * i)}); im.landmarks_2d_norm.push_back({U(rng), U(rng)});
        im.landmarks_flag.push_back((uint8_t)(i % 3)); im.landmarks_3d.push_back(i % 3 ? Point3f{U(rng), U(rng), 5 + U(rng)} : Point3f{});
        for (int k = 0; k < 64; ++k) im.feature_descriptor.push_back(U(rng));
    }
    for (size_t k = 0; k < img; ++k) im.image.push_back((uint8_t)(1 + rng() % 255));
    if (odd && n > 0) {
        const uint32_t o[4] = {0x7fc12345u, 0xff800000u, 0x80000000u, 0x00000001u};
        std::memcpy(&im.feature_descriptor[3], &o[0], 4); std::memcpy(&im.image_desc[7], &o[1], 4); std::memcpy(&im.landmarks_3d[0].z, &o[2], 4); std::memcpy(&im.landmarks_2d_norm[0].x, &o[3], 4);
        im.timestamp = from_bits(0x7ff8000000abcdefull);
    }
    return im;
}
struct Pkt { std::string ch; std::vector<uint8_t> b; };

int main(int argc, char** argv) {
    rng.seed(argc > 1 ? std::atoi(argv[1]) : 1);
    {   // ---- edges: round trip by bits, the one size, the independent reader's input
        int ok = 0, wrong_size = 0;
        for (int k = 0; k < 20; ++k) {
            const LoopEdge e = random_edge(100 + k, k % 4 == 0);
            const auto b = wire::encode(e);
            LoopEdge d;
            ok += b.size() == wire::LOOP_CONN_BYTES && wire::decode(b.data(), b.size(), d) && same(e, d) && wire::encode(d) == b;
            auto longer = b; longer.push_back(0);
            wrong_size += wire::decode(longer.data(), longer.size(), d) ? 1 : 0;
            for (size_t n = 0; n < b.size(); ++n) wrong_size += wire::decode(b.data(), n, d) ? 1 : 0;
        }
        std::printf("EDGE_ROUNDTRIP %d %d\n", ok, wrong_size);
        const LoopEdge e = random_edge(77, true);
        hex("EDGE_HEX", wire::encode(e));
        std::printf("EDGE_FIELDS %lld %lld %lld %d %d %d", (long long)e.id, (long long)e.keyframe_id_a, (long long)e.keyframe_id_b, e.drone_id_a, e.drone_id_b, e.pnp_inlier_num);
        const double dbl[29] = {e.ts_a, e.ts_b, e.relative_pose.pos.x, e.relative_pose.pos.y, e.relative_pose.pos.z, e.relative_pose.att.w, e.relative_pose.att.x, e.relative_pose.att.y,
                                e.relative_pose.att.z, e.self_pose_a.pos.x, e.self_pose_a.pos.y, e.self_pose_a.pos.z, e.self_pose_a.att.w, e.self_pose_a.att.x, e.self_pose_a.att.y,
                                e.self_pose_a.att.z, e.self_pose_b.pos.x, e.self_pose_b.pos.y, e.self_pose_b.pos.z, e.self_pose_b.att.w, e.self_pose_b.att.x, e.self_pose_b.att.y,
                                e.self_pose_b.att.z, e.pos_cov[0], e.pos_cov[1], e.pos_cov[2], e.ang_cov[0], e.ang_cov[1], e.ang_cov[2]};
        for (double v : dbl) std::printf(" %016llx", (unsigned long long)bits(v));
        std::printf("\n");
    }
    {   // ---- whole descriptors: round trip in every mode; the independent reader's input
        int ok = 0, total = 0;
        for (int n : {1, 2, 3, 4, 40, 200})
            for (size_t img : {(size_t)0, (size_t)1, (size_t)331, (size_t)4096})
                for (bool feat : {false, true}) {
                    ImageDescriptor im = make_image(n % 4, n, img, n == 40); im.msg_id = ((int64_t)2 << 40) | n;
                    const auto b = wire::encode(im, feat);
                    ImageDescriptor d;
                    ++total;
                    ok += b.size() == wire::IMAGE_HEAD_BYTES + 4 * (4096 + (feat ? 64 * n : 0) + 7 * (size_t)n) + n + img && wire::decode(b.data(), b.size(), d) && same(im, d, feat) &&
                          wire::encode(d, feat) == b;
                }
        std::printf("IMAGE_ROUNDTRIP %d %d\n", ok, total);
        ImageDescriptor im = make_image(3, 5, 7, true); im.msg_id = 987654321012ll;
        hex("IMAGE_HEX_FEATURES", wire::encode(im, true));
        hex("IMAGE_HEX_BARE", wire::encode(im, false));
    }
    // ---- a key frame through LoopNetWire in each mode
    FisheyeFrameDescriptor f;
    f.msg_id = 4242; f.drone_id = 2; f.timestamp = 12.5;
    const int n_lm[4] = {40, 25, 0, 60};
    int flagged = 0, all = 0;
    for (int d = 0; d < 4; ++d) { f.images.push_back(make_image(d, n_lm[d], 300 + d)); all += n_lm[d]; for (int i = 0; i < n_lm[d]; ++i) flagged += (i % 3) != 0; }
    auto send = [&](bool send_img, bool whole, bool replay, std::vector<Pkt>& out, LoopNetWire& tx) {
        tx.send_img = send_img; tx.send_whole_img_desc = whole; tx.is_pc_replay = replay;
        tx.publish = [&out](const char* ch, const std::vector<uint8_t>& b) { out.push_back({ch, b}); };
        FisheyeFrameDescriptor copy = f;
        tx.broadcast_fisheye_desc(copy);
    };
    auto count = [](const std::vector<Pkt>& p, const char* ch) { int n = 0; for (auto& k : p) n += k.ch == ch; return n; };
    std::vector<Pkt> off, image, whole, replay;
    LoopNetWire tx_off(2), tx_image(2), tx_whole(2), tx_replay(2);
    send(false, false, false, off, tx_off); send(true, false, false, image, tx_image); send(true, true, false, whole, tx_whole); send(false, false, true, replay, tx_replay);
    std::printf("SENT_OFF %zu %d\n", off.size(), count(off, wire::CH_IMG_DES));
    for (auto* p : {&image, &whole}) {
        // the third packet of an image stands behind its landmark packets; its bytes: features or none
        int last = 1, feat = 0, bytes_ok = 1, same_prefix = 1;
        size_t k_off = 0;
        for (size_t k = 0; k < p->size(); ++k) {
            const Pkt& q = (*p)[k];
            if (q.ch != wire::CH_IMG_DES) { same_prefix &= k_off < off.size() && off[k_off].ch == q.ch && off[k_off].b == q.b; ++k_off; continue; }
            last &= k + 1 == p->size() || (*p)[k + 1].ch == wire::CH_HEADER;
            ImageDescriptor d;
            if (!wire::decode(q.b.data(), q.b.size(), d) || d.direction < 0 || d.direction > 3) { bytes_ok = 0; continue; }
            ImageDescriptor src = f.images[d.direction]; src.msg_id = d.msg_id;                      // (the sender numbers its copy)
            bytes_ok &= d.msg_id != 0 && same(src, d, p == &whole) ? 1 : 0;
            feat += !d.feature_descriptor.empty();
        }
        std::printf("SENT_%s %zu %d %d %d %d %d\n", p == &image ? "IMAGE" : "WHOLE", p->size(), count(*p, wire::CH_IMG_DES), last, feat, bytes_ok, same_prefix);
    }
    {
        int whole_ok = 1;
        for (auto& q : replay) { ImageDescriptor d; whole_ok &= q.ch == wire::CH_IMG_DES && wire::decode(q.b.data(), q.b.size(), d) && (int)d.feature_descriptor.size() == 64 * d.landmark_num && d.image.size() == 300u + d.direction; }
        std::printf("SENT_REPLAY %zu %d %d\n", replay.size(), count(replay, wire::CH_IMG_DES), whole_ok);
    }
    // ---- every truncation of a valid packet is dropped (and the packet itself is taken)
    {
        LoopNetWire rx(1);
        const Pkt* wp = nullptr;
        for (auto& q : whole) if (q.ch == wire::CH_IMG_DES) wp = &q;
        int taken = 0;
        for (size_t n = 0; n < wp->b.size(); ++n) taken += rx.on_packet(wire::CH_IMG_DES, wp->b.data(), n, 0.0) ? 1 : 0;
        auto longer = wp->b; longer.push_back(0);
        taken += rx.on_packet(wire::CH_IMG_DES, longer.data(), longer.size(), 0.0) ? 1 : 0;
        const auto eb = wire::encode(random_edge(5, false));
        for (size_t n = 0; n < eb.size(); ++n) taken += rx.on_packet(wire::CH_LOOP_CONN, eb.data(), n, 0.0) ? 1 : 0;
        taken += rx.on_packet(wire::CH_IMG_DES, eb.data(), eb.size(), 0.0) ? 1 : 0;                   // (a packet on the wrong channel)
        taken += rx.on_packet(wire::CH_LOOP_CONN, wp->b.data(), wp->b.size(), 0.0) ? 1 : 0;
        std::printf("TRUNCATED %d %d %d\n", taken, rx.on_packet(wire::CH_IMG_DES, wp->b.data(), wp->b.size(), 0.0) ? 1 : 0, rx.on_packet(wire::CH_LOOP_CONN, eb.data(), eb.size(), 0.0) ? 1 : 0);
    }
    // ---- inconsistent length members: each is dropped.  Offsets of the head's members: landmark_num 36, direction 40, image_desc_size 165, feature_descriptor_size 169,
    //      image_size 173
    {
        LoopNetWire rx(1);
        int callbacks = 0;
        rx.image_callback = [&](const ImageDescriptor&) { ++callbacks; };
        auto take = [&](const std::vector<uint8_t>& b) { return rx.on_packet(wire::CH_IMG_DES, b.data(), b.size(), 0.0) ? 1 : 0; };
        ImageDescriptor im = make_image(1, 10, 50); im.msg_id = 31337;
        const auto good = wire::encode(im, true);
        std::string r;
        auto note = [&](int v) { r += v ? " 1" : " 0"; };
        // right framing, wrong shape
        { ImageDescriptor x = im; x.feature_descriptor.resize(64 * 10); auto b = wire::encode(x, true); b.erase(b.begin() + 177 + 4 * 4096, b.begin() + 177 + 4 * 4096 + 4); put32(b, 169, 64 * 10 - 1); note(take(b)); }
        { ImageDescriptor x = im; auto b = wire::encode(x, false); std::vector<uint8_t> extra(4 * 64, 0); b.insert(b.begin() + 177 + 4 * 4096, extra.begin(), extra.end()); put32(b, 169, 64); note(take(b)); }
        { ImageDescriptor x = im; x.image_desc.resize(100); note(take(wire::encode(x, true))); }
        { ImageDescriptor x = im; x.image_desc.clear(); const int ok = take(wire::encode(x, true)); r += ok ? " (1)" : " (0)"; }                      // (no global descriptor: allowed, as in a header)
        { ImageDescriptor x = im; x.image.assign((size_t)LoopNetWire::MAX_IMAGE_BYTES + 1, 9); note(take(wire::encode(x, true))); }
        { ImageDescriptor x = im; x.image.assign((size_t)LoopNetWire::MAX_IMAGE_BYTES, 9); x.msg_id = 31338; const int ok = take(wire::encode(x, true)); r += ok ? " (1)" : " (0)"; }   // (exactly the cap: taken)
        { ImageDescriptor x = im; x.direction = 4; note(take(wire::encode(x, true))); }
        { ImageDescriptor x = im; x.direction = -1; note(take(wire::encode(x, true))); }
        { ImageDescriptor x = make_image(0, LoopNetWire::MAX_FEATURES + 1, 0); note(take(wire::encode(x, false))); }
        // a length member beyond the packet, or negative: nothing is resized
        for (size_t at : {(size_t)36, (size_t)165, (size_t)169, (size_t)173})
            for (int32_t v : {0x7fffffff, 0x40000000, -1, (int32_t)good.size()}) { auto b = good; put32(b, at, v); note(take(b)); }
        const int good_taken = take(good);
        std::printf("INCONSISTENT%s | %d %d\n", r.c_str(), good_taken, callbacks);
    }
    // ---- a drone ignores its own packets and its own edges; another drone hears them
    {
        int images = 0, edges = 0, frames = 0;
        tx_whole.image_callback = [&](const ImageDescriptor&) { ++images; };
        tx_whole.loopconn_callback = [&](const LoopEdge&) { ++edges; };
        tx_whole.frame_desc_callback = [&](const FisheyeFrameDescriptor&) { ++frames; };
        tx_whole.accept_img_desc = true;
        std::vector<Pkt> sent_edges;
        tx_whole.publish = [&](const char* ch, const std::vector<uint8_t>& b) { sent_edges.push_back({ch, b}); };
        const LoopEdge e1 = random_edge(900, false), e2 = random_edge(901, true);
        tx_whole.broadcast_loop_connection(e1); tx_whole.broadcast_loop_connection(e2);
        for (auto& q : whole) tx_whole.on_packet(q.ch.c_str(), q.b.data(), q.b.size(), 0.0);
        for (auto& q : sent_edges) tx_whole.on_packet(q.ch.c_str(), q.b.data(), q.b.size(), 0.0);
        tx_whole.scan_recv_packets(10.0);
        LoopNetWire rx(1);
        std::vector<LoopEdge> got;
        rx.loopconn_callback = [&](const LoopEdge& e) { got.push_back(e); };
        int all_edges = 1;
        for (auto& q : sent_edges) all_edges &= q.ch == wire::CH_LOOP_CONN && rx.on_packet(q.ch.c_str(), q.b.data(), q.b.size(), 0.0);
        std::printf("OWN %d %d %d | %zu %zu %d %d\n", images, edges, frames, sent_edges.size(), got.size(), all_edges, got.size() == 2 && same(got[0], e1) && same(got[1], e2) ? 1 : 0);
    }
    // ---- the accept_img_desc rule: IMAGE-mode and WHOLE-mode packets, with and without the switch; only the whole-descriptor packets are delivered here
    for (int mode = 0; mode < 2; ++mode)
        for (int accept = 0; accept < 2; ++accept) {
            LoopNetWire rx(1);
            rx.accept_img_desc = accept != 0;
            int images = 0, bad = 0;
            std::vector<FisheyeFrameDescriptor> got;
            rx.image_callback = [&](const ImageDescriptor& d) { ++images; ImageDescriptor s = f.images[d.direction]; s.msg_id = d.msg_id; bad += !same(s, d, mode != 0); };
            rx.frame_desc_callback = [&](const FisheyeFrameDescriptor& fr) { got.push_back(fr); };
            double t = 100.0;
            for (auto& q : mode ? whole : image) if (q.ch == wire::CH_IMG_DES) { rx.on_packet(q.ch.c_str(), q.b.data(), q.b.size(), t); t += 0.001; }
            rx.scan_recv_packets(t + 0.6); rx.scan_recv_packets(t + 1.7);
            int landmarks = 0, content = 1;
            for (auto& fr : got)
                for (auto& im : fr.images) {
                    landmarks += im.landmark_num;
                    if (im.landmark_num) { ImageDescriptor s = f.images[im.direction]; s.msg_id = im.msg_id; content &= same(s, im, true) ? 1 : 0; }
                }
            std::printf("ACCEPT %d %d %d %d %zu %d %d\n", mode, accept, images, bad, got.size(), landmarks, content);
        }
    {   // every packet of a WHOLE-mode drone with the switch on: each image enters the frame flow once (the whole descriptor comes last and is black-listed)
        LoopNetWire rx(1);
        rx.accept_img_desc = true;
        int images = 0;
        std::vector<FisheyeFrameDescriptor> got;
        rx.image_callback = [&](const ImageDescriptor&) { ++images; };
        rx.frame_desc_callback = [&](const FisheyeFrameDescriptor& fr) { got.push_back(fr); };
        double t = 100.0;
        for (auto& q : whole) { rx.on_packet(q.ch.c_str(), q.b.data(), q.b.size(), t); t += 0.001; }
        rx.scan_recv_packets(t + 0.6); rx.scan_recv_packets(t + 1.7);
        int landmarks = 0;
        for (auto& fr : got) for (auto& im : fr.images) landmarks += im.landmark_num;
        std::printf("ACCEPT_ALL %d %zu %d %d %d\n", images, got.size(), landmarks, flagged, all);
    }
    return 0;
}
