// Holds csrc/wire_plan.h to host/loop_net_wire.hpp: omni_wire_pack_host (the g++ build of the plan, csrc/wire_pack_host.cpp compiled into this program) plus the
// host's id patch (wp::patch_header_id / patch_landmark_ids with LoopNetWire's own sequence) must equal the concatenated output of
// LoopNetWire::broadcast_fisheye_desc byte for byte, on random frames and on the edges named below.  Every packet must decode with wire::decode and encode back to
// itself.  Stand-alone, meant for -fsanitize=address,undefined: every buffer is a heap block of exactly the promised size, and the packet buffers are filled with 0xA5
// beforehand so that a byte written behind the last packet shows.
// Prints one line per case: CASE <name> <images> <packets> <bytes> <feature_num of each sent image ...>, then OK <cases>.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../omni-swarm_amd/host/loop_net_wire.hpp"
#include "../../omni-swarm_amd/csrc/wire_pack_host.cpp"

namespace omni {
static std::string g_error;
void set_error(const char* fmt, ...) { char b[512]; va_list ap; va_start(ap, fmt); std::vsnprintf(b, sizeof b, fmt, ap); va_end(ap); g_error = b; }
}  // namespace omni

using namespace omni;

static float bits_f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Frame {
    int n_images, max_num, send_all = 0, self_id = 2;
    float *kps, *desc, *norm, *l3d, *global;
    int* n_kps;
    uint8_t* flag;
    omni_wire_image_meta* meta;
    Frame(int n, int m) : n_images(n), max_num(m) {
        kps = new float[(size_t)n * m * 2](); desc = new float[(size_t)n * m * 64](); norm = new float[(size_t)n * m * 2](); l3d = new float[(size_t)n * m * 3]();
        global = new float[(size_t)n * 4096](); n_kps = new int[n](); flag = new uint8_t[(size_t)n * m](); meta = new omni_wire_image_meta[n]();
    }
    ~Frame() { delete[] kps; delete[] desc; delete[] norm; delete[] l3d; delete[] global; delete[] n_kps; delete[] flag; delete[] meta; }
    void randomise(std::mt19937& rng) {
        std::uniform_real_distribution<float> U(-1.f, 1.f);
        std::uniform_real_distribution<double> D(-10., 10.);
        const size_t nm = (size_t)n_images * max_num;
        for (size_t i = 0; i < nm * 2; ++i) { kps[i] = 300.f * (1.f + U(rng)); norm[i] = U(rng); }
        for (size_t i = 0; i < nm * 64; ++i) desc[i] = U(rng);
        for (size_t i = 0; i < nm * 3; ++i) l3d[i] = 5.f * U(rng);
        for (size_t i = 0; i < (size_t)n_images * 4096; ++i) global[i] = U(rng);
        for (size_t i = 0; i < nm; ++i) flag[i] = (rng() % 3) != 0;
        for (int g = 0; g < n_images; ++g) {
            n_kps[g] = 1 + (int)(rng() % (unsigned)max_num);
            omni_wire_image_meta& m = meta[g];
            m.timestamp = 1.6e9 + D(rng); m.frame_id = ((int64_t)rng() << 20) ^ rng(); m.drone_id = self_id; m.direction = g % 4; m.prevent_adding_db = (int)(rng() & 1);
            for (int k = 0; k < 7; ++k) { m.pose_drone[k] = D(rng); m.camera_extrinsic[k] = D(rng); }
        }
    }
    void flag_exactly(int g, int count) {        // the first `count` odd-or-even-spread slots of image g
        for (int i = 0; i < max_num; ++i) flag[(size_t)g * max_num + i] = 0;
        int done = 0;
        for (int i = 0; i < n_kps[g] && done < count; i += 2, ++done) flag[(size_t)g * max_num + i] = 1;
        for (int i = 1; i < n_kps[g] && done < count; i += 2, ++done) flag[(size_t)g * max_num + i] = 1;
        if (done != count) { std::printf("FAIL flag_exactly\n"); std::exit(1); }
    }
};

static int g_cases = 0;

static void fail(const char* name, const char* what) { std::printf("FAIL %s: %s\n", name, what); std::exit(1); }

static void run_case(const char* name, Frame& f) {
    // the reference path: the message LoopNetWire would be handed, through broadcast_fisheye_desc
    FisheyeFrameDescriptor msg;
    msg.image_num = f.n_images;
    for (int g = 0; g < f.n_images; ++g) {
        const omni_wire_image_meta& m = f.meta[g];
        ImageDescriptor im;
        const int n = f.n_kps[g] < 0 ? 0 : f.n_kps[g] > f.max_num ? f.max_num : f.n_kps[g];
        const size_t at = (size_t)g * f.max_num;
        im.drone_id = m.drone_id; im.landmark_num = n; im.direction = m.direction; im.frame_id = m.frame_id; im.timestamp = m.timestamp;
        im.prevent_adding_db = m.prevent_adding_db != 0;
        im.image_desc.assign(f.global + (size_t)g * 4096, f.global + (size_t)(g + 1) * 4096);
        im.feature_descriptor.assign(f.desc + at * 64, f.desc + (at + n) * 64);
        for (int i = 0; i < n; ++i) {
            const float *k2 = f.kps + (at + i) * 2, *n2 = f.norm + (at + i) * 2, *p3 = f.l3d + (at + i) * 3;
            Point2f p{k2[0], k2[1]}, q{n2[0], n2[1]};
            Point3f l; l.x = p3[0]; l.y = p3[1]; l.z = p3[2];
            im.landmarks_2d.push_back(p); im.landmarks_2d_norm.push_back(q); im.landmarks_3d.push_back(l); im.landmarks_flag.push_back(f.flag[at + i]);
        }
        std::memcpy(im.pose_drone.position, m.pose_drone, 24); std::memcpy(im.pose_drone.quat_wxyz, m.pose_drone + 3, 32);
        std::memcpy(im.camera_extrinsic.position, m.camera_extrinsic, 24); std::memcpy(im.camera_extrinsic.quat_wxyz, m.camera_extrinsic + 3, 32);
        msg.images.push_back(im);
    }
    std::vector<uint8_t> want;
    std::vector<size_t> want_sizes;
    std::vector<std::string> want_ch;
    LoopNetWire tx(f.self_id);
    tx.SEND_ALL_FEATURES = f.send_all != 0;
    tx.publish = [&](const char* ch, const std::vector<uint8_t>& b) { want.insert(want.end(), b.begin(), b.end()); want_sizes.push_back(b.size()); want_ch.push_back(ch); };
    tx.broadcast_fisheye_desc(msg);

    // the plan: buffers of exactly the promised size
    const int64_t cap = omni_wire_packet_capacity(f.max_num);
    const int te = omni_wire_table_ints(f.max_num);
    if (cap != 3 + 16545 + 324 * (int64_t)f.max_num || te != 2 + 2 * (1 + f.max_num)) fail(name, "capacity formula");
    uint8_t* out = new uint8_t[(size_t)cap * f.n_images];
    int* table = new int[(size_t)te * f.n_images];
    std::memset(out, 0xA5, (size_t)cap * f.n_images);
    for (int i = 0; i < te * f.n_images; ++i) table[i] = -77;
    if (omni_wire_pack_host(f.n_images, f.max_num, 64, 4096, f.send_all, f.kps, f.n_kps, f.desc, f.norm, f.l3d, f.flag, f.global, f.meta, out, table) != OMNI_OK)
        fail(name, g_error.c_str());

    // the host's id patch in LoopNetWire's own sequence (next_id: header first, then its landmarks, image after image), then concatenation through the tables
    std::vector<uint8_t> got;
    std::vector<size_t> got_sizes;
    std::vector<std::string> got_ch;
    std::string features;
    int64_t counter = 0;
    auto next_id = [&] { return ((int64_t)f.self_id << 40) | (++counter); };
    for (int g = 0; g < f.n_images; ++g) {
        uint8_t* buf = out + (size_t)g * cap;
        const int* tb = table + (size_t)g * te;
        const int n = f.n_kps[g] < 0 ? 0 : f.n_kps[g] > f.max_num ? f.max_num : f.n_kps[g];
        if ((tb[0] == 0) != (n == 0)) fail(name, "an image is sent exactly when it has key points");
        if (tb[0] < 0 || tb[0] > 1 + f.max_num || tb[1] < 0 || tb[1] > cap) fail(name, "table head out of range");
        for (int e = 2 + 2 * tb[0]; e < te; ++e) if (tb[e] != 0) fail(name, "unused table entries must be zero");
        for (int64_t b = tb[1]; b < cap; ++b) if (buf[b] != 0xA5) fail(name, "a byte behind the last packet was written");
        int64_t header_id = 0, end = 0;
        for (int k = 0; k < tb[0]; ++k) {
            const int off = tb[2 + 2 * k], size = tb[3 + 2 * k];
            if (off < 0 || size <= 0 || (int64_t)off + size > tb[1]) fail(name, "packet outside the used bytes");
            if (k == 0 ? (off != 3 || size != 16545) : (off != 16548 + 324 * (k - 1) || size != 324)) fail(name, "packet placement");
            if ((off + (k == 0 ? 161 : 68)) % 4 != 0) fail(name, "float area not on a 4-byte boundary");
            if (k == 0) { header_id = next_id(); wp::patch_header_id(buf + off, header_id); }
            else wp::patch_landmark_ids(buf + off, next_id(), header_id);
            got.insert(got.end(), buf + off, buf + off + size); got_sizes.push_back((size_t)size); got_ch.push_back(k == 0 ? wire::CH_HEADER : wire::CH_LANDMARKS);
            end = (int64_t)off + size;
            // every packet decodes and round-trips
            if (k == 0) {
                wire::ImageDescriptorHeader h;
                if (!wire::decode(buf + off, (size_t)size, h)) fail(name, "header does not decode");
                const std::vector<uint8_t> again = wire::encode(h);
                if (again.size() != (size_t)size || std::memcmp(again.data(), buf + off, (size_t)size) != 0) fail(name, "header does not round-trip");
                int flagged = 0;
                for (int i = 0; i < n; ++i) flagged += f.flag[(size_t)g * f.max_num + i] > 0;
                if (h.feature_num != flagged || h.msg_id != header_id) fail(name, "feature_num counts the flagged landmarks");
                features += " " + std::to_string(h.feature_num);
            } else {
                wire::LandmarkDescriptor l;
                if (!wire::decode(buf + off, (size_t)size, l)) fail(name, "landmark does not decode");
                const std::vector<uint8_t> again = wire::encode(l);
                if (again.size() != (size_t)size || std::memcmp(again.data(), buf + off, (size_t)size) != 0) fail(name, "landmark does not round-trip");
                if (l.header_id != header_id) fail(name, "header_id");
            }
        }
        if (end != tb[1]) fail(name, "bytes used is the end of the last packet");
    }
    if (got_sizes != want_sizes || got_ch != want_ch) fail(name, "packet sequence differs from broadcast_fisheye_desc");
    if (got != want) fail(name, "bytes differ from broadcast_fisheye_desc");
    std::printf("CASE %s %d %zu %zu%s\n", name, f.n_images, got_sizes.size(), got.size(), features.c_str());
    delete[] out;
    delete[] table;
    ++g_cases;
}

int main(int argc, char** argv) {
    std::mt19937 rng(argc > 1 ? std::atoi(argv[1]) : 1);
    for (int r = 0; r < 6; ++r) {                              // random frames: 1..8 images, several sizes, both settings of send_all_features
        const int sizes[6] = {200, 65, 1, 1024, 64, 257};
        Frame f(1 + (int)(rng() % 8), sizes[r]);
        f.randomise(rng); f.send_all = r & 1; f.self_id = 1 + r;
        for (int g = 0; g < f.n_images; ++g) f.meta[g].drone_id = f.self_id;
        run_case(("random" + std::to_string(r)).c_str(), f);
    }
    { Frame f(3, 200); f.randomise(rng); f.n_kps[1] = 0; run_case("no_keypoints", f); }                                  // image 1 gets no packets
    { Frame f(2, 200); f.randomise(rng); f.n_kps[0] = 120; f.flag_exactly(0, 0); run_case("no_flag", f); }            // header with feature_num 0, no landmark packets
    { Frame f(2, 200); f.randomise(rng); f.n_kps[1] = 200; f.flag_exactly(1, 200); run_case("all_flagged", f); }
    for (int c : {63, 64, 65}) { Frame f(1, 200); f.randomise(rng); f.n_kps[0] = 200; f.flag_exactly(0, c); run_case(("flagged" + std::to_string(c)).c_str(), f); }
    { Frame f(2, 200); f.randomise(rng); f.send_all = 1; f.n_kps[0] = 150; f.flag_exactly(0, 40); run_case("send_all", f); }   // 150 packets, feature_num 40
    { Frame f(2, 65); f.randomise(rng); f.n_kps[0] = 9999; f.n_kps[1] = -3; run_case("clamped_counts", f); }           // n_kps clamped to [0, max_num]
    {                                                          // payload bits: quiet and signalling NaNs with payloads, infinities, -0.0, denormals
        Frame f(1, 65); f.randomise(rng); f.n_kps[0] = 65; f.flag_exactly(0, 65);
        const uint32_t odd[8] = {0x7fc12345u, 0xffc00001u, 0x7f812345u, 0x7f800000u, 0xff800000u, 0x80000000u, 0x00000001u, 0x807fffffu};
        for (int i = 0; i < 65 * 64; ++i) if (i % 5 == 0) f.desc[i] = bits_f(odd[(i / 5) % 8]);
        for (int i = 0; i < 4096; ++i) if (i % 7 == 0) f.global[i] = bits_f(odd[(i / 7) % 8]);
        for (int i = 0; i < 65 * 2; ++i) { f.norm[i] = bits_f(odd[i % 8]); f.kps[i] = bits_f(odd[(i + 3) % 8]); }
        for (int i = 0; i < 65 * 3; ++i) f.l3d[i] = bits_f(odd[(i + 5) % 8]);
        uint64_t nan64 = 0x7ff8000000abcdefull, negzero = 0x8000000000000000ull;
        std::memcpy(&f.meta[0].pose_drone[1], &nan64, 8); std::memcpy(&f.meta[0].camera_extrinsic[6], &negzero, 8); std::memcpy(&f.meta[0].timestamp, &negzero, 8);
        f.meta[0].drone_id = -5; f.meta[0].direction = 3; f.meta[0].frame_id = -1234567890123ll;
        run_case("payload_bits", f);
    }
    // the refusals of the host entry
    {
        Frame f(1, 8); std::mt19937 r2(5); f.randomise(r2);
        uint8_t out[8]; int table[8];
        auto call = [&](int ni, int mn, int dd, int gd, const float* kps) { return omni_wire_pack_host(ni, mn, dd, gd, 0, kps, f.n_kps, f.desc, f.norm, f.l3d, f.flag, f.global, f.meta, out, table); };
        if (call(1, 8, 64, 4096, nullptr) != OMNI_ERR_INVALID || call(0, 8, 64, 4096, f.kps) != OMNI_ERR_INVALID || call(1, 0, 64, 4096, f.kps) != OMNI_ERR_INVALID ||
            call(1, 1025, 64, 4096, f.kps) != OMNI_ERR_INVALID || call(1, 8, 63, 4096, f.kps) != OMNI_ERR_INVALID || call(1, 8, 64, 4095, f.kps) != OMNI_ERR_INVALID)
            fail("refusals", "a bad argument was accepted");
        if (omni_wire_packet_capacity(0) != 0 || omni_wire_packet_capacity(1025) != 0 || omni_wire_table_ints(0) != 0) fail("refusals", "capacity of a bad max_num");
    }
    std::printf("OK %d\n", g_cases);
    return 0;
}
