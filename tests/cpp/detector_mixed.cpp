// detector_mixed.cpp -- LoopDetectorCore's batch whose rows come from both places (host/omni_swarm.hpp: begin_images_batch(frames, unit_rows_dev, n_unit_rows,
// unit_first_row); csrc/rows_assemble.hip) against the frame-by-frame on_image_recv of a second detector.  A plain g++ program linked against libomni_hip.so;
// tests/test_gpu_detector_mixed.py builds it and starts it as a child process on the GPU.
//
// 12 synthetic frames of 3 drones (this drone is 1), 4 images each, rows random unit vectors with near-duplicates planted on both sides of both thresholds, one
// malformed remote frame (an image that claims landmarks with a 100-float descriptor) and one remote image without landmarks.  The self-drone frames' rows are
// uploaded as a "unit" block and their host descriptors are EMPTIED in the batch's copy (what KeyframePipeline's light messages look like): a row the detector took
// from the host would be missing.  Twice: without a geometry stage, and with compute_loop set to a stub that accepts every second candidate while
// inter_drone_init_frames = 1, so that init mode flips inside the batch.  Identical: every LoopCandidate field (the score's bits included), ntotal of both indexes,
// imgid2fisheye, imgid2dir, the loop counters.  Prints one line per run and "OK"; exit code 1 with the first difference otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../omni-swarm_amd/host/omni_swarm.hpp"

using omni::FisheyeFrameDescriptor;
using omni::LoopCandidate;
using omni::LoopDetectorCore;

static std::vector<float> unit_vector(std::mt19937& rng) {
    std::normal_distribution<float> g(0.f, 1.f);
    std::vector<float> v(4096);
    double s = 0;
    for (auto& x : v) { x = g(rng); s += (double)x * x; }
    for (auto& x : v) x = (float)(x / std::sqrt(s));
    return v;
}
// a unit vector whose inner product with `a` is about `ip`
static std::vector<float> near(const std::vector<float>& a, double ip, std::mt19937& rng) {
    const std::vector<float> n = unit_vector(rng);             // (nearly orthogonal to a in 4096 dimensions)
    std::vector<float> v(4096);
    double s = 0;
    for (int i = 0; i < 4096; ++i) { v[i] = (float)(ip * a[i] + std::sqrt(1 - ip * ip) * n[i]); s += (double)v[i] * v[i]; }
    for (auto& x : v) x = (float)(x / std::sqrt(s));
    return v;
}

static std::vector<FisheyeFrameDescriptor> make_frames(uint32_t seed) {
    std::mt19937 rng(seed);
    const int drone[12] = {1, 1, 2, 1, 3, 2, 1, 2, 1, 3, 1, 2};
    std::vector<FisheyeFrameDescriptor> fs(12);
    for (int k = 0; k < 12; ++k) {
        FisheyeFrameDescriptor& f = fs[(size_t)k];
        f.msg_id = 100 + k; f.drone_id = drone[k]; f.timestamp = k; f.image_num = 4;
        f.images.resize(4);
        for (int d = 0; d < 4; ++d) {
            omni::ImageDescriptor& im = f.images[(size_t)d];
            im.drone_id = drone[k]; im.direction = d; im.frame_id = f.msg_id; im.msg_id = 1000 + 4 * k + d; im.landmark_num = 20;
            im.image_desc = unit_vector(rng);
            f.landmark_num += im.landmark_num;
        }
    }
    // the query image is direction 1.  Planted: frame 2 (drone 2) ~0.45 of frame 0: above the init-mode threshold only; frame 3 (self) 0.8 of frame 0: a loop of
    // the self drone, old enough (MATCH_INDEX_DIST = 5); frame 4 (drone 3) 0.8 of frame 1; frame 5 (drone 2) 0.45 of frame 1: found in init mode, missed once init
    // mode is over; frame 6 (self) 0.8 of remote frame 2; frame 7 (drone 2, the malformed one) 0.45 of frame 3: found only while drone 2 is in init mode;
    // frame 8 (self) 0.9 of frame 3; frame 9 (drone 3) 0.45 of frame 6; frame 11 (drone 2) 0.7 of frame 8
    fs[2].images[1].image_desc = near(fs[0].images[1].image_desc, 0.45, rng);
    fs[3].images[1].image_desc = near(fs[0].images[1].image_desc, 0.8, rng);
    fs[4].images[1].image_desc = near(fs[1].images[1].image_desc, 0.8, rng);
    fs[5].images[1].image_desc = near(fs[1].images[1].image_desc, 0.45, rng);
    fs[6].images[1].image_desc = near(fs[2].images[1].image_desc, 0.8, rng);
    fs[7].images[1].image_desc = near(fs[3].images[1].image_desc, 0.45, rng);
    fs[8].images[1].image_desc = near(fs[3].images[1].image_desc, 0.9, rng);
    fs[9].images[1].image_desc = near(fs[6].images[1].image_desc, 0.45, rng);
    fs[11].images[1].image_desc = near(fs[8].images[1].image_desc, 0.7, rng);
    fs[7].images[2].image_desc.resize(100);                    // the malformed remote frame: its image 2 counts as one without landmarks
    fs[9].images[3].landmark_num = 0; fs[9].landmark_num -= 20; fs[9].images[3].image_desc.clear();      // an image without landmarks: a row of zeros, never appended
    fs[10].prevent_adding_db = true;                           // a non-key frame of the self drone: matched, not added
    return fs;
}

static void configure(LoopDetectorCore& det, bool stub, int* calls) {
    det.MATCH_INDEX_DIST = 5;                                  // (above the 4 rows a frame has just appended: a frame does not match itself)
    det.stereo_fisheye = true;
    if (!stub) return;
    det.inter_drone_init_frames = 1;
    det.compute_loop = [calls](const FisheyeFrameDescriptor&, const FisheyeFrameDescriptor&, int, int, bool) { return (++*calls) % 2 == 0; };
}

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

static int compare(const char* what, const std::vector<LoopCandidate>& a, const std::vector<LoopCandidate>& b, LoopDetectorCore& da, LoopDetectorCore& db) {
    if (a.size() != b.size()) { std::printf("FAIL %s: %zu candidates, %zu\n", what, a.size(), b.size()); return 1; }
    for (size_t i = 0; i < a.size(); ++i) {
        const LoopCandidate &x = a[i], &y = b[i];
        if (x.found != y.found || x.old_msg_id != y.old_msg_id || x.image_id != y.image_id || x.direction_new != y.direction_new || x.direction_old != y.direction_old ||
            bits(x.distance) != bits(y.distance) || x.added != y.added || x.queried != y.queried || x.loop != y.loop) {
            std::printf("FAIL %s: frame %zu: batch (found %d old %lld image %d dirs %d %d distance %.9g added %d queried %d loop %d), serial (found %d old %lld image %d dirs %d %d "
                        "distance %.9g added %d queried %d loop %d)\n", what, i, x.found, (long long)x.old_msg_id, x.image_id, x.direction_new, x.direction_old, x.distance, x.added,
                        x.queried, x.loop, y.found, (long long)y.old_msg_id, y.image_id, y.direction_new, y.direction_old, y.distance, y.added, y.queried, y.loop);
            return 1;
        }
    }
    if (da.local_index.ntotal != db.local_index.ntotal || da.remote_index.ntotal != db.remote_index.ntotal) {
        std::printf("FAIL %s: ntotal %lld + %lld, serial %lld + %lld\n", what, (long long)da.local_index.ntotal, (long long)da.remote_index.ntotal, (long long)db.local_index.ntotal,
                    (long long)db.remote_index.ntotal);
        return 1;
    }
    if (da.imgid2fisheye != db.imgid2fisheye || da.imgid2dir != db.imgid2dir) { std::printf("FAIL %s: the id maps differ\n", what); return 1; }
    if (da.inter_drone_loop_count != db.inter_drone_loop_count || da.all_nodes != db.all_nodes) { std::printf("FAIL %s: the loop counters differ\n", what); return 1; }
    if (da.fisheyeframe_database.size() != db.fisheyeframe_database.size()) { std::printf("FAIL %s: the databases differ in size\n", what); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1;
    try {
        omni::Context ctx(0);
        const std::vector<FisheyeFrameDescriptor> frames = make_frames(seed);
        // the self-drone frames' rows as a "unit" block in HBM, in frame order
        std::vector<float> unit;
        std::vector<int64_t> first_row;
        for (const auto& f : frames) {
            if (f.drone_id != 1) { first_row.push_back(-1); continue; }
            first_row.push_back((int64_t)(unit.size() / 4096));
            for (const auto& im : f.images) unit.insert(unit.end(), im.image_desc.begin(), im.image_desc.end());
        }
        const int64_t n_unit_rows = (int64_t)(unit.size() / 4096);
        float* unit_dev = static_cast<float*>(omni_dev_alloc(ctx.get(), unit.size() * 4));
        if (!unit_dev) throw std::runtime_error(omni_last_error());
        omni::check(omni_memcpy_h2d(ctx.get(), unit_dev, unit.data(), unit.size() * 4), "upload");
        int failed = 0;
        for (int stub = 0; stub < 2 && !failed; ++stub) {
            int calls_batch = 0, calls_serial = 0;
            LoopDetectorCore batch(ctx, 1), serial(ctx, 1);
            configure(batch, stub != 0, &calls_batch);
            configure(serial, stub != 0, &calls_serial);
            std::vector<FisheyeFrameDescriptor> mixed = frames;
            for (auto& f : mixed) if (f.drone_id == 1) for (auto& im : f.images) im.image_desc.clear();      // these rows exist in the unit block only
            const std::vector<LoopCandidate> got = batch.on_images_recv_batch(std::move(mixed), unit_dev, n_unit_rows, first_row);
            std::vector<LoopCandidate> want;
            for (const auto& f : frames) want.push_back(serial.on_image_recv(f));
            int found = 0, loops = 0, init_found = 0;
            for (const auto& c : want) { found += c.found; loops += c.loop; init_found += c.found && c.distance < serial.INNER_PRODUCT_THRES; }
            std::printf("RUN stub %d: %zu frames, %d candidates (%d under the init-mode threshold only), %d loops, compute_loop calls %d / %d, rows %lld + %lld\n", stub, want.size(),
                        found, init_found, loops, calls_batch, calls_serial, (long long)serial.local_index.ntotal, (long long)serial.remote_index.ntotal);
            failed = compare(stub ? "stub" : "plain", got, want, batch, serial);
            if (!failed && calls_batch != calls_serial) { std::printf("FAIL: compute_loop calls differ\n"); failed = 1; }
            // conditions on the input, not measurements: both thresholds are crossed, and the stub run's init mode ends inside the batch
            if (!failed && (found < 5 || init_found < 1)) { std::printf("FAIL: the planted duplicates were not found (%d, %d)\n", found, init_found); failed = 1; }
            if (!failed && stub && (loops < 1 || calls_serial < 4)) { std::printf("FAIL: the stub run accepted no loop\n"); failed = 1; }
            // a second batch on the same detectors, of remote frames alone (no unit block): the next ids of drones 2 and 3
            if (!failed) {
                std::vector<FisheyeFrameDescriptor> more;
                for (int k : {2, 4, 5}) { FisheyeFrameDescriptor f = frames[(size_t)k]; f.msg_id += 100; more.push_back(f); }
                const std::vector<FisheyeFrameDescriptor> more_serial = more;
                const std::vector<LoopCandidate> got2 = batch.on_images_recv_batch(std::move(more), nullptr, 0, std::vector<int64_t>(3, -1));
                std::vector<LoopCandidate> want2;
                for (const auto& f : more_serial) want2.push_back(serial.on_image_recv(f));
                failed = compare(stub ? "stub, remote frames alone" : "plain, remote frames alone", got2, want2, batch, serial);
            }
        }
        // the refusals of the new overload: nothing is enqueued, the detector stays usable
        if (!failed) {
            LoopDetectorCore det(ctx, 1);
            int refused = 0;
            try { det.on_images_recv_batch(std::vector<FisheyeFrameDescriptor>(frames), unit_dev, n_unit_rows, std::vector<int64_t>(3, -1)); } catch (const std::invalid_argument&) { ++refused; }
            try { det.on_images_recv_batch(std::vector<FisheyeFrameDescriptor>(frames), unit_dev, 3, first_row); } catch (const std::invalid_argument&) { ++refused; }
            try { det.on_images_recv_batch(std::vector<FisheyeFrameDescriptor>(frames), nullptr, n_unit_rows, first_row); } catch (const std::invalid_argument&) { ++refused; }
            if (refused != 3 || det.batch_pending()) { std::printf("FAIL: %d of 3 refusals\n", refused); failed = 1; }
        }
        omni_dev_free(ctx.get(), unit_dev);
        if (failed) return 1;
        std::printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
}
