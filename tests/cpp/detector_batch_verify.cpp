// detector_batch_verify.cpp -- LoopDetectorCore's late verdicts (host/omni_swarm.hpp: defer_loop + resolve_loops; the rule: host/verify_plan.hpp) against the
// frame-by-frame on_image_recv of a second detector that verifies every candidate on the spot through compute_loop.  The frames are the 12-frame, 3-drone mixed
// batch of detector_mixed.cpp, included as it is (its main renamed).  A plain g++ program linked against libomni_hip.so; tests/test_gpu_detector_batch_verify.py
// builds it and starts it as a child process on the GPU.
//
// The verdict is a pure function of the two frames (every candidate a loop, except drone 3's frame 109), inter_drone_init_frames = 3: three of drone 2's candidates
// are pending when one of its later frames arrives with c = 0, u = 3 -- the crossing, which the program finds by walking the serial flow's candidates -- and nowhere
// else does a mode depend on a pending verdict.
// Identical: every LoopCandidate field (`loop` and the score's bits included), ntotal, the id maps, the loop counters; one early resolve, at the crossing; the same
// again with the hooks and frame-by-frame on_image_recv (batches of one: no early resolve).  Prints one line per run and "OK".
#define main detector_mixed_main
#include "detector_mixed.cpp"
#undef main

struct Stub {
    struct Resolve { size_t tickets; int64_t last_new_msg_id; int count_2_before; };
    std::vector<char> pending;
    std::vector<Resolve> resolves;
    int64_t last_new = -1;
    int deferred = 0, direct = 0;
    static bool verdict(const FisheyeFrameDescriptor& nw, const FisheyeFrameDescriptor&) { return nw.msg_id % 100 != 9; }
    void attach(LoopDetectorCore& det, bool late) {
        det.MATCH_INDEX_DIST = 5; det.stereo_fisheye = true; det.inter_drone_init_frames = 3;
        det.compute_loop = [this](const FisheyeFrameDescriptor& a, const FisheyeFrameDescriptor& b, int, int, bool) { ++direct; return verdict(a, b); };
        if (!late) return;
        det.defer_loop = [this](const FisheyeFrameDescriptor& a, const FisheyeFrameDescriptor& b, int, int, bool) {
            pending.push_back(verdict(a, b)); last_new = std::max(a.msg_id, b.msg_id); return (int64_t)deferred++;
        };
        det.resolve_loops = [this, &det] {
            resolves.push_back({pending.size(), last_new, det.inter_drone_loop_count[{2, 1}]});
            std::vector<char> out; out.swap(pending); return out;
        };
    }
};

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1;
    try {
        omni::Context ctx(0);
        const std::vector<FisheyeFrameDescriptor> frames = make_frames(seed);
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
        {
            Stub sb, ss, so;
            LoopDetectorCore batch(ctx, 1), serial(ctx, 1), one(ctx, 1);
            sb.attach(batch, true); ss.attach(serial, false); so.attach(one, true);
            std::vector<FisheyeFrameDescriptor> mixed = frames;
            for (auto& f : mixed) if (f.drone_id == 1) for (auto& im : f.images) im.image_desc.clear();
            const std::vector<LoopCandidate> got = batch.on_images_recv_batch(std::move(mixed), unit_dev, n_unit_rows, first_row);
            std::vector<LoopCandidate> want, got_one;
            for (const auto& f : frames) want.push_back(serial.on_image_recv(f));
            for (const auto& f : frames) got_one.push_back(one.on_image_recv(f));
            int found = 0, loops = 0, inter = 0;
            for (size_t i = 0; i < want.size(); ++i) { found += want[i].found; loops += want[i].loop; }
            inter = sb.deferred;
            std::printf("RUN batch: %zu frames, %d candidates, %d loops, %d deferred + %d direct (serial: %d direct), early resolves %lld, end resolves %lld, count[2,1] %d\n",
                        want.size(), found, loops, sb.deferred, sb.direct, ss.direct, (long long)batch.early_resolves, (long long)batch.end_resolves,
                        serial.inter_drone_loop_count[{2, 1}]);
            failed = compare("batch", got, want, batch, serial);
            if (!failed) failed = compare("batches of one", got_one, want, one, serial);
            if (!failed && sb.deferred + sb.direct != ss.direct) { std::printf("FAIL: %d + %d candidates verified, serial %d\n", sb.deferred, sb.direct, ss.direct); failed = 1; }
            // conditions on the input: the crossing lies inside the batch
            if (!failed && (inter < 5 || serial.inter_drone_loop_count[{2, 1}] < 4 || loops < 5)) { std::printf("FAIL: the batch does not cross inter_drone_init_frames\n"); failed = 1; }
            // Where the serial flow says a mode depends on verdicts that a batch would still be waiting for: walk its candidates with c as of the last resolve and u
            // since.  The stub must have been asked to resolve exactly there, with exactly the tickets pending there, and once more at the batch's end.
            std::vector<size_t> want_tickets;                  // per expected early resolve: the tickets pending
            int crossing_frame = -1;
            {
                std::map<int, int> c, u;
                std::vector<std::pair<int, bool>> pending;     // (remote drone, verdict)
                for (size_t i = 0; i < frames.size(); ++i) {
                    const int d = frames[i].drone_id;
                    if (d != 1 && want[i].queried && c[d] < 3 && c[d] + u[d] >= 3) {
                        want_tickets.push_back(pending.size()); crossing_frame = (int)i;
                        for (auto& t : pending) c[t.first] += t.second;
                        pending.clear(); u.clear();
                    }
                    if (!want[i].found) continue;
                    const int od = frames[(size_t)(want[i].old_msg_id - 100)].drone_id;
                    if (d != od && (d == 1 || od == 1)) { const int x = d != 1 ? d : od; pending.push_back({x, want[i].loop}); ++u[x]; }
                }
                want_tickets.push_back(pending.size());
            }
            std::printf("    expected resolves:");
            for (size_t t : want_tickets) std::printf(" %zu", t);
            std::printf(" tickets; the crossing is in front of frame %d\n", crossing_frame);
            if (!failed && want_tickets.size() != 2) { std::printf("FAIL: the batch should hold exactly one crossing\n"); failed = 1; }      // a condition on the input
            if (!failed && (batch.early_resolves != 1 || batch.end_resolves != 1 || sb.resolves.size() != 2 || sb.resolves[0].tickets != want_tickets[0] ||
                            sb.resolves[1].tickets != want_tickets[1] || sb.resolves[0].count_2_before != 0 || sb.resolves[1].count_2_before != 3 ||
                            sb.resolves[0].last_new_msg_id >= 100 + crossing_frame)) {
                std::printf("FAIL: resolves:");
                for (const auto& r : sb.resolves) std::printf(" (%zu tickets, last %lld, count %d)", r.tickets, (long long)r.last_new_msg_id, r.count_2_before);
                std::printf(" early %lld end %lld\n", (long long)batch.early_resolves, (long long)batch.end_resolves);
                failed = 1;
            }
            if (!failed && (one.early_resolves != 0 || one.end_resolves != so.deferred)) { std::printf("FAIL: batches of one: early %lld end %lld of %d\n", (long long)one.early_resolves, (long long)one.end_resolves, so.deferred); failed = 1; }
            // a second batch of remote frames alone: init mode is over for drone 2, not for drone 3 -- nothing depends on a pending verdict
            if (!failed) {
                std::vector<FisheyeFrameDescriptor> more;
                for (int k : {2, 4, 5}) { FisheyeFrameDescriptor f = frames[(size_t)k]; f.msg_id += 100; more.push_back(f); }
                const std::vector<FisheyeFrameDescriptor> more_serial = more;
                const std::vector<LoopCandidate> got2 = batch.on_images_recv_batch(std::move(more), nullptr, 0, std::vector<int64_t>(3, -1));
                std::vector<LoopCandidate> want2;
                for (const auto& f : more_serial) want2.push_back(serial.on_image_recv(f));
                failed = compare("remote frames alone", got2, want2, batch, serial);
                if (!failed && batch.early_resolves != 1) { std::printf("FAIL: an early resolve in the second batch\n"); failed = 1; }
            }
            // one hook alone is no hook: the compute_loop path
            if (!failed) {
                Stub sh;
                LoopDetectorCore half(ctx, 1);
                sh.attach(half, true);
                half.resolve_loops = nullptr;
                for (const auto& f : frames) half.on_image_recv(f);
                if (sh.deferred != 0 || sh.direct != so.deferred + so.direct || half.inter_drone_loop_count != one.inter_drone_loop_count) { std::printf("FAIL: defer_loop without resolve_loops was used\n"); failed = 1; }
            }
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
