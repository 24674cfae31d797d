// The plan of a SuperPoint pass (omni-swarm_amd/csrc/sp_plan.h) on the host, for tests/test_sp_plan_cpu.py.
//   sp_plan_pin plans
//     every combination of precision {0, 1, 2} x conv_variant {0..3} x det16 x fused_cand x sparse_desc x sparse_da x split_fuse1a x split_db x requested
//     Winograd mask {0..15} x (H, W) in {(480, 600), (72, 104), (68, 100), (66, 98)} x mask-skip plan exists x aligned4 x fisheye_mask x run_post x calibrating,
//     one row of bytes each on stdout: those 15 inputs in that order ((H, W) as its index), then sp_wino_layers() and the plan's fields as main() lists them.
//   sp_plan_pin skip precision split_fuse1a [aligned4 fisheye_mask stride] ...
//     the passes in order on ONE mask-skip state (600 x 480, every other switch at its default, a mask-skip plan exists); per pass one text line:
//     "calibrate zero_image_offset state_after use_skip"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/sp_plan.h"

using namespace omni;

static const int kSizes[4][2] = {{480, 600}, {72, 104}, {68, 100}, {66, 98}};

static int skip_sequence(int argc, char** argv) {
    SpHandleFacts f;
    f.precision = atoi(argv[2]); f.H = 480; f.W = 600; f.split_fuse1a = atoi(argv[3]) != 0; f.mask_skip = true;
    f.wino = sp_wino_layers(f.precision, 7, f.H, f.W, f.split_fuse1a);
    SpMaskSkipState state = SP_SKIP_STALE;
    for (int i = 4; i + 2 < argc; i += 3) {
        SpPassInputs in;
        in.aligned4 = atoi(argv[i]) != 0; in.fisheye_mask = atoi(argv[i + 1]) != 0; in.run_post = true;
        const SpPassPlan p = sp_plan_pass(f, in);
        const SpMaskSkipStep step = sp_mask_skip_step(state, p, atoi(argv[i + 2]));
        if (step.calibrate) {               // the calibration pass itself goes through the same transition and must leave the state alone
            SpPassInputs cal = in;
            cal.fisheye_mask = true; cal.run_post = false; cal.calibrating = true;
            cal.aligned4 = atoi(argv[i + 2]) % 4 == 0 && step.zero_image_offset == 0;       // (the zero image starts 4-byte aligned)
            const SpMaskSkipStep inner = sp_mask_skip_step(state, sp_plan_pass(f, cal), atoi(argv[i + 2]));
            if (inner.calibrate || inner.after != state) { fprintf(stderr, "the calibration pass changed the state\n"); return 1; }
        }
        state = step.after;
        printf("%d %d %d %d\n", (int)step.calibrate, step.calibrate ? step.zero_image_offset : 0, (int)state, (int)p.use_skip);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "skip")) return skip_sequence(argc, argv);
    if (argc != 2 || strcmp(argv[1], "plans")) {
        fprintf(stderr, "usage: %s plans | skip precision split_fuse1a [aligned4 fisheye_mask stride] ...\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> out;
    for (int code = 0; code < 3 * 4 * 64 * 16 * 4 * 2 * 16; ++code) {
        int c = code;
        auto take = [&](int n) { const int v = c % n; c /= n; return v; };
        const int calibrating = take(2), run_post = take(2), mask = take(2), aligned4 = take(2), mask_skip = take(2), size = take(4), wino_req = take(16);
        SpHandleFacts f;
        f.split_db = take(2); f.split_fuse1a = take(2); f.sparse_da = take(2); f.sparse_desc = take(2); f.fused_cand = take(2); f.det16 = take(2);
        f.conv_variant = take(4); f.precision = take(3);
        f.H = kSizes[size][0]; f.W = kSizes[size][1]; f.mask_skip = mask_skip != 0;
        f.wino = sp_wino_layers(f.precision, wino_req, f.H, f.W, f.split_fuse1a);
        SpPassInputs in;
        in.aligned4 = aligned4 != 0; in.fisheye_mask = mask != 0; in.run_post = run_post != 0; in.calibrating = calibrating != 0;
        const SpPassPlan p = sp_plan_pass(f, in);
        const int row[] = {f.precision, f.conv_variant, f.det16, f.fused_cand, f.sparse_desc, f.sparse_da, f.split_fuse1a, f.split_db, wino_req, size, mask_skip,
                           aligned4, mask, run_post, calibrating,
                           f.wino, p.conv1a, p.conv1b, p.raw_1b, p.conv2a.wino, p.conv2a.convert_in, p.conv2a.out_raw32, p.conv2b.wino, p.conv2b.convert_in,
                           p.conv2b.out_raw32, p.conv3a.wino, p.conv3a.convert_in, p.conv3a.out_raw32, p.use_skip, p.heads_sparse_da, p.tails_f32, p.det,
                           p.cand_fused, p.desc, p.desc_split_db, p.dense_valid, p.heads_full, p.run_post, p.calibrating};
        for (int v : row) out.push_back((uint8_t)v);
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
