// Which kernels one SuperPoint pass runs (superpoint.hip: sp_forward), decided ONCE per pass by a pure function of what is fixed when the handle is
// created (SpHandleFacts: the precision, the image size, the variant switches of config.h) and of the pass itself (SpPassInputs); and the state of the
// fisheye mask's constant region as one value with one transition (sp_mask_skip_step).  This header is the one statement of those rules: sp_forward,
// sp_make_dense, sp_calibrate_mask_skip and sp_postprocess only switch over the plan.  Plain host C++, no HIP: tests/cpp/sp_plan_pin.cpp compiles it
// under g++ and tests/test_sp_plan_cpu.py compares every combination of the switches against an independent restatement.
#pragma once
#include "../../include/omni_hip.h"

namespace omni {

struct SpHandleFacts {
    int precision = OMNI_PREC_F32, H = 0, W = 0;
    int conv_variant = 0;                // OMNI_CONV_V1: 1 = generic conv kernel everywhere, 2 = v2 persistent kernel, 3 = ping-pong without the conv1a fusion (test build)
    bool det16 = true;                   // OMNI_DET16: detector head on the fp16 matrix cores (fp16 and OMNI_PREC_SPLIT)
    bool fused_cand = true;              // OMNI_SP_FUSED_CAND: getKeyPoints' threshold inside the detector head's epilogue
    bool sparse_desc = true;             // OMNI_SP_SPARSE_DESC: convDb + norm only at the cells around the key points, the dense map on demand (omni_sp_get_dense)
    bool sparse_da = true;               // OMNI_SP_SPARSE_DA: convDa only there too (needs sparse_desc; fp16 and OMNI_PREC_SPLIT)
    bool split_fuse1a = true;            // OMNI_SPLIT_FUSE1A: OMNI_PREC_SPLIT builds conv1a inside conv1b's kernel
    bool split_db = true;                // OMNI_SP_SPLIT_DB: OMNI_PREC_SPLIT runs the sparse convDb with split operands (false: the exact-f32 convolution)
    int wino = 0;                        // sp_wino_layers(): the cin = 64 layers that run as Winograd kernels, bit 0 = conv1b, 1 = conv2a, 2 = conv2b, 3 = conv3a
    bool mask_skip = false;              // a rectangle of tiles inside the mask's constant region exists for some layer (sp_plan_mask_skip)
};

// OMNI_SPLIT_WINO as this handle can honour it: F(2x2,3x3) tiles need even maps (conv3a: H / 4, W / 4; conv2a, conv2b: H / 2, W / 2; conv1b: H, W), and
// conv1b's Winograd kernel only exists with the conv1a fusion
inline int sp_wino_layers(int precision, int requested, int H, int W, bool split_fuse1a) {
    if (precision != OMNI_PREC_SPLIT) return 0;
    int m = requested;
    if (H % 8 != 0 || W % 8 != 0) m &= 7;
    if (H % 4 != 0 || W % 4 != 0) m &= 1;
    if (H % 2 != 0 || W % 2 != 0 || !split_fuse1a) m &= ~1;
    return m;
}

struct SpPassInputs {
    bool aligned4 = false;               // image pointer and row stride are multiples of 4 (the fused conv1a reads the image in dwords)
    bool fisheye_mask = false, run_post = false;
    bool calibrating = false;            // the pass over the zero image that sp_calibrate_mask_skip reads the constants from
};

enum SpConv1a { SP_1A_DIRECT = 0, SP_1A_SPLIT, SP_1A_FUSED };                               // conv1a_direct / conv1a_split / none: inside conv1b's kernel
enum SpConv1b { SP_1B_CONV = 0, SP_1B_FUSED_F16, SP_1B_FUSED_SPLIT, SP_1B_FUSED_WINO };     // conv() / conv1ab_fused / conv1ab_split_fused / conv1ab_wino_fused
enum SpDetTail { SP_DET_VALU = 0, SP_DET_MFMA16_F16, SP_DET_MFMA16_F32, SP_DET_MFMA_F32 };  // detector_head / detector_head_mfma16 on fp16 / fp32 input / detector_head_mfma
enum SpDescTail {
    SP_DESC_DENSE_GENERIC = 0,           // 1x1 convDb (generic kernel) + l2norm_channels over the whole map, sampled by sp_sample_kernel
    SP_DESC_DENSE_F16,                   // fp16: convdb_l2norm over the whole map, sampled by sp_sample_kernel
    SP_DESC_SPARSE_F16,                  // fp16: convdb_sparse_sample on the dense cDa half of `heads`
    SP_DESC_SPARSE_DA_F16,               // fp16: conv_c128_sparse (convDa at the key points' cells) + convdb_sparse_sample on its compact rows
    SP_DESC_GATHER_F32,                  // fp32 / split: gather the cDa rows of `heads`, exact-f32 1x1 convDb + l2norm_channels on them
    SP_DESC_SPARSE_DA_SPLIT,             // split: conv_split_c128_sparse, then convdb_l2norm_split (desc_split_db) or the exact-f32 convDb + l2norm_channels
};

// a cin = 64 layer behind conv1b (conv2a, conv2b, conv3a) under OMNI_PREC_SPLIT; every other precision: all false
struct SpC64Plan {
    bool wino = false;                   // conv_wino instead of conv()
    bool convert_in = false;             // its input was left as split-64 frames by a direct kernel: split_to_raw32 into a_tmp first
    bool out_raw32 = false;              // it leaves raw-32 frames (the next layer is a Winograd kernel too) instead of split-64
};

struct SpPassPlan {
    bool calibrating = false;
    SpConv1a conv1a = SP_1A_DIRECT;
    SpConv1b conv1b = SP_1B_CONV;
    bool raw_1b = false;                 // conv1b leaves raw-32 frames
    SpC64Plan conv2a, conv2b, conv3a;
    bool use_skip = false;               // the layers leave the mask's constant rectangles out of their tile walks
    bool heads_sparse_da = false;        // heads layer: cPa alone (256 channels into headsP) instead of cPa | cDa (512 into heads)
    bool tails_f32 = true;               // the heads layer's output (the tails' input) is fp32 (fp32, split) rather than fp16
    SpDetTail det = SP_DET_MFMA_F32;
    bool cand_fused = false;             // the head thresholds its own output into SpPostBuffers::cand_bits
    SpDescTail desc = SP_DESC_DENSE_GENERIC;
    bool desc_split_db = false;
    bool run_post = false;
    // what the pass leaves behind (sp_make_dense updates the first two when it completes them)
    bool dense_valid = false;            // `draw` holds the dense descriptor map
    bool heads_full = true;              // `heads` holds the fused layer's fp32 output (false: split ran cPa alone; fp16 does not consult it: it re-runs the layer)
};

inline SpPassPlan sp_plan_pass(const SpHandleFacts& f, const SpPassInputs& in) {
    const bool f16 = f.precision == OMNI_PREC_F16, split = f.precision == OMNI_PREC_SPLIT, best = f.conv_variant == 0;
    SpPassPlan p;
    p.calibrating = in.calibrating; p.run_post = in.run_post;
    const bool fuse1a = ((f16 && best) || (split && f.split_fuse1a)) && in.aligned4;
    p.conv1a = fuse1a ? SP_1A_FUSED : split ? SP_1A_SPLIT : SP_1A_DIRECT;
    const int wino = split ? f.wino : 0;
    p.conv1b = !fuse1a ? SP_1B_CONV : !split ? SP_1B_FUSED_F16 : (wino & 1) ? SP_1B_FUSED_WINO : SP_1B_FUSED_SPLIT;
    // between two Winograd layers the frame is raw-32; a Winograd layer behind a direct one converts its input
    const bool w[4] = {p.conv1b == SP_1B_FUSED_WINO, (wino & 2) != 0, (wino & 4) != 0, (wino & 8) != 0};
    SpC64Plan* c64[3] = {&p.conv2a, &p.conv2b, &p.conv3a};
    p.raw_1b = w[0] && w[1];
    for (int i = 0; i < 3; ++i) {
        c64[i]->wino = w[i + 1];
        c64[i]->convert_in = w[i + 1] && !w[i];
        c64[i]->out_raw32 = w[i + 1] && i < 2 && w[i + 2];
    }
    // the constant region of the fisheye mask: the persistent kernels of the production path (fp16: only with conv1a fused into conv1b)
    p.use_skip = f.mask_skip && in.fisheye_mask && (fuse1a || split) && !in.calibrating;
    const bool sparse = best && f.sparse_desc && in.run_post;      // descriptors only at the key points' cells; no post-processing, no key points
    const bool sparse_da = sparse && f.sparse_da && (f16 || split);
    p.heads_sparse_da = sparse_da;
    p.tails_f32 = !f16;
    p.det = f.conv_variant == 1 ? SP_DET_VALU : (f16 && f.det16) ? SP_DET_MFMA16_F16 : (split && f.det16) ? SP_DET_MFMA16_F32 : SP_DET_MFMA_F32;
    p.cand_fused = in.run_post && f.fused_cand && f.conv_variant != 1;
    p.desc = sparse ? (f16 ? (sparse_da ? SP_DESC_SPARSE_DA_F16 : SP_DESC_SPARSE_F16) : (sparse_da ? SP_DESC_SPARSE_DA_SPLIT : SP_DESC_GATHER_F32))
                    : (f16 && best) ? SP_DESC_DENSE_F16 : SP_DESC_DENSE_GENERIC;
    p.desc_split_db = p.desc == SP_DESC_SPARSE_DA_SPLIT && f.split_db;
    p.dense_valid = !sparse;
    p.heads_full = p.desc != SP_DESC_SPARSE_DA_SPLIT;
    return p;
}

// The rectangles of the mask's constant region hold valid constants (written by a calibration pass) or not.  conv1a's own rectangle (OMNI_PREC_SPLIT) is
// only filled by an unfused calibration, so the state remembers which conv1a form it was calibrated with.
enum SpMaskSkipState { SP_SKIP_STALE = 0, SP_SKIP_READY_FUSED, SP_SKIP_READY_UNFUSED };
struct SpMaskSkipStep {
    bool calibrate;                      // run sp_calibrate_mask_skip before this pass ...
    int zero_image_offset;               // ... on the zero image this many bytes past its (4-aligned) start
    SpMaskSkipState after;               // the state once this pass is enqueued
};
// A pass that skips needs the constants of its own conv1a form; a pass that does not skip overwrites the rectangles; the calibration pass itself does
// neither.  The calibration takes the conv1a form of the pass it serves: an unfused pass whose row stride would allow the fusion (stride % 4 == 0)
// calibrates one byte into the zero image, so that this pass misses the fusion through its pointer too.
inline SpMaskSkipStep sp_mask_skip_step(SpMaskSkipState state, const SpPassPlan& p, int stride) {
    if (p.calibrating) return {false, 0, state};
    if (!p.use_skip) return {false, 0, SP_SKIP_STALE};
    const bool fused = p.conv1a == SP_1A_FUSED;
    const SpMaskSkipState want = fused ? SP_SKIP_READY_FUSED : SP_SKIP_READY_UNFUSED;
    return {state != want, (!fused && stride % 4 == 0) ? 1 : 0, want};
}

}  // namespace omni
