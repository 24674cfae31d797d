// Which kernels a MobileNetVLAD pass runs (vlad.hip: vlad_backbone_fused, vlad_forward), decided ONCE per handle and precision by a pure function of what is
// fixed when the handle is created (VladHandleFacts: the layer table's grouping, the OMNI_VLAD_* switches of config.h, the NetVLAD sizes; VladBlockFacts per
// inverted-residual block), and the constant region of the fisheye mask: its rectangles of whole tiles per layer (vlad_plan_mask_rects) and what a pass does
// with them (vlad_pass_skip).  This header is the one statement of those rules: vlad.hip only switches over the plan.  Plain host C++, no HIP:
// tests/cpp/vlad_plan_pin.cpp compiles it under g++ and tests/test_vlad_plan_cpu.py compares every combination against an independent restatement.
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/omni_hip.h"

namespace omni {

// ---- tile shapes (the kernels and the constant-region arithmetic read the same constants) ----
constexpr int SB_TW = 16, SB_TH = 8;                                       // vlad_stem_b0_kernel: output pixels per workgroup
constexpr int VLAD_SBLOCK_TW = 8;                                          // vlad_sblock_kernel: 8 x 8 at stride 1, 4 rows x 8 at stride 2
constexpr int vlad_sblock_th(int stride) { return stride == 1 ? 8 : 4; }
constexpr int VLAD_MBLOCK_TILE = 8;                                        // vlad_mblock_kernel: 8 x 8
constexpr int VLAD_FC_MFMA_K = 256;                                        // vlad_fc_mfma_kernel: its K split divides n_in = K * Dm into groups of this size

struct VladHandleFacts {
    bool fusable = false;                // the layer table grouped into inverted-residual blocks that the fused kernels cover
    bool unfused = false;                // OMNI_VLAD_UNFUSED: the layer-by-layer path even so
    bool sblock = true;                  // OMNI_VLAD_SBLOCK: blocks with a split-fp16 form run on vlad_sblock_kernel
    bool stem_fuse = true;               // OMNI_VLAD_STEM_FUSE: stem + block 0 in one kernel
    bool mfma = true;                    // OMNI_VLAD_MFMA: low-resolution blocks as pointwise MFMA / depthwise / pointwise MFMA
    // OMNI_VLAD_MBLOCK_PX: vlad_mblock_kernel for blocks of at most this many input pixels per image (0: none).  Measured at 32 images
    // (profiles/r02_vlad32_*): the ten 38x30 / 19x15 blocks take 451 us on it vs 502 us as three launches each; on the 75x60 ... 300x240 blocks it is
    // slower than the fp32-VALU fused kernel (one 8x8 tile per workgroup keeps 47-108 KB of LDS: 1-2 workgroups per CU, and every phase of a chunk is a
    // dependent chain behind a barrier -- waves wait 50 % of their life, MFMA-busy 14-18 %).  A split-fp16 variant (v_mfma_f32_32x32x16_f16, hi/lo
    // operands: 5x less matrix time) measured SLOWER still (60 us per block): the matrix pipe is not what bounds these blocks, the per-workgroup latency
    // chain is.
    int mblock_px = 2048;
    int mfma_px = 0;                     // OMNI_VLAD_MFMA_PX: > 0 replaces the 2048 input pixels per image that bound the three-launch path
    bool fc_mfma = true;                 // OMNI_VLAD_FC_MFMA: the FC on the matrix cores
    bool mask_skip = true;               // OMNI_VLAD_MASK_SKIP: masked passes leave the mask's constant region out of the tile walks
    int sb_persist = 1;                  // OMNI_VLAD_SB_PERSIST: an operand of launch_vlad_sblock, no decision depends on it
    int mblock_cpw = 0;                  // OMNI_VLAD_MBLOCK_CPW: chunks of the hidden layer per workgroup of vlad_mblock_kernel (0: all, no split)
    int K = 0, Dm = 0, out_dim = 0, H = 0, W = 0;
};

struct VladStemFacts { int cout = 0, stride = 0; };

struct VladBlockFacts {
    int cin = 0, hid = 0, cout = 0, stride = 1, expand = 0, res = 0;
    int px = 0;                          // input pixels per image
    int hout = 0, wout = 0;
    bool blob = false, mblob = false, hblob = false, sblob = false;        // the packed forms that exist: fp32 VALU / f32 MFMA / fp16 / split fp16
};

// vlad_stem_b0_kernel is written for one shape: a 16-channel stride-2 stem and a t = 1 block 16 -> 16 -> 8 at stride 1 without residual
inline bool vlad_stem_b0_shape(const VladStemFacts& s, const VladBlockFacts& b0) {
    return s.cout == 16 && s.stride == 2 && !b0.expand && !b0.res && b0.cin == 16 && b0.hid == 16 && b0.cout == 8 && b0.stride == 1;
}

enum VladBlockPath {
    VB_HBLOCK = 0,                       // vlad_hblock_kernel (fp16 operands)
    VB_SBLOCK,                           // vlad_sblock_kernel (split-fp16 operands, fp32-class)
    VB_MBLOCK,                           // vlad_mblock_kernel (exact f32 on the matrix cores)
    VB_PW_MFMA3,                         // three launches: vlad_pw_mfma, vlad_dw_kernel, vlad_pw_mfma
    VB_VALU,                             // vlad_block (fp32 VALU)
};

// (per-image sizes, here and below: the numerics of a block do not depend on the batch)
inline bool vlad_mblock_eligible(const VladHandleFacts& f, const VladBlockFacts& b) { return b.mblob && b.px <= f.mblock_px; }

// The priority order of the block kernels.  The three-launch path needs whole groups of 8 channels on both sides of the expansion.
inline VladBlockPath vlad_plan_block(const VladHandleFacts& f, const VladBlockFacts& b, int precision) {
    if (precision == OMNI_PREC_F16 && b.hblob) return VB_HBLOCK;
    if (f.sblock && b.sblob) return VB_SBLOCK;
    if (vlad_mblock_eligible(f, b)) return VB_MBLOCK;
    const int mfma_max_px = f.mfma_px > 0 ? f.mfma_px : 2048;
    if (b.expand && b.cin % 8 == 0 && b.hid % 8 == 0 && b.px <= mfma_max_px && f.mfma) return VB_PW_MFMA3;
    return VB_VALU;
}

// vlad_mblock_kernel's projection is padded to whole 32-column tiles; its hidden-layer split writes [tile][group][64][cop] partial sums
inline int vlad_mblock_cop(int cout) { return (cout + 31) / 32 * 32; }
struct VladMBlockSplit { int cpw, n_groups; size_t partial_bytes; };
inline VladMBlockSplit vlad_mblock_split(const VladHandleFacts& f, const VladBlockFacts& b, int batch) {
    const int n_chunks = (b.hid + 31) / 32, cpw = f.mblock_cpw > 0 ? f.mblock_cpw : n_chunks, n_groups = (n_chunks + cpw - 1) / cpw;
    const size_t tiles = (size_t)((b.wout + VLAD_MBLOCK_TILE - 1) / VLAD_MBLOCK_TILE) * ((b.hout + VLAD_MBLOCK_TILE - 1) / VLAD_MBLOCK_TILE) * batch;
    return {cpw, n_groups, tiles * n_groups * 64 * vlad_mblock_cop(b.cout) * 4};
}
// ... as a pass runs it: without the split when the handle's scratch cannot hold the partial sums
inline VladMBlockSplit vlad_mblock_split(const VladHandleFacts& f, const VladBlockFacts& b, int batch, size_t scratch_bytes) {
    const VladMBlockSplit s = vlad_mblock_split(f, b, batch);
    return s.partial_bytes > scratch_bytes ? VladMBlockSplit{(b.hid + 31) / 32, 1, 0} : s;
}
// the scratch a handle keeps for it: the largest block that may run on vlad_mblock_kernel at the full batch (0: none; more than 1 GB: none, no split)
inline size_t vlad_mblock_scratch_bytes(const VladHandleFacts& f, const std::vector<VladBlockFacts>& blocks, int max_batch) {
    size_t need = 0;
    for (const VladBlockFacts& b : blocks) {
        const size_t bytes = vlad_mblock_eligible(f, b) ? vlad_mblock_split(f, b, max_batch).partial_bytes : 0;
        if (bytes > need) need = bytes;
    }
    return need <= ((size_t)1 << 30) ? need : 0;
}

// One layer's rectangle of whole tiles inside the constant region of the fisheye mask.  LoopCam blanks the bottom quarter of the frame before the network
// runs: inside that band, one 3x3 tap in from its borders per convolution, the output of the stem and of every block is one constant vector.
struct VladSkipRect {
    int ty0 = 0, ty1 = 0, tx0 = 0, tx1 = 0;       // tile rectangle in the layer's output tile grid
    int oy0 = 0, oy1 = 0, ox0 = 0, ox1 = 0;       // the same in output pixels
    int oh = 0, ow = 0, oc = 0;                   // the layer's output map
    double frac = 0.0;                            // the rectangle's share of the layer's tiles
};

enum VladStem { VLAD_STEM4 = 0, VLAD_STEM_B0 };                            // vlad_stem4_kernel, then block 0 as a block / vlad_stem_b0_kernel (stem + block 0)
enum VladHead { VLAD_ASSIGN_AGG = 0, VLAD_ASSIGN2_AGG8 };                  // vlad_assign_kernel + vlad_aggregate_kernel / vlad_assign2_kernel + vlad_aggregate8_kernel
enum VladFc { VLAD_FC_VALU = 0, VLAD_FC4, VLAD_FC_MFMA };                  // vlad_fc_kernel / vlad_fc4_kernel, each followed by l2norm_rows / vlad_fc_mfma_kernel + vlad_fc_finish_kernel

// Where the stem's / the blocks' outputs are constant under the fisheye mask, and the tile rectangles inside: integer arithmetic on (H, W), the layers'
// strides and the kernels' tile shapes.  A 3x3 convolution with padding 1 at stride s reads input rows s r - 1 .. s r + 1: the zero padding is not the
// constant.  [0] = stem + block 0 (vlad_stem_b0_kernel), [k] = block k, as long as the blocks run on vlad_sblock_kernel (the only block kernel with the
// shortened tile walk) and a rectangle exists; the caller has checked the fused path, the switches and vlad_stem_b0_shape.
inline std::vector<VladSkipRect> vlad_plan_mask_rects(int H, int W, const std::vector<VladBlockFacts>& blocks) {
    std::vector<VladSkipRect> rects;
    int m0, m1;
    omni_fisheye_mask_rows(H, 1, &m0, &m1);
    int a = m0, b = m1 - 1, c = 0, d = W - 1;                    // constant rows [a, b] x columns [c, d] (inclusive) of the current map
    auto conv3 = [&](int stride) {                               // through a 3x3 convolution, padding 1
        if (stride == 2) { a = (a + 2) / 2; b = (b - 1) >> 1; c = (c + 2) / 2; d = (d - 1) >> 1; }      // rows 2r - 1 .. 2r + 1 inside [a, b]
        else { a += 1; b -= 1; c += 1; d -= 1; }
    };
    auto plan = [&](int th, int tw, const VladBlockFacts& B) -> bool {
        VladSkipRect k;
        if (b < a || d < c) return false;
        k.ty0 = (a + th - 1) / th; k.ty1 = (b + 1) / th; k.tx0 = (c + tw - 1) / tw; k.tx1 = (d + 1) / tw;
        if (k.ty1 <= k.ty0 || k.tx1 <= k.tx0) return false;
        k.oy0 = k.ty0 * th; k.oy1 = k.ty1 * th; k.ox0 = k.tx0 * tw; k.ox1 = k.tx1 * tw;
        k.oh = B.hout; k.ow = B.wout; k.oc = B.cout;
        k.frac = (double)(k.ty1 - k.ty0) * (k.tx1 - k.tx0) / ((double)((B.hout + th - 1) / th) * ((B.wout + tw - 1) / tw));
        rects.push_back(k);
        return true;
    };
    conv3(2);                                                    // the stem
    conv3(1);                                                    // block 0's depthwise convolution (its projection is 1x1)
    if (!plan(SB_TH, SB_TW, blocks[0])) return rects;
    for (size_t bi = 1; bi < blocks.size(); ++bi) {
        const VladBlockFacts& B = blocks[bi];
        if (!B.sblob || (B.cout * 4) % 16 != 0) break;           // (the constant is written in 16-byte pieces)
        conv3(B.stride);                                         // (expand and projection are 1x1; the residual adds two constants)
        if (!plan(vlad_sblock_th(B.stride), VLAD_SBLOCK_TW, B)) break;
    }
    return rects;
}

// A handle's plan at one precision (omni_vlad_create; omni_vlad_set_precision makes it again): a pass only reads it
struct VladPlan {
    bool fused = false;                  // one kernel per block (false: vlad_backbone_unfused, layer by layer; `stem` and `blocks` are not read)
    VladStem stem = VLAD_STEM4;
    std::vector<VladBlockPath> blocks;   // per block; [0] is not read under VLAD_STEM_B0
    VladHead head = VLAD_ASSIGN_AGG;
    VladFc fc = VLAD_FC_VALU;
    std::vector<VladSkipRect> skip;      // the layers with a rectangle in the mask's constant region: each owns an output buffer (the rotating ones are shared)
    int n_skip() const { return (int)skip.size(); }
};

inline VladPlan vlad_make_plan(const VladHandleFacts& f, const VladStemFacts& stem, const std::vector<VladBlockFacts>& blocks, int precision) {
    VladPlan p;
    p.fused = f.fusable && !f.unfused;
    p.stem = f.stem_fuse && !blocks.empty() && vlad_stem_b0_shape(stem, blocks[0]) ? VLAD_STEM_B0 : VLAD_STEM4;
    for (const VladBlockFacts& b : blocks) p.blocks.push_back(vlad_plan_block(f, b, precision));
    p.head = p.fused && f.K <= 32 ? VLAD_ASSIGN2_AGG8 : VLAD_ASSIGN_AGG;
    const bool fc_mfma = f.fc_mfma && p.fused && f.out_dim % 32 == 0 && (f.K * f.Dm) % VLAD_FC_MFMA_K == 0;
    p.fc = fc_mfma ? VLAD_FC_MFMA : p.fused ? VLAD_FC4 : VLAD_FC_VALU;
    // the rectangles do not depend on the precision (their buffers are allocated once); whether a pass uses them does: vlad_pass_skip
    if (p.fused && f.sblock && f.mask_skip && p.stem == VLAD_STEM_B0) p.skip = vlad_plan_mask_rects(f.H, f.W, blocks);
    return p;
}

// What one pass does with the mask's constant region.  Only vlad_stem_b0_kernel and vlad_sblock_kernel know the shortened tile walk, so a pass at
// OMNI_PREC_F16 (blocks on vlad_hblock_kernel) runs every tile into the rotating buffers, as a pass without the mask does: the rectangles stay valid.
// The calibration pass (a blank masked frame) writes every tile into the layers' own buffers; the constants are read from it.
struct VladPassSkip {
    int n_own = 0;                       // layers [0, n_own) write into their own buffers (the ring of rotating buffers is not advanced) ...
    bool leave_out = false;              // ... and leave their rectangles out of the tile walk
};
inline VladPassSkip vlad_pass_skip(const VladPlan& p, int precision, bool fisheye_mask, bool calibrating) {
    if (calibrating) return {p.n_skip(), false};
    if (p.fused && fisheye_mask && p.n_skip() > 0 && precision != OMNI_PREC_F16) return {p.n_skip(), true};
    return {0, false};
}

}  // namespace omni
