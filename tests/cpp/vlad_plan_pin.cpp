// The plan of a MobileNetVLAD handle (omni-swarm_amd/csrc/vlad_plan.h) on the host, for tests/test_vlad_plan_cpu.py.
//   vlad_plan_pin blocks
//     vlad_plan_block for every combination of precision {0, 1} x blob x mblob x hblob x sblob x OMNI_VLAD_SBLOCK x OMNI_VLAD_MFMA x expand x cin {24, 12} x
//     hid {144, 44} x OMNI_VLAD_MBLOCK_PX {0, 1200} x OMNI_VLAD_MFMA_PX {0, 400} x input pixels kPx[]; one row of int32 each on stdout: those 13 inputs in
//     that order (the last five as their index), then the path.
//   vlad_plan_pin handles
//     vlad_make_plan + vlad_pass_skip at 600 x 480 for every combination of OMNI_VLAD_UNFUSED x fusable x OMNI_VLAD_STEM_FUSE x stem / block 0 shape kShapes[]
//     x K kK[] x OMNI_VLAD_FC_MFMA x out_dim kOut[] x Dm kDm[] x OMNI_VLAD_SBLOCK x OMNI_VLAD_MASK_SKIP x precision x fisheye_mask x calibrating; a row of
//     int32 each: those 13 inputs (indices where a table is named), then fused, stem, head, fc, n_skip > 0, n_own == n_skip > 0, leave_out.
//     The layer table is block 0 of the shape and one 8 -> 48 -> 8 block with every packed form (no block 0 at all for the last shape).
//   vlad_plan_pin plan H W precision stem_cout stem_stride [SWITCH=value ...] [block cin,hid,cout,stride,expand,res,forms ...]
//     (forms: bit 0 blob, 1 mblob, 2 hblob, 3 sblob; the maps' sizes follow from H, W and the strides).  Text lines:
//     "plan fused stem head fc", "blocks path ...", "rect ty0 ty1 tx0 tx1 oy0 oy1 ox0 ox1 oh ow oc frac" per mask-skip layer, and
//     "skip fisheye_mask calibrating n_own leave_out" for the four kinds of pass.
//   vlad_plan_pin mblock hid cout hout wout px MBLOCK_PX MBLOCK_CPW batch scratch_bytes
//     the hidden-layer split of vlad_mblock_kernel for one block with an mblob: "split cpw n_groups partial_bytes" as asked for, "pass cpw n_groups" as a pass
//     with that much scratch runs it, "scratch bytes" = what a handle of max_batch = batch allocates for it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/vlad_plan.h"

using namespace omni;

static const int kPx[8] = {399, 400, 401, 1200, 1201, 2048, 2049, 72000};
static const int kK[4] = {16, 32, 33, 64}, kOut[2] = {4096, 4080}, kDm[3] = {112, 100, 128};
// stem cout, stem stride, block 0: cin, hid, cout, stride, expand, res; the last row: no blocks
static const int kShapes[10][8] = {{16, 2, 16, 16, 8, 1, 0, 0}, {32, 2, 16, 16, 8, 1, 0, 0}, {16, 1, 16, 16, 8, 1, 0, 0}, {16, 2, 8, 16, 8, 1, 0, 0}, {16, 2, 16, 32, 8, 1, 0, 0},
                                   {16, 2, 16, 16, 16, 1, 0, 0}, {16, 2, 16, 16, 8, 2, 0, 0}, {16, 2, 16, 16, 8, 1, 1, 0}, {16, 2, 16, 16, 8, 1, 0, 1}, {16, 2, 0, 0, 0, 0, 0, 0}};

static void put(std::vector<int32_t>& out, std::initializer_list<int> row) { for (int v : row) out.push_back(v); }

// the maps' sizes along the chain: stem, then each block's depthwise convolution (3x3, padding 1)
static void chain_sizes(int H, int W, int stem_stride, std::vector<VladBlockFacts>& blocks) {
    int h = (H - 1) / stem_stride + 1, w = (W - 1) / stem_stride + 1;
    for (VladBlockFacts& b : blocks) {
        b.px = h * w;
        h = (h - 1) / b.stride + 1; w = (w - 1) / b.stride + 1;
        b.hout = h; b.wout = w;
    }
}

static int block_table() {
    std::vector<int32_t> out;
    for (int code = 0; code < 2 * 16 * 2 * 2 * 2 * 2 * 2 * 2 * 2 * 8; ++code) {
        int c = code;
        auto take = [&](int n) { const int v = c % n; c /= n; return v; };
        const int px = take(8), mfma_px = take(2), mblock_px = take(2), hid = take(2), cin = take(2);
        VladBlockFacts b;
        VladHandleFacts f;
        b.expand = take(2); f.mfma = take(2); f.sblock = take(2); b.sblob = take(2); b.hblob = take(2); b.mblob = take(2); b.blob = take(2);
        const int precision = take(2);
        b.cin = cin ? 12 : 24; b.hid = hid ? 44 : 144; b.cout = 8; b.px = kPx[px];
        f.mblock_px = mblock_px ? 1200 : 0; f.mfma_px = mfma_px ? 400 : 0;
        put(out, {precision, b.blob, b.mblob, b.hblob, b.sblob, f.sblock, f.mfma, b.expand, cin, hid, mblock_px, mfma_px, px, (int)vlad_plan_block(f, b, precision)});
    }
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}

static int handle_table() {
    std::vector<int32_t> out;
    for (int code = 0; code < 2 * 2 * 2 * 10 * 4 * 2 * 2 * 3 * 2 * 2 * 2 * 2 * 2; ++code) {
        int c = code;
        auto take = [&](int n) { const int v = c % n; c /= n; return v; };
        const int calibrating = take(2), mask = take(2), precision = take(2);
        VladHandleFacts f;
        f.mask_skip = take(2); f.sblock = take(2);
        const int dm = take(3), od = take(2);
        f.fc_mfma = take(2);
        const int k = take(4), shape = take(10);
        f.stem_fuse = take(2); f.fusable = take(2); f.unfused = take(2);
        f.K = kK[k]; f.Dm = kDm[dm]; f.out_dim = kOut[od]; f.H = 480; f.W = 600;
        const int* s = kShapes[shape];
        VladStemFacts stem;
        stem.cout = s[0]; stem.stride = s[1];
        std::vector<VladBlockFacts> blocks;
        if (s[2]) {
            VladBlockFacts b0, b1;
            b0.cin = s[2]; b0.hid = s[3]; b0.cout = s[4]; b0.stride = s[5]; b0.expand = s[6]; b0.res = s[7]; b0.blob = true;
            b1.cin = b0.cout; b1.hid = 48; b1.cout = 8; b1.expand = 1; b1.blob = b1.mblob = b1.hblob = b1.sblob = true;
            blocks = {b0, b1};
            chain_sizes(f.H, f.W, stem.stride, blocks);
        }
        const VladPlan p = vlad_make_plan(f, stem, blocks, precision);
        const VladPassSkip ps = vlad_pass_skip(p, precision, mask != 0, calibrating != 0);
        if (ps.n_own != 0 && ps.n_own != p.n_skip()) { fprintf(stderr, "n_own is neither 0 nor n_skip\n"); return 1; }
        put(out, {f.unfused, f.fusable, f.stem_fuse, shape, k, f.fc_mfma, od, dm, f.sblock, f.mask_skip, precision, mask, calibrating,
                  p.fused, (int)p.stem, (int)p.head, (int)p.fc, p.n_skip() > 0, ps.n_own > 0, ps.leave_out});
    }
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}

static int one_plan(int argc, char** argv) {
    VladHandleFacts f;
    f.fusable = true; f.K = 32; f.Dm = 112; f.out_dim = 4096;
    f.H = atoi(argv[2]); f.W = atoi(argv[3]);
    const int precision = atoi(argv[4]);
    VladStemFacts stem;
    stem.cout = atoi(argv[5]); stem.stride = atoi(argv[6]);
    std::vector<VladBlockFacts> blocks;
    for (int i = 7; i < argc; ++i) {
        int v[7];
        char name[32];
        int val;
        if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7) {
            VladBlockFacts b;
            b.cin = v[0]; b.hid = v[1]; b.cout = v[2]; b.stride = v[3]; b.expand = v[4]; b.res = v[5];
            b.blob = v[6] & 1; b.mblob = (v[6] & 2) != 0; b.hblob = (v[6] & 4) != 0; b.sblob = (v[6] & 8) != 0;
            blocks.push_back(b);
        } else if (sscanf(argv[i], "%31[A-Z_]=%d", name, &val) == 2) {
            if (!strcmp(name, "UNFUSED")) f.unfused = val != 0;
            else if (!strcmp(name, "SBLOCK")) f.sblock = val != 0;
            else if (!strcmp(name, "STEM_FUSE")) f.stem_fuse = val != 0;
            else if (!strcmp(name, "MFMA")) f.mfma = val != 0;
            else if (!strcmp(name, "MBLOCK_PX")) f.mblock_px = val;
            else if (!strcmp(name, "MFMA_PX")) f.mfma_px = val;
            else if (!strcmp(name, "FC_MFMA")) f.fc_mfma = val != 0;
            else if (!strcmp(name, "MASK_SKIP")) f.mask_skip = val != 0;
            else { fprintf(stderr, "unknown switch %s\n", name); return 2; }
        } else { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    }
    chain_sizes(f.H, f.W, stem.stride, blocks);
    const VladPlan p = vlad_make_plan(f, stem, blocks, precision);
    printf("plan %d %d %d %d\nblocks", (int)p.fused, (int)p.stem, (int)p.head, (int)p.fc);
    for (VladBlockPath b : p.blocks) printf(" %d", (int)b);
    printf("\n");
    for (const VladSkipRect& k : p.skip)
        printf("rect %d %d %d %d %d %d %d %d %d %d %d %.17g\n", k.ty0, k.ty1, k.tx0, k.tx1, k.oy0, k.oy1, k.ox0, k.ox1, k.oh, k.ow, k.oc, k.frac);
    for (int mask = 0; mask < 2; ++mask)
        for (int cal = 0; cal < 2; ++cal) {
            const VladPassSkip ps = vlad_pass_skip(p, precision, mask != 0, cal != 0);
            printf("skip %d %d %d %d\n", mask, cal, ps.n_own, (int)ps.leave_out);
        }
    return 0;
}

static int mblock_split(char** argv) {
    VladBlockFacts b;
    VladHandleFacts f;
    b.mblob = true; b.expand = 1; b.cin = 24;
    b.hid = atoi(argv[2]); b.cout = atoi(argv[3]); b.hout = atoi(argv[4]); b.wout = atoi(argv[5]); b.px = atoi(argv[6]);
    f.mblock_px = atoi(argv[7]); f.mblock_cpw = atoi(argv[8]);
    const int batch = atoi(argv[9]);
    const VladMBlockSplit s = vlad_mblock_split(f, b, batch), p = vlad_mblock_split(f, b, batch, (size_t)atoll(argv[10]));
    printf("split %d %d %zu\npass %d %d\nscratch %zu\n", s.cpw, s.n_groups, s.partial_bytes, p.cpw, p.n_groups, vlad_mblock_scratch_bytes(f, {b}, batch));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 11 && !strcmp(argv[1], "mblock")) return mblock_split(argv);
    if (argc == 2 && !strcmp(argv[1], "blocks")) return block_table();
    if (argc == 2 && !strcmp(argv[1], "handles")) return handle_table();
    if (argc >= 7 && !strcmp(argv[1], "plan")) return one_plan(argc, argv);
    fprintf(stderr, "usage: %s blocks | handles | plan H W precision stem_cout stem_stride [SWITCH=value ...] [cin,hid,cout,stride,expand,res,forms ...]\n", argv[0]);
    return 2;
}
