// omni_sp_*: drop-in for SuperPointTensorRT (swarm_loop/include/swarm_loop/superpoint_tensorrt.h:12-29,
// swarm_loop/src/superpoint_tensorrt.cpp:91-230) including the TensorRT engine it wraps (the graph of
// swarm_loop/superpoint.ipynb:135-205) and the runner plumbing of tensorrt_generic.cpp:14-120.
//
// HBM layout per handle (sized for max_batch images, all NHWC, element type = precision):
//   a1a [B][H][W][64]   a1b [B][H/2][W/2][64]   a2a  a2b [B][H/4][W/4][64]   a3a [..][128]  a3b [B][H/8][W/8][128]
//   a4a a4b [..][128]   heads [B][Hc][Wc][512] (cPa | cDa, one fused N=512 conv; fp32 under OMNI_PREC_SPLIT)   draw [B][Hc][Wc][256] fp32
//   semi [B][H][W] fp32
//   headsP [B][Hc][Wc][256] cPa alone, for the passes that run convDa only at the key points' cells (fp16; OMNI_PREC_SPLIT: fp32)
//   da_compact [B][max_num][4][256] fp16 (fp16 path) / cx32, cy32 [ceil8(B * max_num * 4)][256] fp32 (fp32, split): cDa at the four coarse cells around
//   every key point, and (cy32) convDb + norm of those rows
// OMNI_PREC_SPLIT keeps every activation map in a zero frame (conv.h: split-64, or raw-32 between two Winograd layers).
// Which kernels a pass runs on these buffers is decided by sp_plan_pass (sp_plan.h), nowhere else.
#include <algorithm>
#include <vector>

#include "config.h"
#include "conv.h"
#include "sp_plan.h"
#include "sp_post.h"

namespace {
struct LayerDef { const char* name; int cin, cout, ks, div; bool pool; };     // div: the layer's INPUT map is H / div x W / div; pool: 2x2 max-pool behind it
const LayerDef kLayers[OMNI_SP_NUM_LAYERS] = {
    {"conv1a", 1, 64, 3, 1, false},    {"conv1b", 64, 64, 3, 1, true},     {"conv2a", 64, 64, 3, 2, false},    {"conv2b", 64, 64, 3, 2, true},
    {"conv3a", 64, 128, 3, 4, false},  {"conv3b", 128, 128, 3, 4, true},   {"conv4a", 128, 128, 3, 8, false},  {"conv4b", 128, 128, 3, 8, false},
    {"convPa", 128, 256, 3, 8, false}, {"convPb", 256, 65, 1, 8, false},   {"convDa", 128, 256, 3, 8, false},  {"convDb", 256, 256, 1, 8, false}};
enum { L1A = 0, L1B, L2A, L2B, L3A, L3B, L4A, L4B, LPA, LPB, LDA, LDB };
// profiling stages
enum { ST_CONV1A = 0, ST_CONV1B, ST_CONV2A, ST_CONV2B, ST_CONV3A, ST_CONV3B, ST_CONV4A, ST_CONV4B, ST_HEADS_A,
       ST_DET_TAIL, ST_DESC_TAIL, ST_POST, ST_COUNT };
const char* kStageNames[OMNI_SP_NUM_STAGES] = {
    "conv1a", "conv1b+pool", "conv2a", "conv2b+pool", "conv3a", "conv3b+pool", "conv4a", "conv4b", "convPa|convDa",
    "convPb+softmax+d2s", "convDb+l2norm", "nms+topk+describe", "", "", "", ""};
}  // namespace

struct omni_sp {
    omni_ctx* ctx = nullptr;
    omni::Config cfg;                        // the switches as they stood when the handle was created (config.h)
    omni::SpHandleFacts facts;               // ... and what sp_plan_pass reads of them (sp_plan.h)
    omni::SpPassPlan last;                   // the plan of the last forward pass: what it left in the buffers (sp_make_dense, omni_sp_debug_layer)
    omni::SpMaskSkipState skip_state = omni::SP_SKIP_STALE;
    omni::DevMem mem;                        // every device allocation of the handle (common.h)
    int W = 0, H = 0, Hc = 0, Wc = 0, max_num = 0, max_batch = 0, precision = 0, pca_dim = 0, desc_dim = 256;
    float thres = 0.f;
    size_t esz = 4;
    // weights
    void* wpk[OMNI_SP_NUM_LAYERS] = {};     // packed MFMA weights (L1B..L4B, LDB) ; heads_a fused in wpk[LPA]
    float* bias[OMNI_SP_NUM_LAYERS] = {};
    float* bias_s[OMNI_SP_NUM_LAYERS] = {};  // OMNI_PREC_SPLIT: conv_split_act_scale() * bias (the split layers write scaled activations)
    float winv[OMNI_SP_NUM_LAYERS] = {};     // OMNI_PREC_SPLIT: 2^-k of the layer's weight scaling
    float* w1a = nullptr;                    // [64][9]
    float* wPbT = nullptr;                   // [256][65]
    float *wPbA = nullptr, *wPbDust = nullptr; // convPb in MFMA A-fragment order + the dustbin row
    void* wPbA16 = nullptr;                    // convPb as split-fp16 A fragments (detector_head_mfma16_kernel); OMNI_DET16=0 keeps the f32 MFMA head
    void* headsP = nullptr;                  // [B][Hc][Wc][256] cPa alone (passes with convDa at the key points only)
    void* da_compact = nullptr;              // [B][max_num][4][256] fp16: cDa at the corner cells of the key points
    float *cx32 = nullptr, *cy32 = nullptr;  // fp32 paths: the gathered cDa rows / their convDb + norm, [ceil8(B * max_num * 4)][256] each
    int last_batch = 0;                      // images of the last forward pass (0: none yet -- nothing to make a dense map from)
    int post_batch = 0;                      // images of the last pass that ran sp_postprocess (0: none yet -- pb.raw_desc / pb.norm_partial hold nothing)
    void* wDbFrag = nullptr;                    // convDb as register-resident fp16 A fragments (fused convDb + L2 norm, fp16 path)
    void* wDbFragHi = nullptr; void* wDbFragLo = nullptr;      // OMNI_PREC_SPLIT: the same as (hi, lo) pairs (convdb_l2norm_split); OMNI_SP_SPLIT_DB=0: exact-f32 convDb
    float* bias_heads = nullptr;             // [512]
    float* lut = nullptr;
    uint16_t* w1a_frag = nullptr;            // conv1a split-fp16 A fragments (fused conv1a+conv1b, fp16 path)
    uint32_t* lut_hl = nullptr;              // u8 -> (half hi, half lo) table
    // OMNI_PREC_SPLIT, Winograd F(2x2,3x3) kernels (conv_wino.hip) for the cin = 64 layers named by facts.wino: their weights; a_tmp: the converted
    // input of a Winograd layer behind a direct one (mixed configurations only, allocated by the first pass that needs it)
    void* wpk_w[OMNI_SP_NUM_LAYERS] = {};
    float winv_w[OMNI_SP_NUM_LAYERS] = {};
    void* a_tmp = nullptr;
    float* pca_compT = nullptr;
    float* pca_mean = nullptr;
    // activations
    void *a1a = nullptr, *a1b = nullptr, *a2a = nullptr, *a2b = nullptr, *a3a = nullptr, *a3b = nullptr, *a4a = nullptr,
         *a4b = nullptr, *heads = nullptr;
    float *draw = nullptr, *semi = nullptr;
    uint8_t* gray_stage = nullptr;           // device copy for host-pointer entry points
    omni::SpPostBuffers pb = {};
    omni::HostBuf hstage;
    omni::DevBuf dense_tmp;
    hipEvent_t ev[OMNI_SP_NUM_STAGES + 1] = {};
    hipEvent_t ev_convs = nullptr;           // recorded behind the last CU-filling kernel of a pass (the detector head): what omni_cam_order_after waits for
    bool perf = false, perf_valid = false;    // omni_sp_set_perf: every pass records its stage events (omni_sp_last_stage_ms)
    // The image-independent band of the fisheye mask (fp16 and OMNI_PREC_SPLIT; OMNI_SP_MASK_SKIP=0 / OMNI_SP_MASK_SKIP_SPLIT=0 switch it off).  LoopCam blanks rows
    // [3H/4, 3H/4 + H/4) of every image before the network sees it (loop_cam.cpp:536-539).  Where those rows reach the bottom edge (H % 4 == 0), every
    // output pixel of a layer from row `a` down -- one row further per 3x3 convolution, halved by every pool -- has all its taps in blanked rows or in
    // the zero padding, over the WHOLE width: it holds the same bits whatever the image.  (Away from the edges it is one vector per layer; near the
    // side edges it varies with the column and near the bottom edge with the row, because padding is not that vector.)  The tile rows that lie in
    // that region -- the BAND, [band_ty0, tiles_y) x [0, tiles_x) -- are computed once by a pass over an all-zero image into image slot 0
    // (sp_calibrate_mask_skip) and copied into every other slot of the activation buffers; the persistent kernels then leave them out of their walk
    // (ConvArgs::skip_*).  Results are bit-identical to the dense pass (tests/test_gpu_mask_skip.py, tests/test_gpu_mask_band.py).  A pass without
    // the mask (or on another path) overwrites the band: the next masked pass calibrates again (skip_state, sp_mask_skip_step).
    // The RECTANGLE (ty0 .. tx1) is the part of the band where the output is that one vector: whole tiles one pixel per convolution away from
    // the bottom and side edges.  It is what omni_sp_mask_skip_plan reports, what conv1a's own band (OMNI_PREC_SPLIT, unfused) is filled by, what a
    // height with H % 4 != 0 (blanked rows that stop short of the bottom edge) still skips, and, under OMNI_SP_MASK_RECT=1, all that is skipped
    // (filled by broadcasting the vector: the A/B reference for the band).
    struct MaskSkip {
        int ty0 = 0, ty1 = 0, tx0 = 0, tx1 = 0;      // tile rectangle in the layer's conv-output tile grid (before the pool)
        int oy0 = 0, oy1 = 0, ox0 = 0, ox1 = 0;      // the same rectangle in the layer's output map (after the pool)
        int band_ty0 = 0, tiles_y = 0, tiles_x = 0;  // the band: tile rows [band_ty0, tiles_y) of the same grid, every tile column (none: band_ty0 == tiles_y)
        int band_oy0 = 0;                            // ... = rows [band_oy0, oh) of the output map
        int oh = 0, ow = 0, oc = 0;                  // output map: rows, cols, channels
        int pix_bytes = 0;                           // its layout: bytes per pixel, per row, per image, offset of pixel (0, 0) (fp16: NHWC; split: framed split-64)
        int64_t row_bytes = 0, img_bytes = 0, org_bytes = 0;
        void* vec = nullptr;                         // [pix_bytes]: the rectangle's constant (only where the rectangle is what gets filled)
        void** map = nullptr;                        // the activation buffer
        double frac = 0.0, band_frac = 0.0;          // the rectangle's / the band's share of the layer's tiles
    };
    MaskSkip mskip[6];                       // conv1a (OMNI_PREC_SPLIT, unfused, only: rectangle), conv1b (+pool), conv2a, conv2b (+pool), conv3a, conv3b (+pool)
    bool mask_band = false;                  // layers 1..5 leave out their band (false: their rectangle -- OMNI_SP_MASK_RECT=1, or H % 4 != 0)
    uint8_t* zero_gray = nullptr;            // the calibration's all-zero image (grows with the largest stride seen)
    size_t zero_gray_bytes = 0;
    omni_pcafit* pcafit = nullptr;           // omni_sp_set_pcafit: every pass adds its rows to this accumulator (borrowed; null: none)
    std::mutex mu;
};

namespace omni {

template <typename T>
static int dev_upload(omni_sp* s, T** dst, const void* src, size_t bytes) {
    hipStream_t st = s->ctx->stream;
    if (int rc = s->mem.alloc(dst, bytes)) return rc;
    OMNI_HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
    OMNI_HIP_TRY(hipStreamSynchronize(st));
    return OMNI_OK;
}

// Where every layer's output does not depend on the image under the fisheye mask: the band of whole tile rows, and the tile rectangle inside it where
// the output is one vector (see omni_sp::MaskSkip): pure integer arithmetic on (H, W) and the kernels' tile shapes; k[0] = conv1a (OMNI_PREC_SPLIT
// only), k[1..5] = conv1b, conv2a, conv2b, conv3a, conv3b
static void sp_mask_skip_rects(int H, int W, bool split, omni_sp::MaskSkip (&ks)[6]) {
    int m0, m1;
    omni_fisheye_mask_rows(H, 1, &m0, &m1);
    int h = H, w = W;
    for (auto& k : ks) k = omni_sp::MaskSkip{};
    // conv1a's output is relu(bias) on the rows whose three input rows are blanked (the zero padding below the image counts as blanked), in
    // every column (the padding left and right of the image is zeros too)
    int a = m0 + 1, b = (m1 == h) ? h - 1 : m1 - 2, c = 0, d = w - 1;
    if (split && b >= a) {                                 // conv1a_split: 8-row tile rows, the whole width
        omni_sp::MaskSkip& k = ks[0];
        k.ty0 = (a + 7) / 8; k.ty1 = (b + 1) / 8; k.tx0 = 0; k.tx1 = (w + 31) / 32;
        if (k.ty1 <= k.ty0) k.ty0 = k.ty1 = k.tx0 = k.tx1 = 0;
        k.oy0 = k.ty0 * 8; k.oy1 = k.ty1 * 8 < h ? k.ty1 * 8 : h; k.ox0 = 0; k.ox1 = k.ty1 > k.ty0 ? w : 0;
        k.oh = h; k.ow = w; k.oc = 64;
        k.frac = (double)(k.ty1 - k.ty0) / ((h + 7) / 8);
    }
    const bool pool[5] = {true, false, true, false, true};
    const int chans[5] = {64, 64, 64, 128, 128};
    static_assert(CONV_TW == 32, "tile width");
    const int TW = 32;
    const bool to_bottom = m1 == H;                        // the blanked rows reach the bottom edge: from row `a` down nothing depends on the image (H % 4 != 0: they stop short of it)
    bool rect = true;                                      // something is still constant
    for (int i = 0; i < 5; ++i) {                          // conv1b, conv2a, conv2b, conv3a, conv3b (cin = 128: the split kernel's 2 x 32 tiles, the fp16 register-stationary kernel's 6 x 32)
        const int TH = split ? (i == 4 ? 2 : 4) : (i == 4 ? conv_rs_pool_tile_rows() : CONV_TH);  // the kernels' output tiles (conv_split.hip: 4 x 32 / 2 x 32, conv.hip: CONV_TH x CONV_TW / RS_TH x RS_TW)
        a += 1; b -= 1; c += 1; d -= 1;                    // a 3x3 convolution (zero padding is NOT the constant): one pixel in from every side
        omni_sp::MaskSkip& k = ks[1 + i];
        const int f = pool[i] ? 2 : 1;
        // the band: rows [a, h) over the whole width (padding is as independent of the image as the blanked rows are), in whole tile rows
        k.tiles_y = (h + TH - 1) / TH; k.tiles_x = (w + TW - 1) / TW;
        k.band_ty0 = to_bottom ? std::min((a + TH - 1) / TH, k.tiles_y) : k.tiles_y;
        k.band_oy0 = k.band_ty0 * TH / f;
        k.band_frac = (double)(k.tiles_y - k.band_ty0) / k.tiles_y;
        rect = rect && b >= a && d >= c;                   // (false: nothing constant from here on)
        if (rect) {
            k.ty0 = (a + TH - 1) / TH; k.ty1 = (b + 1) / TH; k.tx0 = (c + TW - 1) / TW; k.tx1 = (d + 1) / TW;
            if (k.ty1 <= k.ty0 || k.tx1 <= k.tx0) k.ty0 = k.ty1 = k.tx0 = k.tx1 = 0;
            k.frac = (double)(k.ty1 - k.ty0) * (k.tx1 - k.tx0) / ((double)k.tiles_y * k.tiles_x);
            k.oy0 = k.ty0 * TH / f; k.oy1 = k.ty1 * TH / f; k.ox0 = k.tx0 * TW / f; k.ox1 = k.tx1 * TW / f;
        }
        if (pool[i]) { a = (a + 1) / 2; b = (b - 1) >> 1; c = (c + 1) / 2; d = (d - 1) >> 1; h /= 2; w /= 2; }      // pooled pixel r = conv pixels 2r, 2r + 1
        k.oh = h; k.ow = w; k.oc = chans[i];
    }
}

static int sp_plan_mask_skip(omni_sp* s) {
    s->facts.mask_skip = false;
    const bool split = s->precision == OMNI_PREC_SPLIT;
    if (s->facts.conv_variant != 0 || s->precision == OMNI_PREC_F32) return OMNI_OK;
    if (!s->cfg[split ? CFG_SP_MASK_SKIP_SPLIT : CFG_SP_MASK_SKIP]) return OMNI_OK;       // = 0: the dense pass (A/B, tests)
    sp_mask_skip_rects(s->H, s->W, split, s->mskip);
    // the band wherever the plan has one (a height whose blanked rows stop short of the bottom edge has none: its rectangles); OMNI_SP_MASK_RECT=1: the rectangles
    s->mask_band = false;
    for (int i = 1; i < 6 && !s->cfg[CFG_SP_MASK_RECT]; ++i) s->mask_band = s->mask_band || s->mskip[i].band_ty0 < s->mskip[i].tiles_y;
    void** maps[6] = {&s->a1a, &s->a1b, &s->a2a, &s->a2b, &s->a3a, &s->a3b};
    for (int i = 0; i < 6; ++i) {
        omni_sp::MaskSkip& k = s->mskip[i];
        k.map = maps[i];
        if (k.oc == 0) continue;
        if (split) {
            k.pix_bytes = k.oc * 4;
            k.row_bytes = (int64_t)split_frame_w(k.ow) * k.pix_bytes;
            k.img_bytes = (int64_t)split_frame_bytes(k.oh, k.ow, k.oc);
            k.org_bytes = k.row_bytes + k.pix_bytes;
        } else {
            k.pix_bytes = k.oc * 2; k.row_bytes = (int64_t)k.ow * k.pix_bytes; k.img_bytes = k.row_bytes * k.oh; k.org_bytes = 0;
        }
        if (s->mask_band && i > 0) {
            if (k.band_ty0 < k.tiles_y) s->facts.mask_skip = true;                   // (filled by a copy: no vector)
        } else if (k.ty1 > k.ty0) {
            if (int rc = s->mem.alloc(&k.vec, (size_t)k.pix_bytes * 4)) return rc;   // (x 4: conv2a as a Winograd layer keeps one vector per position in the 2 x 2 tile)
            s->facts.mask_skip = true;
        }
    }
    return OMNI_OK;
}

// what sp_plan_pass reads of the handle: the switches of config.h as they stand now (mask_skip: sp_plan_mask_skip, at the end of sp_init)
static void sp_set_facts(omni_sp* s) {
    SpHandleFacts& f = s->facts;
    f.precision = s->precision; f.H = s->H; f.W = s->W;
    f.conv_variant = s->cfg[CFG_CONV_V1];
    f.det16 = s->cfg[CFG_DET16] != 0;
    f.fused_cand = s->cfg[CFG_SP_FUSED_CAND] != 0;
    f.sparse_desc = s->cfg[CFG_SP_SPARSE_DESC] != 0;
    f.sparse_da = s->cfg[CFG_SP_SPARSE_DA] != 0;
    f.split_fuse1a = s->cfg[CFG_SPLIT_FUSE1A] != 0;
    f.split_db = s->cfg[CFG_SP_SPLIT_DB] != 0;
    f.wino = sp_wino_layers(s->precision, s->cfg[CFG_SPLIT_WINO], s->H, s->W, f.split_fuse1a);
}

static int sp_init(omni_sp* s, const omni_sp_weights* w, const float* pca_comp, const float* pca_mean) {
    hipStream_t st = s->ctx->stream;
    int rc;
    // biases, conv1a, convPb (fp32 always)
    for (int l = 0; l < OMNI_SP_NUM_LAYERS; ++l)
        if ((rc = dev_upload(s, &s->bias[l], w->bias[l], (size_t)kLayers[l].cout * 4))) return rc;
    if ((rc = dev_upload(s, &s->w1a, w->weight[L1A], 64 * 9 * 4))) return rc;
    {
        std::vector<float> t(256 * 65);
        for (int c = 0; c < 65; ++c)
            for (int k = 0; k < 256; ++k) t[(size_t)k * 65 + c] = w->weight[LPB][(size_t)c * 256 + k];
        if ((rc = dev_upload(s, &s->wPbT, t.data(), t.size() * 4))) return rc;
        std::vector<float> wa(16384), wdst(256);
        detector_pack_weights(t.data(), wa.data(), wdst.data());
        if ((rc = dev_upload(s, &s->wPbA, wa.data(), wa.size() * 4))) return rc;
        if ((rc = dev_upload(s, &s->wPbDust, wdst.data(), wdst.size() * 4))) return rc;
        std::vector<uint16_t> w16(2 * 2 * 16 * 64 * 8);
        detector_pack_weights16(t.data(), w16.data());
        if ((rc = dev_upload(s, &s->wPbA16, w16.data(), w16.size() * 2))) return rc;
    }
    {
        std::vector<float> bh(512);
        memcpy(bh.data(), w->bias[LPA], 256 * 4);
        memcpy(bh.data() + 256, w->bias[LDA], 256 * 4);
        if ((rc = dev_upload(s, &s->bias_heads, bh.data(), 512 * 4))) return rc;
    }
    {   // cv::Mat::convertTo(CV_32F, 1/255.0) (superpoint_tensorrt.cpp:127): OpenCV 3.4 scales 8-bit sources in float (cvt_32f): float(u8) * float(1/255.0)
        float lut[256];
        const volatile float alpha = (float)(1.0 / 255.0);                    // (volatile: one fp32 multiply, no contraction / folding in double)
        for (int i = 0; i < 256; ++i) lut[i] = (float)i * alpha;
        if ((rc = dev_upload(s, &s->lut, lut, sizeof(lut)))) return rc;
    }
    if (s->precision == OMNI_PREC_F16) {
        std::vector<uint16_t> db(65536);
        convdb_pack_weights(w->weight[LDB], db.data());
        if ((rc = dev_upload(s, &s->wDbFrag, db.data(), db.size() * 2))) return rc;
    }
    if (s->precision == OMNI_PREC_SPLIT && s->facts.split_db) {
        std::vector<uint16_t> hi(65536), lo(65536);
        convdb_pack_weights_split(w->weight[LDB], hi.data(), lo.data());
        if ((rc = dev_upload(s, &s->wDbFragHi, hi.data(), hi.size() * 2))) return rc;
        if ((rc = dev_upload(s, &s->wDbFragLo, lo.data(), lo.size() * 2))) return rc;
    }
    if (s->precision != OMNI_PREC_F32) {       // conv1a inside conv1b's kernel: its A fragments (OMNI_PREC_SPLIT: x the activation scale) and the u8 -> (hi, lo) table
        const bool split = s->precision == OMNI_PREC_SPLIT, from_bytes = !split && s->cfg[CFG_PP_U8];      // fp16: operands straight from the bytes, no table (lut_hl stays null)
        std::vector<uint16_t> fr(2048);
        (split ? conv1a_split_pack_fused : from_bytes ? conv1a_pack_u8_weights : conv1a_pack_split_weights)(w->weight[L1A], w->bias[L1A], fr.data());
        if ((rc = dev_upload(s, &s->w1a_frag, fr.data(), fr.size() * 2))) return rc;
        uint32_t lh[256];
        conv1a_make_split_lut(lh);
        if (!from_bytes && (rc = dev_upload(s, &s->lut_hl, lh, sizeof(lh)))) return rc;
    }
    // packed MFMA weights
    auto pack_upload = [&](int l, const float* w_oihw, int cin, int cout, int ks) -> int {
        const size_t n = conv_packed_elems(cin, cout, ks);
        if (s->precision == OMNI_PREC_SPLIT && ks == 3) {
            std::vector<uint16_t> p(n * 2);
            s->winv[l] = conv_pack_weights_split(w_oihw, cin, cout, p.data());
            return dev_upload(s, &s->wpk[l], p.data(), n * 4);
        }
        if (s->precision == OMNI_PREC_F16) {
            std::vector<__half> p(n);
            conv_pack_weights_f16(w_oihw, cin, cout, ks, p.data());
            return dev_upload(s, &s->wpk[l], p.data(), n * 2);
        }
        std::vector<float> p(n);
        conv_pack_weights_f32(w_oihw, cin, cout, ks, p.data());
        return dev_upload(s, &s->wpk[l], p.data(), n * 4);
    };
    for (int l : {L1B, L2A, L2B, L3A, L3B, L4A, L4B, LDB})
        if ((rc = pack_upload(l, w->weight[l], kLayers[l].cin, kLayers[l].cout, kLayers[l].ks))) return rc;
    {   // convPa | convDa fused along the output-channel axis: one N = 512 conv over the shared conv4b activations
        const size_t per = (size_t)256 * 128 * 9;
        std::vector<float> wh(per * 2);
        memcpy(wh.data(), w->weight[LPA], per * 4);
        memcpy(wh.data() + per, w->weight[LDA], per * 4);
        if ((rc = pack_upload(LPA, wh.data(), 128, 512, 3))) return rc;
    }
    if (s->precision == OMNI_PREC_SPLIT) {
        for (int l : {L1B, L2A, L2B, L3A}) {
            if (!(s->facts.wino & (l == L1B ? 1 : l == L2A ? 2 : l == L2B ? 4 : 8))) continue;
            const int co = kLayers[l].cout;
            std::vector<uint16_t> p((size_t)64 * co * 16 * 2);
            s->winv_w[l] = conv_pack_weights_wino(w->weight[l], 64, co, p.data());
            if ((rc = dev_upload(s, &s->wpk_w[l], p.data(), p.size() * 2))) return rc;
        }
    }
    if (s->precision == OMNI_PREC_SPLIT) {
        const float S = conv_split_act_scale();
        for (int l : {L1B, L2A, L2B, L3A, L3B, L4A, L4B}) {
            std::vector<float> b(kLayers[l].cout);
            for (int c = 0; c < kLayers[l].cout; ++c) b[c] = S * w->bias[l][c];
            if ((rc = dev_upload(s, &s->bias_s[l], b.data(), b.size() * 4))) return rc;
        }
    }
    if (pca_comp) {
        std::vector<float> t((size_t)256 * s->pca_dim);
        for (int j = 0; j < s->pca_dim; ++j)
            for (int c = 0; c < 256; ++c) t[(size_t)c * s->pca_dim + j] = pca_comp[(size_t)j * 256 + c];
        if ((rc = dev_upload(s, &s->pca_compT, t.data(), t.size() * 4))) return rc;
        if ((rc = dev_upload(s, &s->pca_mean, pca_mean, 256 * 4))) return rc;
    }
    // activations
    const size_t B = s->max_batch, H = s->H, W = s->W, e = s->esz;
    {
        // OMNI_PREC_SPLIT: every map in its zero frame (conv.h), zeroed here once
        struct Act { void** p; size_t h, w, c; };
        const Act acts[] = {{&s->a1a, H, W, 64},         {&s->a1b, H / 2, W / 2, 64},  {&s->a2a, H / 2, W / 2, 64},  {&s->a2b, H / 4, W / 4, 64},
                            {&s->a3a, H / 4, W / 4, 128}, {&s->a3b, H / 8, W / 8, 128}, {&s->a4a, H / 8, W / 8, 128}, {&s->a4b, H / 8, W / 8, 128}};
        for (const Act& a : acts) {
            const bool framed = s->precision == OMNI_PREC_SPLIT;
            if ((rc = s->mem.alloc(a.p, framed ? B * split_frame_bytes((int)a.h, (int)a.w, (int)a.c) : B * a.h * a.w * a.c * e, st, framed))) return rc;
        }
        OMNI_HIP_TRY(hipStreamSynchronize(st));
    }
    if ((rc = s->mem.alloc(&s->heads, B * (H / 8) * (W / 8) * 512 * e))) return rc;
    if (s->precision == OMNI_PREC_F16) {
        if ((rc = s->mem.alloc(&s->headsP, B * (H / 8) * (W / 8) * 256 * e))) return rc;
        if ((rc = s->mem.alloc(&s->da_compact, B * (size_t)s->max_num * 4 * 256 * 2))) return rc;
    }
    if (s->precision != OMNI_PREC_F16) {
        const size_t rows = ((B * (size_t)s->max_num * 4) + 7) & ~(size_t)7;
        if ((rc = s->mem.alloc(&s->cx32, rows * 256 * 4, st, true))) return rc;      // rows of key points that do not exist are never written (and never read back)
        if ((rc = s->mem.alloc(&s->cy32, rows * 256 * 4))) return rc;
        OMNI_HIP_TRY(hipStreamSynchronize(st));
    }
    if (s->precision == OMNI_PREC_SPLIT && (rc = s->mem.alloc(&s->headsP, B * (H / 8) * (W / 8) * 256 * 4))) return rc;     // cPa alone, fp32 (sparse convDa passes)
    if ((rc = s->mem.alloc(&s->draw, B * (H / 8) * (W / 8) * 256 * 4))) return rc;
    if ((rc = s->mem.alloc(&s->semi, B * H * W * 4))) return rc;
    if ((rc = s->mem.alloc(&s->gray_stage, B * H * W))) return rc;
    // post-processing buffers (the results zeroed once: the slots of key points that do not exist)
    const size_t hw = H * W, M = s->max_num;
    if ((rc = s->mem.alloc(&s->pb.cand, B * hw * 4))) return rc;
    if ((rc = s->mem.alloc(&s->pb.cand_masks, B * hw * 16))) return rc;
    if ((rc = s->mem.alloc(&s->pb.counters, B * 4 * 4))) return rc;
    if ((rc = s->mem.alloc(&s->pb.surv_keys, B * hw * 8))) return rc;
    if ((rc = s->mem.alloc(&s->pb.raw_desc, B * M * 256 * 4))) return rc;
    if ((rc = s->mem.alloc(&s->pb.norm_partial, B * 8 * 256 * 4))) return rc;
    if ((rc = s->mem.alloc(&s->pb.kps_xy, B * M * 2 * 4, st, true))) return rc;
    if ((rc = s->mem.alloc(&s->pb.scores, B * M * 4, st, true))) return rc;
    if ((rc = s->mem.alloc(&s->pb.n_kps, B * 4, st, true))) return rc;
    if ((rc = s->mem.alloc(&s->pb.desc_out, B * M * s->desc_dim * 4, st, true))) return rc;
    if ((rc = s->mem.alloc(&s->pb.cand_bits, B * (H / 8) * (W / 8) * 2 * 4))) return rc;
    s->pb.pca_compT = s->pca_compT;
    s->pb.pca_mean = s->pca_mean;
    for (int i = 0; i <= OMNI_SP_NUM_STAGES; ++i) OMNI_HIP_TRY(hipEventCreate(&s->ev[i]));
    OMNI_HIP_TRY(hipEventCreateWithFlags(&s->ev_convs, hipEventDisableTiming));
    OMNI_HIP_TRY(hipStreamSynchronize(st));
    return sp_plan_mask_skip(s);
}

// ---- one way to make a layer call ---------------------------------------------------------------------------------------------------------------
static int tails_prec(const SpPassPlan& p) { return p.tails_f32 ? OMNI_PREC_F32 : OMNI_PREC_F16; }     // the heads layer's output type: OMNI_PREC_SPLIT hands its tails fp32

enum SpKernelFamily { SP_K_DIRECT, SP_K_WINO };      // conv_mfma / conv_split and the kernels fused around them; conv_wino.hip
// The ConvArgs of layer l of this handle, for every call site.  Shape, pool and ReLU are the layer's (kLayers); cout = 256 runs the heads layer for
// cPa alone.  n_cu, zero_page and variant are set for every layer.  (The call sites used to differ in them; no difference was ever read: conv_mfma
// looks at the three for 3x3 layers only -- the 1x1 convDb runs the generic kernel whatever they say -- and conv_split, conv_wino and the fused
// conv1a + conv1b launchers read neither `variant` nor, conv1ab_fused apart, which needs it, `zero_page`.)
static ConvArgs sp_layer_args(const omni_sp* s, const SpPassPlan& p, int l, SpKernelFamily fam, const void* in, void* out, int batch, int cout = 0) {
    const LayerDef& d = kLayers[l];
    const bool split = s->precision == OMNI_PREC_SPLIT, wino = fam == SP_K_WINO;
    ConvArgs a;
    a.in = in; a.out = out; a.batch = batch; a.H = s->H / d.div; a.W = s->W / d.div; a.cin = d.cin; a.cout = cout ? cout : d.cout; a.ksize = d.ks;
    a.relu = l != LDB; a.pool = d.pool;
    a.out_f32 = l == LDB || (l == LPA && split);               // the descriptor map; OMNI_PREC_SPLIT: the heads layer's output, true values
    if (l == LDB) a.in_cstride = 512;                          // cDa: channels [256, 512) of the fused heads buffer
    a.w_packed = wino ? s->wpk_w[l] : s->wpk[l];
    a.split_inv = wino ? s->winv_w[l] : s->winv[l];            // (0 outside OMNI_PREC_SPLIT)
    a.bias = l == LPA ? s->bias_heads : (split && !a.out_f32) ? s->bias_s[l] : s->bias[l];       // the scaled bias goes with scaled (split-64 / raw-32) outputs
    a.n_cu = s->ctx->prop.multiProcessorCount; a.zero_page = s->ctx->zero_page; a.variant = s->facts.conv_variant;
    const int i = l == L1B ? 1 : l == L2A ? 2 : l == L2B ? 3 : l == L3A ? 4 : l == L3B ? 5 : -1;
    if (p.use_skip && i >= 0) {
        const omni_sp::MaskSkip& k = s->mskip[i];
        if (s->mask_band) { a.skip_ty0 = k.band_ty0; a.skip_ty1 = k.tiles_y; a.skip_tx0 = 0; a.skip_tx1 = k.tiles_x; }      // (full width down to the last tile row: tile_walk.h, bw = 0)
        else { a.skip_ty0 = k.ty0; a.skip_ty1 = k.ty1; a.skip_tx0 = k.tx0; a.skip_tx1 = k.tx1; }
    }
    return a;
}
// layer l on the precision's direct kernels (convDb: the tails' precision)
static int sp_conv(omni_sp* s, const SpPassPlan& p, int l, const void* in, void* out, int batch, int cout = 0) {
    const ConvArgs a = sp_layer_args(s, p, l, SP_K_DIRECT, in, out, batch, cout);
    if (l == LDB) return conv_mfma(s->ctx->stream, tails_prec(p), a);
    return s->precision == OMNI_PREC_SPLIT ? conv_split(s->ctx->stream, a) : conv_mfma(s->ctx->stream, s->precision, a);
}
// convPa | convDa fused over every cell into `heads`, or (cpa_only) convPa alone into headsP: the detector branch needs cPa everywhere, cDa (output
// channels 256-511 of the fused layer) is only read around the key points
static int sp_heads_layer(omni_sp* s, const SpPassPlan& p, int batch, bool cpa_only) {
    return sp_conv(s, p, LPA, s->a4b, cpa_only ? s->headsP : s->heads, batch, cpa_only ? 256 : 512);
}
static const void* sp_cda(const omni_sp* s) { return (const char*)s->heads + (size_t)256 * s->esz; }      // cDa inside `heads`: pixel stride 512
// the dense descriptor map, fp16: convDb + descriptor L2 norm in one HBM pass
static int sp_desc_dense_f16(omni_sp* s, int batch) {
    return convdb_l2norm(s->ctx->stream, s->ctx, sp_cda(s), 512, s->wDbFrag, s->bias[LDB], s->draw, (int64_t)batch * s->Hc * s->Wc);
}
// ... every other path: the generic 1x1 convolution, then the norm in place
static int sp_desc_dense_generic(omni_sp* s, const SpPassPlan& p, int batch) {
    if (int rc = sp_conv(s, p, LDB, sp_cda(s), s->draw, batch)) return rc;
    return l2norm_channels(s->ctx->stream, s->draw, (int64_t)batch * s->Hc * s->Wc);
}
// the operands of every descriptor tail that runs inside the post-processing; p.desc says which of them are read
static SpSparseDesc sp_sparse_desc(const omni_sp* s, const SpPassPlan& p) {
    SpSparseDesc sd;
    sd.mode = p.desc; sd.split_db = p.desc_split_db; sd.cand_fused = p.cand_fused;
    sd.ctx = s->ctx; sd.cda = sp_cda(s); sd.in_cstride = 512; sd.bias = s->bias[LDB];
    sd.wfrag = s->wDbFrag; sd.wdb_hi = s->wDbFragHi; sd.wdb_lo = s->wDbFragLo; sd.wdb_f32 = s->wpk[LDB];
    sd.a4b = s->a4b; sd.da_w = s->wpk[LPA]; sd.da_bias = s->bias_heads; sd.da_g32_first = 8; sd.da_inv = s->winv[LPA]; sd.da_compact = s->da_compact;
    sd.cx = s->cx32; sd.cy = s->cy32; sd.n_cu = s->ctx->prop.multiProcessorCount; sd.zero_page = s->ctx->zero_page;
    sd.pcafit = s->pcafit;
    return sd;
}

static int sp_forward(omni_sp* s, const uint8_t* gray_dev, int stride, int batch, int fisheye_mask, bool with_events, bool run_post, bool calibrating = false);
// One dense pass of one image, all zeros, with the mask on; then every planned layer's band -- the rows [band_oy0, oh) of its output map, one
// contiguous block in both layouts -- is copied from image slot 0 into every other slot of the layer's activation buffer.  Where the rectangle
// is what gets skipped (conv1a; every layer of a handle without bands) the layer's constant is read from the middle of its rectangle and written
// into that rectangle of every slot.  The pass starts zero_image_offset bytes into the zero image (sp_mask_skip_step: so that it takes the conv1a
// form of the pass it serves, conv1a's own rectangle (OMNI_PREC_SPLIT) is filled when that pass skips it, and the bands come from the same kernels).
static int sp_calibrate_mask_skip(omni_sp* s, int stride, int zero_image_offset) {
    hipStream_t st = s->ctx->stream;
    int rc;
    const size_t need = (size_t)stride * s->H + 4;
    if (s->zero_gray_bytes < need) {
        s->mem.release_one(s->zero_gray);
        s->zero_gray = nullptr; s->zero_gray_bytes = 0;
        if ((rc = s->mem.alloc(&s->zero_gray, need, st, true))) return rc;
        s->zero_gray_bytes = need;
    }
    if ((rc = sp_forward(s, s->zero_gray + zero_image_offset, stride, 1, 1, false, false, true))) return rc;
    const SpPassPlan& cal = s->last;       // the calibration pass's own plan
    for (const omni_sp::MaskSkip& k : s->mskip) {
        if (s->mask_band && k.map != &s->a1a) {
            if (k.band_ty0 >= k.tiles_y || k.band_oy0 >= k.oh) continue;
            // rows [band_oy0, oh) from the first pixel of the first to the last pixel of the last: nothing outside the map's own rows (split: the frame columns
            // between two rows are zeros in every slot)
            const int64_t first = k.org_bytes + k.band_oy0 * k.row_bytes, bytes = (k.oh - 1 - k.band_oy0) * k.row_bytes + (int64_t)k.ow * k.pix_bytes;
            if ((rc = conv_copy_slot0_bytes(st, *k.map, s->max_batch, k.img_bytes, first, bytes))) return rc;
            continue;
        }
        if (k.ty1 <= k.ty0 || (k.map == &s->a1a && cal.conv1a == SP_1A_FUSED)) continue;
        if ((k.map == &s->a2a && cal.conv2a.wino) || (k.map == &s->a3a && cal.conv3a.wino)) {     // an unpooled Winograd layer: constant per position in the 2 x 2 output tile
            if ((rc = conv_read_pixels2x2_bytes(st, *k.map, k.row_bytes, k.org_bytes, k.pix_bytes, ((k.oy0 + k.oy1) / 2) & ~1, ((k.ox0 + k.ox1) / 2) & ~1, k.vec))) return rc;
            if ((rc = conv_fill_rect2x2_bytes(st, *k.map, s->max_batch, k.img_bytes, k.row_bytes, k.org_bytes, k.pix_bytes, k.oy0, k.oy1, k.ox0, k.ox1, k.vec))) return rc;
            continue;
        }
        if ((rc = conv_read_pixel_bytes(st, *k.map, k.row_bytes, k.org_bytes, k.pix_bytes, (k.oy0 + k.oy1) / 2, (k.ox0 + k.ox1) / 2, k.vec))) return rc;
        if ((rc = conv_fill_rect_bytes(st, *k.map, s->max_batch, k.img_bytes, k.row_bytes, k.org_bytes, k.pix_bytes, k.oy0, k.oy1, k.ox0, k.ox1, k.vec))) return rc;
    }
    return OMNI_OK;
}

static SpPostParams post_params(const omni_sp* s) {
    SpPostParams p;
    p.width = s->W; p.height = s->H; p.thres = s->thres; p.max_num = s->max_num; p.dist_thresh = 4; p.pca_dim = s->pca_dim;
    return p;
}

// Enqueue the whole network + post-processing for `batch` HBM-resident images, as sp_plan_pass lays it out.  with_events records an event before
// every stage (profiling only).
static int sp_forward(omni_sp* s, const uint8_t* gray_dev, int stride, int batch, int fisheye_mask, bool with_events, bool run_post, bool calibrating) {
    hipStream_t st = s->ctx->stream;
    const int H = s->H, W = s->W, n_cu = s->ctx->prop.multiProcessorCount;
    int rc, stage = 0;
    if ((rc = s->ctx->ensure_zero_page())) return rc;
    SpPassInputs in;
    in.aligned4 = stride % 4 == 0 && ((uintptr_t)gray_dev & 3) == 0; in.fisheye_mask = fisheye_mask != 0; in.run_post = run_post; in.calibrating = calibrating;
    const SpPassPlan p = sp_plan_pass(s->facts, in);
    const SpMaskSkipStep step = sp_mask_skip_step(s->skip_state, p, stride);
    if (step.calibrate) {
        s->skip_state = SP_SKIP_STALE;
        if ((rc = sp_calibrate_mask_skip(s, stride, step.zero_image_offset))) return rc;
    }
    s->skip_state = step.after;
    s->last = p; s->last_batch = batch;
    auto mark = [&]() -> int { if (with_events) OMNI_HIP_TRY(hipEventRecord(s->ev[stage], st)); ++stage; return OMNI_OK; };
    if ((rc = mark())) return rc;
    switch (p.conv1a) {
        case SP_1A_FUSED: break;           // computed inside conv1b's kernel: the conv1a activation tensor is never materialised
        case SP_1A_SPLIT: rc = conv1a_split(st, gray_dev, stride, batch, H, W, fisheye_mask, s->w1a, s->bias[L1A], s->lut, s->a1a, p.use_skip ? s->mskip[0].ty0 : 0, p.use_skip ? s->mskip[0].ty1 : 0); break;
        case SP_1A_DIRECT: rc = conv1a_direct(st, s->precision, gray_dev, stride, batch, H, W, fisheye_mask, s->w1a, s->bias[L1A], s->lut, s->a1a); break;
    }
    if (rc || (rc = mark())) return rc;
    if (p.conv1b == SP_1B_CONV) rc = sp_conv(s, p, L1B, s->a1a, s->a1b, batch);
    else {
        const ConvArgs a = sp_layer_args(s, p, L1B, p.conv1b == SP_1B_FUSED_WINO ? SP_K_WINO : SP_K_DIRECT, nullptr, s->a1b, batch);
        if (p.conv1b == SP_1B_FUSED_WINO) rc = conv1ab_wino_fused(st, a, gray_dev, stride, fisheye_mask, s->w1a_frag, s->lut_hl, /*out_split=*/!p.raw_1b);
        else if (p.conv1b == SP_1B_FUSED_SPLIT) rc = conv1ab_split_fused(st, a, gray_dev, stride, fisheye_mask, s->w1a_frag, s->lut_hl);
        else rc = conv1ab_fused(st, a, gray_dev, stride, fisheye_mask, reinterpret_cast<const _Float16*>(s->w1a_frag), s->bias[L1A], s->lut_hl);
    }
    if (rc || (rc = mark())) return rc;
    // conv2a, conv2b, conv3a: the direct kernel, or a Winograd layer: raw-32 input (converted into a_tmp when the layer before it wrote split-64: mixed
    // configurations), raw-32 or split-64 output
    auto c64 = [&](int l, const SpC64Plan& c, const void* in, void* out) -> int {
        if (!c.wino) return sp_conv(s, p, l, in, out, batch);
        if (c.convert_in) {
            if (!s->a_tmp && (rc = s->mem.alloc(&s->a_tmp, (size_t)s->max_batch * split_frame_bytes(H / 2, W / 2, 64)))) return rc;
            if ((rc = split_to_raw32(st, in, s->a_tmp, batch, 64, H / kLayers[l].div, W / kLayers[l].div))) return rc;
            in = s->a_tmp;
        }
        return conv_wino(st, sp_layer_args(s, p, l, SP_K_WINO, in, out, batch), /*out_split=*/!c.out_raw32);
    };
    if ((rc = c64(L2A, p.conv2a, s->a1b, s->a2a)) || (rc = mark())) return rc;
    if ((rc = c64(L2B, p.conv2b, s->a2a, s->a2b)) || (rc = mark())) return rc;
    if ((rc = c64(L3A, p.conv3a, s->a2b, s->a3a)) || (rc = mark())) return rc;
    if ((rc = sp_conv(s, p, L3B, s->a3a, s->a3b, batch)) || (rc = mark())) return rc;
    if ((rc = sp_conv(s, p, L4A, s->a3b, s->a4a, batch)) || (rc = mark())) return rc;
    if ((rc = sp_conv(s, p, L4B, s->a4a, s->a4b, batch)) || (rc = mark())) return rc;
    if ((rc = sp_heads_layer(s, p, batch, p.heads_sparse_da)) || (rc = mark())) return rc;
    // the head thresholds its own output into the candidate lists when the post-processing follows (superpoint_tensorrt.cpp:167-173 inside the epilogue)
    DetCand dc;
    if (p.cand_fused) { dc.thres = s->thres; dc.bits = s->pb.cand_bits; }
    const void* cpa = p.heads_sparse_da ? s->headsP : s->heads;
    const int cpa_stride = p.heads_sparse_da ? 256 : 512, PH = tails_prec(p);
    switch (p.det) {
        case SP_DET_VALU: rc = detector_head(st, PH, cpa, cpa_stride, 0, batch, s->Hc, s->Wc, s->wPbT, s->bias[LPB], s->semi); break;
        // fp16: exact operands, split weights; split precision: the heads layer's fp32 output split on the fly as well (three terms: fp32-class logits)
        case SP_DET_MFMA16_F16: case SP_DET_MFMA16_F32:
            rc = detector_head_mfma16(st, PH, cpa, cpa_stride, 0, batch, s->Hc, s->Wc, s->wPbA16, s->wPbDust, s->bias[LPB], s->semi, n_cu, dc); break;
        case SP_DET_MFMA_F32: rc = detector_head_mfma(st, PH, cpa, cpa_stride, 0, batch, s->Hc, s->Wc, s->wPbA, s->wPbDust, s->bias[LPB], s->semi, n_cu, dc); break;
    }
    if (rc || (rc = mark())) return rc;
    OMNI_HIP_TRY(hipEventRecord(s->ev_convs, st));        // the convolution stack and the detector head are enqueued: what follows are small grids
    if (p.desc == SP_DESC_DENSE_F16) rc = sp_desc_dense_f16(s, batch);
    else if (p.desc == SP_DESC_DENSE_GENERIC) rc = sp_desc_dense_generic(s, p, batch);
    // (every other tail: convDb runs inside the post-processing, at the key points only)
    if (rc || (rc = mark())) return rc;
    if (p.run_post) {
        if ((rc = sp_postprocess(st, post_params(s), s->pb, s->semi, s->draw, batch, sp_sparse_desc(s, p)))) return rc;
        s->post_batch = batch;
    }
    return mark();
}

// the dense head activations and descriptor map of the LAST forward pass, when it sampled its descriptors sparsely: the fused heads layer over
// every cell (conv4b's output is still in HBM) + convDb + L2 norm.  fp16 runs the fused layer whatever the pass left in `heads`; fp32 / split only
// where the pass ran cPa alone
static int sp_make_dense(omni_sp* s) {
    SpPassPlan& p = s->last;
    int rc;
    if (!p.tails_f32 || !p.heads_full) {
        if ((rc = sp_heads_layer(s, p, s->last_batch, false))) return rc;
        p.heads_full = true;
    }
    if ((rc = p.tails_f32 ? sp_desc_dense_generic(s, p, s->last_batch) : sp_desc_dense_f16(s, s->last_batch))) return rc;
    p.dense_valid = true;
    return OMNI_OK;
}

static int sp_fetch_locked(omni_sp* s, int batch, float* kps_xy, int* n_kps, float* desc, float* scores) {
    hipStream_t st = s->ctx->stream;
    const size_t M = s->max_num, D = s->desc_dim;
    const size_t b_kps = (size_t)batch * M * 2 * 4, b_n = (size_t)batch * 4, b_desc = (size_t)batch * M * D * 4, b_sc = (size_t)batch * M * 4;
    int rc;
    if ((rc = s->hstage.ensure(b_kps + b_n + b_desc + b_sc))) return rc;
    char* h = s->hstage.as<char>();
    OMNI_HIP_TRY(hipMemcpyAsync(h, s->pb.kps_xy, b_kps, hipMemcpyDeviceToHost, st));
    OMNI_HIP_TRY(hipMemcpyAsync(h + b_kps, s->pb.n_kps, b_n, hipMemcpyDeviceToHost, st));
    OMNI_HIP_TRY(hipMemcpyAsync(h + b_kps + b_n, s->pb.desc_out, b_desc, hipMemcpyDeviceToHost, st));
    OMNI_HIP_TRY(hipMemcpyAsync(h + b_kps + b_n + b_desc, s->pb.scores, b_sc, hipMemcpyDeviceToHost, st));
    OMNI_HIP_TRY(hipStreamSynchronize(st));
    if (kps_xy) memcpy(kps_xy, h, b_kps);
    if (n_kps) memcpy(n_kps, h + b_kps, b_n);
    if (desc) memcpy(desc, h + b_kps + b_n, b_desc);
    if (scores) memcpy(scores, h + b_kps + b_n + b_desc, b_sc);
    return OMNI_OK;
}

void sp_drop_pcafit(omni_sp* s, omni_pcafit* f) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->pcafit == f) { s->pcafit = nullptr; (void)pcafit_set_owner(f, nullptr); }
}

static int upload_gray(omni_sp* s, const uint8_t* gray_host, int stride, int batch) {
    // pack rows to a dense [batch][H][W] device image (stride = W)
    const size_t n = (size_t)batch * s->H * s->W;
    int rc;
    if ((rc = s->hstage.ensure(n))) return rc;
    uint8_t* h = s->hstage.as<uint8_t>();
    for (int b = 0; b < batch; ++b)
        for (int y = 0; y < s->H; ++y)
            memcpy(h + ((size_t)b * s->H + y) * s->W, gray_host + ((size_t)b * s->H + y) * stride, s->W);
    OMNI_HIP_TRY(hipMemcpyAsync(s->gray_stage, h, n, hipMemcpyHostToDevice, s->ctx->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(s->ctx->stream));   // hstage is reused by fetch
    return OMNI_OK;
}

}  // namespace omni

extern "C" {

omni_sp* omni_sp_create(omni_ctx* ctx, const omni_sp_weights* w, const float* pca_comp, const float* pca_mean, int pca_dim,
                        int width, int height, float thres, int max_num, int precision, int max_batch) {
    if (!ctx || !w) { omni::set_error("null ctx/weights"); return nullptr; }
    for (int l = 0; l < OMNI_SP_NUM_LAYERS; ++l)
        if (!w->weight[l] || !w->bias[l]) { omni::set_error("weights for layer %s missing", kLayers[l].name); return nullptr; }
    if (width <= 0 || height <= 0 || width % 8 || height % 8) {
        omni::set_error("width=%d height=%d must be positive multiples of 8 (the reference asserts the engine size, superpoint_tensorrt.cpp:122)", width, height);
        return nullptr;
    }
    if (precision != OMNI_PREC_F32 && precision != OMNI_PREC_F16 && precision != OMNI_PREC_SPLIT) { omni::set_error("bad precision %d", precision); return nullptr; }
    if (max_num < 1 || max_num > 1024 || max_batch < 1 || max_batch > 256) { omni::set_error("max_num=%d (1..1024) / max_batch=%d (1..256) out of range", max_num, max_batch); return nullptr; }
    if (pca_comp && (!pca_mean || pca_dim < 1 || pca_dim > 256)) { omni::set_error("bad PCA arguments"); return nullptr; }
    if ((size_t)width * height / 16 * 4 + 16 > 160 * 1024) { omni::set_error("image %dx%d exceeds the in-LDS NMS plane", width, height); return nullptr; }
    (void)hipSetDevice(ctx->device);
    omni_sp* s = new omni_sp();
    s->ctx = ctx; s->W = width; s->H = height; s->Hc = height / 8; s->Wc = width / 8; s->thres = thres; s->max_num = max_num;
    s->max_batch = max_batch; s->precision = precision; s->esz = precision == OMNI_PREC_F16 ? 2 : 4;
    s->pca_dim = pca_comp ? pca_dim : 0; s->desc_dim = pca_comp ? pca_dim : 256;
    if (omni::config_resolve(&s->cfg) != OMNI_OK) { delete s; return nullptr; }
    omni::sp_set_facts(s);
#ifndef OMNI_TEST_VARIANTS
    if (s->facts.conv_variant != 0) {
        omni::set_error("OMNI_CONV_V1=%d: the reference variants of the fp16 convolutions are only built into the test library (omni-swarm_amd/lib_test/, make -C omni-swarm_amd test-variants)", s->facts.conv_variant);
        delete s;
        return nullptr;
    }
#endif
    if (omni::sp_init(s, w, pca_comp, pca_mean) != OMNI_OK) { omni_sp_destroy(s); return nullptr; }
    return s;
}

void omni_sp_destroy(omni_sp* s) {
    if (!s) return;
    if (s->pcafit) { (void)omni::pcafit_set_owner(s->pcafit, nullptr); s->pcafit = nullptr; }
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    s->mem.release_all();
    s->hstage.release(); s->dense_tmp.release();
    for (auto& e : s->ev) if (e) (void)hipEventDestroy(e);
    if (s->ev_convs) (void)hipEventDestroy(s->ev_convs);
    delete s;
}

int omni_sp_desc_dim(const omni_sp* s) { return s ? s->desc_dim : -1; }

int omni_sp_image_size(const omni_sp* s, int* width, int* height) {
    OMNI_REQUIRE(s, OMNI_ERR_INVALID, "null handle");
    if (width) *width = s->W;
    if (height) *height = s->H;
    return OMNI_OK;
}

int omni_sp_enqueue_dev(omni_sp* s, const uint8_t* gray_dev, int stride, int batch, int fisheye_mask) {
    omni::TraceRange trace_range("SuperPoint enqueue (convolutions + heads + post-processing)");
    OMNI_REQUIRE(s && gray_dev, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    OMNI_REQUIRE(stride >= s->W, OMNI_ERR_INVALID, "stride=%d < width=%d", stride, s->W);
    std::lock_guard<std::mutex> lk(s->mu);
    (void)hipSetDevice(s->ctx->device);
    s->perf_valid = s->perf;
    return omni::sp_forward(s, gray_dev, stride, batch, fisheye_mask, s->perf, true);
}

int omni_sp_fetch(omni_sp* s, int batch, float* kps_xy, int* n_kps, float* desc, float* scores) {
    OMNI_REQUIRE(s, OMNI_ERR_INVALID, "null handle");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    std::lock_guard<std::mutex> lk(s->mu);
    (void)hipSetDevice(s->ctx->device);
    return omni::sp_fetch_locked(s, batch, kps_xy, n_kps, desc, scores);
}

int omni_sp_infer(omni_sp* s, const uint8_t* gray_host, int stride, int batch, int fisheye_mask, float* kps_xy, int* n_kps,
                  float* desc, float* scores) {
    omni::TraceRange trace_range("SuperPoint inference (upload, network, post-processing, download)");
    OMNI_REQUIRE(s && gray_host && kps_xy && n_kps && desc, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    OMNI_REQUIRE(stride >= s->W, OMNI_ERR_INVALID, "stride=%d < width=%d", stride, s->W);
    std::lock_guard<std::mutex> lk(s->mu);
    (void)hipSetDevice(s->ctx->device);
    int rc;
    if ((rc = omni::upload_gray(s, gray_host, stride, batch))) return rc;
    s->perf_valid = s->perf;
    if ((rc = omni::sp_forward(s, s->gray_stage, s->W, batch, fisheye_mask, s->perf, true))) return rc;
    return omni::sp_fetch_locked(s, batch, kps_xy, n_kps, desc, scores);
}

int omni_sp_set_pcafit(omni_sp* s, omni_pcafit* fit) {
    OMNI_REQUIRE(s, OMNI_ERR_INVALID, "null handle");
    OMNI_REQUIRE(!fit || omni::pcafit_ctx(fit)->device == s->ctx->device, OMNI_ERR_INVALID, "the fit's context is on device %d, the handle's on device %d",
                 fit ? omni::pcafit_ctx(fit)->device : -1, s->ctx->device);
    // the accumulation runs on the pass's stream and the fit's readers wait for the fit's: one context, so one stream, and nothing to order
    OMNI_REQUIRE(!fit || omni::pcafit_ctx(fit) == s->ctx, OMNI_ERR_INVALID, "the fit belongs to another context than the handle: create it on the handle's context");
    std::lock_guard<std::mutex> lk(s->mu);
    if (fit == s->pcafit) return OMNI_OK;
    if (fit) { if (int rc = omni::pcafit_set_owner(fit, s)) return rc; }
    if (s->pcafit) (void)omni::pcafit_set_owner(s->pcafit, nullptr);
    s->pcafit = fit;
    return OMNI_OK;
}

int omni_sp_dev_outputs(omni_sp* s, const float** kps_xy_dev, const int** n_kps_dev, const float** desc_dev, const float** scores_dev) {
    OMNI_REQUIRE(s, OMNI_ERR_INVALID, "null handle");
    if (kps_xy_dev) *kps_xy_dev = s->pb.kps_xy;
    if (n_kps_dev) *n_kps_dev = s->pb.n_kps;
    if (desc_dev) *desc_dev = s->pb.desc_out;
    if (scores_dev) *scores_dev = s->pb.scores;
    return OMNI_OK;
}

int omni_sp_get_dense(omni_sp* s, int batch, float* semi_host, float* desc_host) {
    OMNI_REQUIRE(s, OMNI_ERR_INVALID, "null handle");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    std::lock_guard<std::mutex> lk(s->mu);
    (void)hipSetDevice(s->ctx->device);
    hipStream_t st = s->ctx->stream;
    int rc;
    if (semi_host) OMNI_HIP_TRY(hipMemcpyAsync(semi_host, s->semi, (size_t)batch * s->H * s->W * 4, hipMemcpyDeviceToHost, st));
    if (desc_host) {
        if (!s->last.dense_valid) {
            // the last forward pass sampled its descriptors without the dense map: produce it now from the head activations still in HBM
            OMNI_REQUIRE(batch <= s->last_batch, OMNI_ERR_INVALID, "no forward pass of >= %d images to take the dense descriptors from", batch);
            if ((rc = omni::sp_make_dense(s))) return rc;
        }
        const size_t n = (size_t)batch * 256 * s->Hc * s->Wc;
        if ((rc = s->dense_tmp.ensure(n * 4))) return rc;
        if ((rc = omni::nhwc_to_nchw(st, s->draw, s->dense_tmp.as<float>(), batch, 256, s->Hc * s->Wc))) return rc;
        OMNI_HIP_TRY(hipMemcpyAsync(desc_host, s->dense_tmp.p, n * 4, hipMemcpyDeviceToHost, st));
    }
    OMNI_HIP_TRY(hipStreamSynchronize(st));
    return OMNI_OK;
}

int omni_sp_postprocess_dense(omni_sp* s, const float* semi_host, const float* desc_host, int batch, float* kps_xy, int* n_kps,
                              float* desc, float* scores) {
    OMNI_REQUIRE(s && semi_host && desc_host, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    std::lock_guard<std::mutex> lk(s->mu);
    (void)hipSetDevice(s->ctx->device);
    hipStream_t st = s->ctx->stream;
    int rc;
    const size_t n = (size_t)batch * 256 * s->Hc * s->Wc;
    if ((rc = s->dense_tmp.ensure(n * 4))) return rc;
    OMNI_HIP_TRY(hipMemcpyAsync(s->semi, semi_host, (size_t)batch * s->H * s->W * 4, hipMemcpyHostToDevice, st));
    OMNI_HIP_TRY(hipMemcpyAsync(s->dense_tmp.p, desc_host, n * 4, hipMemcpyHostToDevice, st));
    if ((rc = omni::nchw_to_nhwc(st, s->dense_tmp.as<float>(), s->draw, batch, 256, s->Hc * s->Wc))) return rc;
    s->last.dense_valid = true; s->last_batch = batch;          // `draw` / `semi` now hold the caller's maps
    omni::SpSparseDesc sd;
    sd.cand_from_list = s->facts.fused_cand;       // threshold + window masks as the pipeline makes them (OMNI_SP_FUSED_CAND=0: sp_cand_kernel)
    if ((rc = omni::sp_postprocess(st, omni::post_params(s), s->pb, s->semi, s->draw, batch, sd))) return rc;
    s->post_batch = batch;
    return omni::sp_fetch_locked(s, batch, kps_xy, n_kps, desc, scores);
}

int omni_sp_debug_layer(omni_sp* s, const char* name, int batch, float* out_nchw_host, int* C, int* Hl, int* Wl) {
    OMNI_REQUIRE(s && name, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    struct Ent { const char* n; const void* p; int c, div, prec; };
    const bool rows_in = strcmp(name, "desc_rows_in") == 0;
    if (rows_in || strcmp(name, "desc_rows_out") == 0) {       // the sparse descriptor tail's compact rows as they lie: [batch][4 max_num][256] fp32
        OMNI_REQUIRE(s->cx32 && (s->last.desc == omni::SP_DESC_SPARSE_DA_SPLIT || s->last.desc == omni::SP_DESC_GATHER_F32) && batch <= s->last_batch,
                     OMNI_ERR_INVALID, "layer %s: the last pass of >= %d images left no compact descriptor rows", name, batch);
        if (C) *C = 4 * s->max_num;
        if (Hl) *Hl = 256;
        if (Wl) *Wl = 1;
        if (!out_nchw_host) return OMNI_OK;
        std::lock_guard<std::mutex> lk(s->mu);
        (void)hipSetDevice(s->ctx->device);
        OMNI_HIP_TRY(hipMemcpyAsync(out_nchw_host, rows_in ? s->cx32 : s->cy32, (size_t)batch * s->max_num * 4 * 256 * 4, hipMemcpyDeviceToHost, s->ctx->stream));
        OMNI_HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        return OMNI_OK;
    }
    const bool d_raw = strcmp(name, "desc_raw") == 0;
    if (d_raw || strcmp(name, "desc_norm_partial") == 0) {     // the descriptor tail's stage outputs as they lie: raw_desc [batch][max_num][256], norm_partial [batch][8][256] fp32
        std::lock_guard<std::mutex> lk(s->mu);
        OMNI_REQUIRE(batch <= s->post_batch, OMNI_ERR_INVALID, "layer %s: no post-processing pass of >= %d images to take it from", name, batch);
        const int rows = d_raw ? s->max_num : 8;
        if (C) *C = rows;
        if (Hl) *Hl = 256;
        if (Wl) *Wl = 1;
        if (!out_nchw_host) return OMNI_OK;
        (void)hipSetDevice(s->ctx->device);
        OMNI_HIP_TRY(hipMemcpyAsync(out_nchw_host, d_raw ? s->pb.raw_desc : s->pb.norm_partial, (size_t)batch * rows * 256 * 4, hipMemcpyDeviceToHost, s->ctx->stream));
        OMNI_HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        return OMNI_OK;
    }
    const int P = s->precision;
    const Ent tab[] = {{"conv1a", s->a1a, 64, 1, P},   {"conv1b", s->a1b, 64, 2, P},   {"conv2a", s->a2a, 64, 2, P},
                       {"conv2b", s->a2b, 64, 4, P},   {"conv3a", s->a3a, 128, 4, P},  {"conv3b", s->a3b, 128, 8, P},
                       {"conv4a", s->a4a, 128, 8, P},  {"conv4b", s->a4b, 128, 8, P},  {"heads", s->heads, 512, 8, P == OMNI_PREC_SPLIT ? OMNI_PREC_F32 : P},
                       {"desc", s->draw, 256, 8, OMNI_PREC_F32}};
    for (const Ent& e : tab) {
        if (strcmp(e.n, name) != 0) continue;
        if (e.p == s->a1a && s->last.conv1a == omni::SP_1A_FUSED) { omni::set_error("conv1a is fused into conv1b on this path and not materialised (OMNI_CONV_V1=3 keeps it)"); return OMNI_ERR_INVALID; }
        if ((e.p == s->heads || e.p == s->draw) && !s->last.dense_valid) {
            OMNI_REQUIRE(batch <= s->last_batch, OMNI_ERR_INVALID, "no forward pass of >= %d images to take layer %s from", batch, name);
            std::lock_guard<std::mutex> lk(s->mu);
            (void)hipSetDevice(s->ctx->device);
            int rc = omni::sp_make_dense(s);
            if (rc) return rc;
        }
        const int h = s->H / e.div, w = s->W / e.div;
        if (C) *C = e.c;
        if (Hl) *Hl = h;
        if (Wl) *Wl = w;
        if (!out_nchw_host) return OMNI_OK;
        std::lock_guard<std::mutex> lk(s->mu);
        (void)hipSetDevice(s->ctx->device);
        const size_t n = (size_t)batch * e.c * h * w;
        int rc;
        if ((rc = s->dense_tmp.ensure(n * 4))) return rc;
        if (e.prec == OMNI_PREC_SPLIT && ((e.p == s->a1b && s->last.raw_1b) || (e.p == s->a2a && s->last.conv2a.out_raw32) || (e.p == s->a2b && s->last.conv2b.out_raw32))) {      // a raw-32 frame between two Winograd layers
            if ((rc = omni::raw32_to_nchw_f32(s->ctx->stream, e.p, s->dense_tmp.as<float>(), batch, e.c, h, w))) return rc;
        } else if (e.prec == OMNI_PREC_SPLIT) { if ((rc = omni::split_to_nchw_f32(s->ctx->stream, e.p, s->dense_tmp.as<float>(), batch, e.c, h, w))) return rc; }
        else if ((rc = omni::nhwc_any_to_nchw_f32(s->ctx->stream, e.prec, e.p, s->dense_tmp.as<float>(), batch, e.c, h * w))) return rc;
        OMNI_HIP_TRY(hipMemcpyAsync(out_nchw_host, s->dense_tmp.p, n * 4, hipMemcpyDeviceToHost, s->ctx->stream));
        OMNI_HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        return OMNI_OK;
    }
    omni::set_error("unknown layer '%s'", name);
    return OMNI_ERR_INVALID;
}

int omni_sp_last_plan(const omni_sp* s) {
    if (!s) return -1;
    const omni::SpPassPlan& p = s->last;
    return (p.conv1b == omni::SP_1B_FUSED_WINO ? 1 : 0) | (p.conv2a.wino ? 2 : 0) | (p.conv2b.wino ? 4 : 0) | (p.conv3a.wino ? 8 : 0) | (p.conv1a == omni::SP_1A_FUSED ? 16 : 0)
         | (p.det == omni::SP_DET_MFMA16_F32 ? 32 : 0) | (p.desc_split_db ? 64 : 0)
         | (p.desc == omni::SP_DESC_SPARSE_DA_SPLIT || p.desc == omni::SP_DESC_GATHER_F32 ? 128 : 0);
}

// (internal, cam.hip) the event a pass records behind its convolution stack
hipEvent_t omni_sp_convs_event(omni_sp* s) { return s ? s->ev_convs : nullptr; }

const char* omni_sp_stage_name(int stage) { return (stage >= 0 && stage < OMNI_SP_NUM_STAGES) ? kStageNames[stage] : ""; }

double omni_sp_stage_flops(const omni_sp* s, int stage) {
    if (!s) return 0.0;
    const double H = s->H, W = s->W;
    auto c = [](double h, double w, double cin, double cout, double k) { return 2.0 * h * w * cin * cout * k * k; };
    switch (stage) {
        case ST_CONV1A: return c(H, W, 1, 64, 3);
        case ST_CONV1B: return c(H, W, 64, 64, 3);
        case ST_CONV2A: case ST_CONV2B: return c(H / 2, W / 2, 64, 64, 3);
        case ST_CONV3A: return c(H / 4, W / 4, 64, 128, 3);
        case ST_CONV3B: return c(H / 4, W / 4, 128, 128, 3);
        case ST_CONV4A: case ST_CONV4B: return c(H / 8, W / 8, 128, 128, 3);
        case ST_HEADS_A: return c(H / 8, W / 8, 128, 512, 3);
        case ST_DET_TAIL: return c(H / 8, W / 8, 256, 65, 1);
        case ST_DESC_TAIL: return c(H / 8, W / 8, 256, 256, 1);
        default: return 0.0;
    }
}

int omni_sp_mask_skip_plan(int width, int height, int precision, int layer, int* rect, double* frac) {
    OMNI_REQUIRE(width > 0 && height > 0 && layer >= 0 && layer < 6, OMNI_ERR_INVALID, "bad argument");
    omni_sp::MaskSkip ks[6];
    if (precision != OMNI_PREC_F32) omni::sp_mask_skip_rects(height, width, precision == OMNI_PREC_SPLIT, ks);
    if (rect) { rect[0] = ks[layer].ty0; rect[1] = ks[layer].ty1; rect[2] = ks[layer].tx0; rect[3] = ks[layer].tx1; }
    if (frac) *frac = ks[layer].ty1 > ks[layer].ty0 ? ks[layer].frac : 0.0;
    return OMNI_OK;
}

int omni_sp_mask_band_plan(int width, int height, int precision, int layer, int* ty0, int* tiles_y, double* frac) {
    OMNI_REQUIRE(width > 0 && height > 0 && layer >= 0 && layer < 6, OMNI_ERR_INVALID, "bad argument");
    omni_sp::MaskSkip ks[6];
    if (precision != OMNI_PREC_F32) omni::sp_mask_skip_rects(height, width, precision == OMNI_PREC_SPLIT, ks);
    if (ty0) *ty0 = ks[layer].band_ty0;
    if (tiles_y) *tiles_y = ks[layer].tiles_y;
    if (frac) *frac = ks[layer].band_ty0 < ks[layer].tiles_y ? ks[layer].band_frac : 0.0;
    return OMNI_OK;
}

double omni_sp_stage_tiles_left_out(const omni_sp* s, int stage) {
    if (!s || !s->facts.mask_skip) return 0.0;
    const int i = stage == ST_CONV1A ? 0 : stage == ST_CONV1B ? 1 : stage == ST_CONV2A ? 2 : stage == ST_CONV2B ? 3 : stage == ST_CONV3A ? 4 : stage == ST_CONV3B ? 5 : -1;
    return i < 0 ? 0.0 : (s->mask_band && i > 0) ? s->mskip[i].band_frac : s->mskip[i].frac;
}

// enable_perf of the reference's runners (superpoint_tensorrt.cpp:130-162 prints the engine time and the post-processing time of every call): with perf on, every
// pass records an event in front of each stage (a dozen hipEventRecord: microseconds of host time) and omni_sp_last_stage_ms returns the LAST pass's stage times
int64_t omni_sp_pack_constants(int which, const float* w, const float* bias, int cout, uint16_t* out, int64_t out_halfs, float* scale) {
    if (!w || !out || !scale) { omni::set_error("omni_sp_pack_constants: null argument"); return -2; }
    if (which == 0) {
        if (!bias || out_halfs < 2048) { omni::set_error("omni_sp_pack_constants: conv1a needs a bias and 2048 halfs"); return -2; }
        omni::conv1a_pack_u8_weights(w, bias, out);
        *scale = 1.f;
        return 2048;
    }
    if (which == 1) {
        const int64_t need = (int64_t)64 * cout * 32;
        if (cout < 64 || cout % 64 || out_halfs < need) { omni::set_error("omni_sp_pack_constants: cout %d, %lld halfs", cout, (long long)out_halfs); return -2; }
        *scale = omni::conv_pack_weights_wino(w, 64, cout, out);
        return need;
    }
    if (which == 2) {                                      // a direct split layer; cin (64 or 128) from the room offered: cin * cout * 9 * 2 halfs
        const int64_t per_cin = (int64_t)cout * 18;
        const int cin = cout >= 64 && cout % 64 == 0 && out_halfs % per_cin == 0 ? (int)(out_halfs / per_cin) : 0;
        if (cin != 64 && cin != 128) { omni::set_error("omni_sp_pack_constants: cout %d, %lld halfs", cout, (long long)out_halfs); return -2; }
        *scale = omni::conv_pack_weights_split(w, cin, cout, out);
        return out_halfs;
    }
    if (which == 3) {                                      // convDb [256][256]: the hi fragments, then the lo fragments
        if (out_halfs < 2 * 65536) { omni::set_error("omni_sp_pack_constants: convDb needs 131072 halfs"); return -2; }
        omni::convdb_pack_weights_split(w, out, out + 65536);
        *scale = 1.f;
        return 2 * 65536;
    }
    omni::set_error("omni_sp_pack_constants: which = %d", which);
    return -2;
}

int omni_sp_set_perf(omni_sp* s, int on) {
    OMNI_REQUIRE(s, OMNI_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(s->mu);
    s->perf = on != 0;
    if (!s->perf) s->perf_valid = false;
    return OMNI_OK;
}
int omni_sp_last_stage_ms(omni_sp* s, float* stage_ms) {
    OMNI_REQUIRE(s && stage_ms, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    OMNI_REQUIRE(s->perf_valid, OMNI_ERR_INVALID, "omni_sp_last_stage_ms: no pass was run with omni_sp_set_perf on");
    (void)hipSetDevice(s->ctx->device);
    OMNI_HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    for (int i = 0; i < OMNI_SP_NUM_STAGES; ++i) stage_ms[i] = 0.f;
    for (int i = 0; i < ST_COUNT; ++i) OMNI_HIP_TRY(hipEventElapsedTime(&stage_ms[i], s->ev[i], s->ev[i + 1]));
    return OMNI_OK;
}

int omni_sp_profile(omni_sp* s, const uint8_t* gray_dev, int stride, int batch, int reps, float* stage_ms) {
    const int prof_mask = s ? s->cfg[omni::CFG_SP_PROFILE_MASK] : 0;   // stage times with the fisheye mask on (as the key-frame pipeline runs)
    OMNI_REQUIRE(s && gray_dev && stage_ms && reps >= 1, OMNI_ERR_INVALID, "bad argument");
    OMNI_REQUIRE(batch >= 1 && batch <= s->max_batch, OMNI_ERR_CAPACITY, "batch=%d outside [1,%d]", batch, s->max_batch);
    std::lock_guard<std::mutex> lk(s->mu);
    (void)hipSetDevice(s->ctx->device);
    for (int i = 0; i < OMNI_SP_NUM_STAGES; ++i) stage_ms[i] = 0.f;
    // the MEDIAN over the repetitions: the first passes after an idle stretch run at a lower clock (their launches are 10-20 % longer in a kernel
    // trace of the same run); the median is the launch duration a kernel trace of the timed loop shows
    std::vector<float> all((size_t)reps * ST_COUNT);
    for (int r = 0; r < reps; ++r) {
        int rc = omni::sp_forward(s, gray_dev, stride, batch, prof_mask, true, true);
        if (rc) return rc;
        OMNI_HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        for (int i = 0; i < ST_COUNT; ++i) {
            float ms = 0.f;
            OMNI_HIP_TRY(hipEventElapsedTime(&ms, s->ev[i], s->ev[i + 1]));
            all[(size_t)i * reps + r] = ms;
        }
    }
    for (int i = 0; i < ST_COUNT; ++i) {
        float* v = all.data() + (size_t)i * reps;
        std::sort(v, v + reps);
        stage_ms[i] = (reps & 1) ? v[reps / 2] : 0.5f * (v[reps / 2 - 1] + v[reps / 2]);
    }
    return OMNI_OK;
}

}  // extern "C"
