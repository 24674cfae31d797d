// SuperPoint post-processing on the GPU (the reference does all of this on the CPU after a 5.8 MB D2H copy):
//   getKeyPoints          swarm_loop/src/superpoint_tensorrt.cpp:164-189
//   NMS2                  swarm_loop/src/superpoint_tensorrt.cpp:237-310
//   computeDescriptors    swarm_loop/src/superpoint_tensorrt.cpp:192-230
#pragma once
#include "common.h"
#include "sp_plan.h"

namespace omni {

struct SpPostParams {
    int width, height;      // image size (multiples of 8)
    float thres;            // prob > thres (strict)                      :167
    int max_num;            // keep at most max_num key points           :305
    int dist_thresh;        // NMS radius, 4                              :183
    int pca_dim;            // 0 = no PCA (desc_dim 256)
};

struct SpPostBuffers {      // all device pointers, sized for max_batch images
    uint32_t* cand_bits;    // [B][H/8 * W/8][2]   prob > thres as a bitmap: word (cell, hh) = rows 0-7 x columns 4 hh .. 4 hh + 3 of the 8 x 8 cell, bit i = (row i >> 2, column i & 3)
    int* cand;              // [B][H*W]            candidate pixel indices (unordered)
    uint64_t* cand_masks;   // [B][H*W][2]         per candidate: earlier / later higher-confidence window masks
    int* counters;          // [B][4]              n_cand, n_surv, n_iter, spare
    uint64_t* surv_keys;    // [B][H*W]            survivor keys (unordered)
    float* raw_desc;        // [B][max_num][256]   sampled descriptors (before the channel normalisation)
    float* norm_partial;    // [B][8][256]         per-channel sums of squares over key-point segments
    // results
    float* kps_xy;          // [B][max_num][2]
    float* scores;          // [B][max_num]
    int* n_kps;             // [B]
    float* desc_out;        // [B][max_num][desc_dim]
    // constants
    const float* pca_compT; // [256][pca_dim]  (pca_comp transposed, as superpoint_tensorrt.cpp:110)
    const float* pca_mean;  // [256]
};

// How sp_postprocess gets its descriptors: `mode` (the pass's descriptor tail, sp_plan.h) picks the path, the pointers are operands only.  The two
// dense modes sample the finished map desc_nhwc; the sparse ones run convDb + L2 norm only at the <= 4 * max_num coarse cells the sampler reads --
// bit-identical to the dense map + sp_sample_kernel (a 1x1 conv and the per-cell norm do not look at neighbours).
struct SpSparseDesc {
    SpDescTail mode = SP_DESC_DENSE_GENERIC;
    bool split_db = false;          // SP_DESC_SPARSE_DA_SPLIT: convdb_l2norm_split (false: the exact-f32 convolution + l2norm_channels)
    const omni_ctx* ctx = nullptr;
    const void* cda = nullptr;      // cDa inside the heads buffer (fp16 / fp32 NHWC, pixel stride in_cstride elements): SP_DESC_SPARSE_F16, SP_DESC_GATHER_F32
    int in_cstride = 0;
    const float* bias = nullptr;    // convDb's
    const void* wfrag = nullptr;    // convdb_pack_weights (fp16 modes)
    const void* wdb_f32 = nullptr;  // conv_pack_weights_f32 of convDb (the exact-f32 convolution)
    const void* wdb_hi = nullptr; const void* wdb_lo = nullptr;      // convdb_pack_weights_split
    // convDa itself only around the key points (conv_c128_sparse -> da_compact / conv_split_c128_sparse -> cx): a4b = conv4b's output (fp16 NHWC / split-64
    // frames), da_w / da_bias / da_inv = the fused heads layer's packed weights, bias and split_inv, of which convDa is the 32-channel groups from da_g32_first
    const void* a4b = nullptr; const void* da_w = nullptr; const float* da_bias = nullptr; int da_g32_first = 0; float da_inv = 0.f;
    void* da_compact = nullptr;     // [B][max_num][4][256] fp16
    float* cx = nullptr; float* cy = nullptr;       // fp32 modes: the cDa rows / their convDb + norm, [ceil8(batch * max_num * 4)][256] each
    int n_cu = 0; const void* zero_page = nullptr;
    // the detector head already thresholded the map (conv.h DetCand): SpPostBuffers::cand_bits is filled; sp_mask_kernel compacts it into the candidate
    // lists and makes the window masks of the candidates only -- sp_cand_kernel, which re-reads the whole heat map through LDS tiles, is not launched
    bool cand_fused = false;
    // a heat map that did not come from the head (omni_sp_postprocess_dense): the same two steps as separate kernels -- sp_thresh_kernel makes the bitmap,
    // sp_mask_kernel lists and masks -- so that every edge case of the post-processing tests runs through the kernel the pipeline uses
    bool cand_from_list = false;
    // omni_sp_set_pcafit: the pass's rows go into this accumulator behind sp_chan_sumsq_kernel (pca_fit.hip); null: nothing is launched
    omni_pcafit* pcafit = nullptr;
};

// semi: [B][H][W] f32 probability map; desc_nhwc: [B][H/8][W/8][256] f32 (channel-normalised coarse descriptors; read by the two dense modes only)
int sp_postprocess(hipStream_t stream, const SpPostParams& p, const SpPostBuffers& b, const float* semi,
                   const float* desc_nhwc, int batch, const SpSparseDesc& sparse = SpSparseDesc{});

// layout helpers between the reference's NCHW binding layout and the internal NHWC
int nchw_to_nhwc(hipStream_t stream, const float* in, float* out, int batch, int C, int HW);
int nhwc_to_nchw(hipStream_t stream, const float* in, float* out, int batch, int C, int HW);

}  // namespace omni
