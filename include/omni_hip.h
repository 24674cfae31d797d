/*
 * omni_hip.h -- C ABI of the MI355X-native (gfx950 / CDNA4) swarm_loop hot path.
 *
 * Drop-in boundary for HKUST-Aerial-Robotics/Omni-swarm's per-keyframe CNN frontend and
 * loop-closure matcher.  The reference has no FFI layer; the seam is four C++ call surfaces
 * used by LoopCam / LoopDetector.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root):
 *
 *   omni_sp_*      SuperPointTensorRT            swarm_loop/include/swarm_loop/superpoint_tensorrt.h:12-29
 *                                                swarm_loop/src/superpoint_tensorrt.cpp:91-230,237-310
 *                  (+ the TensorRT engine = the graph of swarm_loop/superpoint.ipynb:135-205,
 *                   + TensorRTInferenceGeneric   swarm_loop/src/tensorrt_generic.cpp:14-120)
 *   omni_vlad_*    MobileNetVLADTensorRT         swarm_loop/include/swarm_loop/mobilenetvlad_tensorrt.h:6-22
 *                                                swarm_loop/src/mobilenetvlad_tensorrt.cpp:4-14
 *   omni_index_*   faiss::IndexFlatIP            used at swarm_loop/src/loop_detector.cpp:166,169,213,232,291,842
 *   omni_bf_*      cv::BFMatcher(NORM_L2,true)   used at swarm_loop/src/loop_cam.cpp:147-150,
 *                                                        swarm_loop/src/loop_detector.cpp:564-567
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch/OpenCV types cross this boundary.
 *   - every function that can fail returns int: 0 = OMNI_OK, otherwise an OMNI_ERR_* code;
 *     omni_last_error() gives a thread-local message.  The reference aborts on failure
 *     (live asserts, NV_CUDA_CHECK -- SURVEY.md F13); this library never aborts.
 *   - "_dev" variants take pointers to HBM (hipMalloc'd or omni_dev_alloc'd) and are asynchronous on the
 *     context's stream; the plain variants take host pointers, copy, run and synchronise (the reference's
 *     blocking batch-1 semantics, tensorrt_generic.cpp:58-75).
 *   - handles are thread-compatible: calls on one handle are serialised internally by a mutex
 *     (the reference's LoopDetector is entered from two threads with no lock).
 *   - there is NO CPU fallback: if the HIP device or a kernel launch fails the call returns OMNI_ERR_HIP.
 */
#ifndef OMNI_HIP_H
#define OMNI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMNI_ABI_VERSION 2      /* 2: omni_cam_result gained n_images; omni_cam_set_active / omni_cam_ready */

enum {
    OMNI_OK = 0,
    OMNI_ERR_INVALID = 1,   /* bad argument / shape mismatch (the reference asserts, superpoint_tensorrt.cpp:122) */
    OMNI_ERR_HIP = 2,       /* HIP runtime / launch failure */
    OMNI_ERR_NOMEM = 3,
    OMNI_ERR_CAPACITY = 4   /* batch / k / row count beyond what the handle was created for */
};

enum { OMNI_PREC_F32 = 0,   /* exact-f32 MFMA (v_mfma_f32_32x32x2_f32), fp32 activations: the parity mode */
       OMNI_PREC_F16 = 1,   /* fp16 storage + v_mfma_f32_32x32x16_f16, fp32 accumulate: the reference's engines
                               are fp16 TensorRT (launch/realsense.launch:10-11) */
       OMNI_PREC_SPLIT = 2 }; /* omni_sp only: fp32-class on the fp16 matrix cores -- every operand of the 3x3 convolutions is a
                               (hi, lo) pair of halfs, three MFMA terms per product, heads in exact f32: meets north_star's
                               tolerance (key points identical to the fp32 graph, descriptors <= 1e-3) at ~1/3 of the fp16 rate */

enum { OMNI_STORE_F32 = 0, OMNI_STORE_F16 = 1 };   /* global-descriptor DB storage */

enum { OMNI_BF_OPENCV = 0,  /* cv::batchDistance(K=1, crosscheck=true) semantics (what the reference runs) */
       OMNI_BF_MUTUAL = 1 };/* strict mutual nearest neighbour (SURVEY.md 8c restatement) */

typedef struct omni_ctx omni_ctx;
typedef struct omni_sp omni_sp;
typedef struct omni_vlad omni_vlad;
typedef struct omni_index omni_index;
typedef struct omni_cam omni_cam;
typedef struct omni_shard omni_shard;
typedef struct omni_flatten omni_flatten;
typedef struct omni_resize omni_resize;

int         omni_abi_version(void);
const char* omni_last_error(void);
/* roctx ranges (OMNI_ROCTX=1; no-ops otherwise): the library brackets its own stages with them and the host loop its own through these two -- what the reference's
 * per-stage timers print (swarm_loop/src/superpoint_tensorrt.cpp:130-162, loop_cam.cpp:205-207) as a `rocprofv3 --marker-trace` timeline */
void        omni_trace_push(const char* name);
void        omni_trace_pop(void);

/* ---- configuration: EVERY switch of the library is an entry of one table (csrc/config.h): environment variable, default, valid range, class
 * (0 = variant: another kernel for the same results -- A/B measurements, bit-identity tests; 1 = tuning threshold; 2 = debug / timing ablation;
 * 3 = test fault injection; 4 = string), one line of documentation.  Handles resolve the table when they are created (a value outside its range
 * fails the creation); nothing else reads the environment.  The defaults ARE the production path (tests/test_config_cpu.py). */
int omni_config_count(void);
int omni_config_describe(int i, const char** env, int* def, int* lo, int* hi, int* cls, const char** doc);
/* what a handle created NOW would see for option `env` (defaults overridden by the current environment); OMNI_ERR_INVALID on an unknown name or
 * on any option holding a value outside its range */
int omni_config_value(const char* env, int* value);
/* 1: the option is read process-wide (frozen at first use: launch-site hooks, index thresholds), 0: snapshot per handle at creation */
int         omni_config_is_process_wide(int i);

/* ---- context: one per GPU/stream; owns a HIP stream, scratch and timers -------------------------------------
 * replaces TensorRTInferenceGeneric's cudaStreamCreate / cudaMalloc plumbing (tensorrt_generic.cpp:14-36,99-120) */
omni_ctx* omni_ctx_create(int device_id);
/* the same with the context's stream at the device's highest stream priority: for short, latency-bound work the host waits on (the detector's
 * searches) next to streams that keep every CU busy -- its kernels get the next free CUs instead of queueing behind whole launches */
omni_ctx* omni_ctx_create_priority(int device_id, int high_priority);
/* everything enqueued on `later`'s stream from now on runs after everything enqueued on `earlier`'s stream so far (an event on the device: the
 * host does not wait).  E.g. a network's stream behind the detector's, whose appends still read the network's output buffer. */
int       omni_ctx_order_after(omni_ctx* later, omni_ctx* earlier);
/* device -> PINNED host memory on the context's stream, without waiting: omni_ctx_sync() (or any later synchronising call) completes it */
int       omni_memcpy_d2h_async(omni_ctx* ctx, void* dst_pinned, const void* src, size_t bytes);
void      omni_ctx_destroy(omni_ctx* ctx);
int       omni_ctx_sync(omni_ctx* ctx);
void*     omni_ctx_stream(omni_ctx* ctx);                 /* hipStream_t, for callers that enqueue their own work */
int       omni_ctx_device_info(omni_ctx* ctx, char* name, int name_len, int* n_cu, int* clock_mhz, size_t* hbm_bytes);
/* Calibration (measurement support, no counterpart in the reference): v_mfma_f32_32x32x16_f16 back to back on every SIMD for about `ms` milliseconds;
 * returns what the board sustained (TFLOP/s) and the shader clock it held meanwhile -- bench.py quotes it next to the data-sheet peak. */
int       omni_ctx_mfma_ceiling(omni_ctx* ctx, float ms, float* tflops, float* sclk_ghz);

void* omni_dev_alloc(omni_ctx* ctx, size_t bytes);        /* HBM; NULL on failure */
int   omni_dev_free(omni_ctx* ctx, void* p);
void* omni_host_alloc(size_t bytes);                      /* pinned host memory (cudaMallocHost, tensorrt_generic.cpp:116-117); NULL on failure */
int   omni_host_free(void* p);
int   omni_memcpy_h2d(omni_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);  /* blocking */
int   omni_memcpy_d2h(omni_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);  /* blocking */
int   omni_timer_start(omni_ctx* ctx);                    /* hipEventRecord on the ctx stream */
int   omni_timer_stop(omni_ctx* ctx, float* ms);          /* records, synchronises, returns elapsed ms */

/* ---- SuperPoint -------------------------------------------------------------------------------------------------
 * weights: the 12 conv layers of superpoint.ipynb:143-160 in execution order
 *   conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa convDb,
 * each weight OIHW float32 and bias [O] float32 (the checkpoint's state_dict layout, superpoint.ipynb:270). */
#define OMNI_SP_NUM_LAYERS 12
typedef struct omni_sp_weights {
    const float* weight[OMNI_SP_NUM_LAYERS];
    const float* bias[OMNI_SP_NUM_LAYERS];
} omni_sp_weights;

/* SuperPointTensorRT::SuperPointTensorRT(engine, pca_comp, pca_mean, width, height, thres, max_num)
 * (superpoint_tensorrt.cpp:91-115).  pca_comp = sklearn components_ [pca_dim x 256] row-major, pca_mean [256]
 * (the two CSVs of :110-111); pca_comp == NULL disables PCA (#undef USE_PCA, :220-225) and desc is n x 256.
 * width, height must be multiples of 8.  max_batch = images processed per call (reference: 1). */
omni_sp* omni_sp_create(omni_ctx* ctx, const omni_sp_weights* w, const float* pca_comp, const float* pca_mean,
                        int pca_dim, int width, int height, float thres, int max_num, int precision, int max_batch);
void     omni_sp_destroy(omni_sp* sp);
int      omni_sp_desc_dim(const omni_sp* sp);              /* pca_dim, or 256 without PCA */
int      omni_sp_image_size(const omni_sp* sp, int* width, int* height);   /* the size the handle was created for (:122 asserts it per call) */

/* The rows the fisheye mask blanks in an image of `height` rows: [*row0, *row1) = cv::Rect(0, rows*3/4, cols, rows/4) of
 * LoopCam::extractor_img_desc_deepnet (loop_cam.cpp:536-539; integer divisions: a height that is not a multiple of 4 keeps its last rows).
 * fisheye_mask == 0: an empty range at the end of the image.  Every kernel that reads the gray image takes its mask rows from here. */
static inline void omni_fisheye_mask_rows(int height, int fisheye_mask, int* row0, int* row1) {
    *row0 = fisheye_mask ? height * 3 / 4 : height;
    *row1 = fisheye_mask ? height * 3 / 4 + height / 4 : height;
}

/* SuperPointTensorRT::inference(const cv::Mat&, std::vector<cv::Point2f>&, std::vector<float>&)
 * (superpoint_tensorrt.cpp:117-162) for `batch` images.
 *   gray      : batch images, u8, row stride `stride` bytes, image i at gray + i*stride*height
 *   fisheye_mask != 0 zeroes the rows omni_fisheye_mask_rows() names first (LoopCam::extractor_img_desc_deepnet, loop_cam.cpp:536-539)
 *   kps_xy    : [batch][max_num][2] float (x, y) integer-valued; order = (confidence desc, row-major index asc)
 *   n_kps     : [batch]
 *   desc      : [batch][max_num][desc_dim] float
 *   scores    : [batch][max_num] confidences, may be NULL */
int omni_sp_infer(omni_sp* sp, const uint8_t* gray_host, int stride, int batch, int fisheye_mask,
                  float* kps_xy, int* n_kps, float* desc, float* scores);
/* asynchronous, HBM-resident input; results stay in the handle's device buffers until fetched */
int omni_sp_enqueue_dev(omni_sp* sp, const uint8_t* gray_dev, int stride, int batch, int fisheye_mask);
int omni_sp_fetch(omni_sp* sp, int batch, float* kps_xy, int* n_kps, float* desc, float* scores);  /* D2H + sync */
/* device views of the last results: kps [max_batch][max_num][2] f32, n [max_batch] i32, desc [max_batch][max_num][dim] */
int omni_sp_dev_outputs(omni_sp* sp, const float** kps_xy_dev, const int** n_kps_dev, const float** desc_dev,
                        const float** scores_dev);
/* the engine's raw outputs in the reference's binding layout (tensorrt_generic.cpp:62-73):
 * semi [batch][H][W] f32 and desc [batch][256][H/8][W/8] f32 (NCHW).  For parity tests.  On the OMNI_PREC_F16 path a forward pass only
 * evaluates the descriptor head at the coarse cells around its key points (the key-point descriptors are bit-identical to sampling the
 * dense map); the dense `desc` is computed here, on demand, from the activations of the LAST forward pass (batch <= that pass's batch). */
int omni_sp_get_dense(omni_sp* sp, int batch, float* semi_host, float* desc_host);
/* run only the post-processing (getKeyPoints + NMS2 + computeDescriptors, superpoint_tensorrt.cpp:164-310) on
 * caller-supplied engine outputs in the layout above -- isolates the detector from conv rounding in tests */
int omni_sp_postprocess_dense(omni_sp* sp, const float* semi_host, const float* desc_host, int batch,
                              float* kps_xy, int* n_kps, float* desc, float* scores);
/* test hook: one intermediate activation of the last forward pass as NCHW float32 (name in {"conv1a","conv1b",...,
 * "conv4b","heads","desc"}; post-ReLU, post-pool where the layer pools).  out may be NULL to query the shape only.
 * "desc_rows_in" / "desc_rows_out" (fp32-class paths behind a pass that sampled its descriptors sparsely): the compact cDa rows around the key points and
 * their convDb + norm, as they lie: [batch][4 max_num][256] (C = 4 max_num, H = 256, W = 1); rows of key points that do not exist are not meaningful.
 * "desc_raw" / "desc_norm_partial" (after any pass that ran the post-processing -- infer, enqueue + fetch, postprocess_dense --, batch <= that pass's): the sampled
 * descriptors before the channel normalisation, [batch][max_num][256] (C = max_num, H = 256, W = 1; rows beyond an image's n_kps are not meaningful), and the
 * per-channel sums of their squares over the 8 key-point segments, [batch][8][256] (C = 8, H = 256, W = 1), as they lie.  Plain copies: nothing is launched or changed. */
int omni_sp_debug_layer(omni_sp* sp, const char* name, int batch, float* out_nchw_host, int* C, int* H, int* W);
/* test hook: the kernel forms of the last forward pass (csrc/sp_plan.h), as bits: 1, 2, 4, 8 = conv1b, conv2a, conv2b, conv3a ran the Winograd kernel; 16 = conv1a
 * was fused into conv1b; 32 = the split detector head (detector_head_mfma16 over fp32 input); 64 = the sparse descriptor tail ran convdb_l2norm_split; 128 = the
 * descriptors were sampled from compact fp32 rows ("desc_rows_in" / "desc_rows_out").  -1 for a null handle. */
int omni_sp_last_plan(const omni_sp* sp);
/* per-stage device time: runs the network `reps` times on HBM-resident input with HIP events between stages.
 * stage_ms [OMNI_SP_NUM_STAGES] MEDIAN ms per call over the repetitions; names via omni_sp_stage_name(). */
#define OMNI_SP_NUM_STAGES 16
int         omni_sp_profile(omni_sp* sp, const uint8_t* gray_dev, int stride, int batch, int reps, float* stage_ms);
/* enable_perf of the reference's runners (superpoint_tensorrt.cpp:130-162): with perf on every pass records its stage events; omni_sp_last_stage_ms waits for the
 * handle's stream and returns the LAST pass's device time per stage in milliseconds (stage_ms[OMNI_SP_NUM_STAGES], names: omni_sp_stage_name) */
int         omni_sp_set_perf(omni_sp* sp, int on);
int         omni_sp_last_stage_ms(omni_sp* sp, float* stage_ms);
const char* omni_sp_stage_name(int stage);
double      omni_sp_stage_flops(const omni_sp* sp, int stage);   /* algorithmic FLOP per image for that stage */
/* share of the stage's output tiles a fisheye-masked pass leaves out of the kernel's tile walk (the image-independent band of the mask, loop_cam.cpp:536-539:
 * computed once per handle over an all-zero image and copied into every image slot, bit-identical results); 0 when the stage computes every tile */
double      omni_sp_stage_tiles_left_out(const omni_sp* sp, int stage);
/* the band itself (pure arithmetic on the image size and the kernels' tile shapes; no device needed): layer 1..5 = conv1b, conv2a, conv2b, conv3a, conv3b (both
 * matrix-core precisions); the tile rows [*ty0, *tiles_y) of the layer's conv-output tile grid, over every tile column, hold the same bits whatever the image
 * (every tap of their receptive fields lies in the blanked rows or in the zero padding) and are left out; *ty0 == *tiles_y = no band (a height that is no
 * multiple of 4: the blanked rows stop short of the bottom edge; layer 0, conv1a: its rectangle below is a full-width band already); frac = its share of the tiles */
int         omni_sp_mask_band_plan(int width, int height, int precision, int layer, int* ty0, int* tiles_y, double* frac);
/* the rectangle inside the band where a layer's output is ONE constant vector (whole tiles one pixel per convolution away from the bottom and side edges, where
 * the zero padding is not that vector); what a masked pass left out before the band, and what OMNI_SP_MASK_RECT=1 still leaves out.  Pure arithmetic as above:
 * layer 0 = conv1a (OMNI_PREC_SPLIT only), 1..5 = conv1b, conv2a, conv2b, conv3a, conv3b (both matrix-core precisions); rect = {tile row 0, tile row 1, tile
 * column 0, tile column 1} of the layer's conv-output tile grid (empty = no such tile), frac = its share of the layer's tiles */
int         omni_sp_mask_skip_plan(int width, int height, int precision, int layer, int* rect, double* frac);

/* ---- MobileNetVLAD (ASSUMED architecture -- the reference ships only the I/O contract) --------- */
enum { OMNI_VLAD_CONV3X3_RELU6 = 0, OMNI_VLAD_PW_RELU6 = 1, OMNI_VLAD_DW3X3_RELU6 = 2,
       OMNI_VLAD_PW_LINEAR = 3, OMNI_VLAD_PW_LINEAR_RES = 4 };
typedef struct omni_vlad_layer {
    int kind, cin, cout, stride;
    const float* weight;   /* OIHW (depthwise: [C][1][3][3]) */
    const float* bias;
} omni_vlad_layer;
typedef struct omni_vlad_weights {
    int n_layers;
    const omni_vlad_layer* layers;
    int n_clusters, feat_dim, out_dim;
    const float* assign_w;   /* [K][D] */
    const float* assign_b;   /* [K] */
    const float* clusters;   /* [K][D] */
    const float* fc_w;       /* [out_dim][K*D] */
    const float* fc_b;       /* [out_dim] */
} omni_vlad_weights;

/* MobileNetVLADTensorRT(engine, width, height) (mobilenetvlad_tensorrt.h:10-19) */
omni_vlad* omni_vlad_create(omni_ctx* ctx, const omni_vlad_weights* w, int width, int height, int max_batch);
void       omni_vlad_destroy(omni_vlad* v);
/* OMNI_PREC_F32 (default): exact-f32 kernels, the parity mode.  OMNI_PREC_F16: the inverted-residual blocks run with fp16 matrix-core
 * operands and fp32 accumulation / residual stream -- the reference's engine is an fp16 TensorRT plan (launch/realsense.launch:10-11) */
int        omni_vlad_set_precision(omni_vlad* v, int precision);
/* test hook (host only, no device needed): the weight blob of one inverted-residual block as the split-fp16 matrix-core kernel reads it
 * (expand [hid][cin] + bias, depthwise [hid][9] + bias, projection [cout][hid], the layer table's OIHW order).  Returns the blob size in
 * bytes (out == NULL: size query), -1 when no kernel instantiation covers the shape, -2 on bad arguments.  Layout (vlad_s.hip): per 48-channel
 * chunk [10][48] fp32 depthwise taps + bias for all chunks, then per chunk the expand A fragments ([x_hi | x_lo | 1 1] pass with
 * We_hi, We_hi, be_hi, be_lo; x_hi pass with We_lo) and the projection A fragments (hi, lo per k-step), each fragment [64 lanes][8 halfs]. */
int64_t    omni_vlad_pack_block(int cin, int hid, int cout, int stride, const float* we, const float* be, const float* wd, const float* bd,
                                const float* wp, void* out, int64_t out_bytes);
/* Host-only test hooks (no GPU): the packed constants of two SuperPoint kernels, so that their algebra can be checked on the CPU.
 * which = 0: conv1a's matrix-core fragments for operands taken straight from the image bytes (csrc/conv.hip conv1a_pack_u8_weights): w [64][9],
 *   bias [64] -> out [2048] halfs, *scale = 1; which = 1: a cin = 64 layer's Winograd F(2x2,3x3) fragments (csrc/conv_wino.hip conv_pack_weights_wino):
 *   w OIHW [cout][64][3][3] -> out [64 * cout * 32] halfs, *scale = 2^-k of the packed values; which = 2: a direct split layer's fragments
 *   (csrc/conv_split.hip conv_pack_weights_split): w OIHW [cout][cin][3][3], cin = 64 or 128 taken from out_halfs = cin * cout * 18, *scale = 2^-k;
 *   which = 3: convDb's split fragments (csrc/conv.hip convdb_pack_weights_split): w [256][256] -> out [65536 hi | 65536 lo], *scale = 1.
 *   Returns the number of halfs written, -2 on bad arguments. */
int64_t omni_sp_pack_constants(int which, const float* w, const float* bias, int cout, uint16_t* out, int64_t out_halfs, float* scale);
/* std::vector<float> MobileNetVLADTensorRT::inference(const cv::Mat&) (mobilenetvlad_tensorrt.cpp:4-14):
 * u8 -> f32 with NO scaling feeds the net; out [batch][out_dim] */
int omni_vlad_infer(omni_vlad* v, const uint8_t* gray_host, int stride, int batch, int fisheye_mask, float* out);
int omni_vlad_enqueue_dev(omni_vlad* v, const uint8_t* gray_dev, int stride, int batch, int fisheye_mask);
int omni_vlad_fetch(omni_vlad* v, int batch, float* out);
int omni_vlad_dev_output(omni_vlad* v, const float** out_dev);
/* The layers (0 = stem + block 0, k = block k) whose tiles inside the constant region of the fisheye mask a masked pass leaves out (loop_cam.cpp:536-539
 * blanks the rows before netvlad_net.inference, :556-558): returns their number, frac[k] = the share of layer k's tiles left out (up to max_layers). */
int omni_vlad_mask_skip_layers(const omni_vlad* v, double* frac, int max_layers);
/* Test hooks: the activations of a pass, layer by layer (what omni_sp_debug_layer is to SuperPoint).  The three activation buffers of a handle rotate, so a
 * pass keeps no intermediate map unless asked to.  omni_vlad_debug_taps(v, 1): from now on a pass runs the same kernels with the same arguments and, behind the
 * stem (where it runs on its own) and behind every inverted-residual block, copies that layer's output on the device into a buffer of its own (allocated by the
 * first such pass); a layer that wrote into its mask-skip buffer is copied whole, rectangle included.  Off (the default): a pass enqueues nothing for it.
 * omni_vlad_debug_layer: one layer of the LAST pass as NCHW float32; name = "stem" (an error when the stem is fused into block 0), "b0" .. "b16" (the output
 * of that block, residual included; on the layer-by-layer path the output of its projection layer), "assign" (K x hf x wf), "vlad" (K * D x 1 x 1: the
 * intra- and L2-normalised vector the FC reads), "out" (out_dim x 1 x 1).  out may be NULL to query the shape only.  Errors (a code, no abort): the taps
 * are off, an unknown name, batch larger than the last tapped pass's. */
int omni_vlad_debug_taps(omni_vlad* v, int on);
int omni_vlad_debug_layer(omni_vlad* v, const char* name, int batch, float* out_nchw_host, int* C, int* H, int* W);
/* Which kernels the handle's current plan runs: paths[0] = the stem's form (OMNI_VLAD_STEM_*), paths[1 + k] = block k's kernel (OMNI_VB_*; OMNI_VB_NONE for
 * block 0 when the stem kernel computes it).  On the layer-by-layer path only paths[0] = OMNI_VLAD_STEM_LAYERS is returned.  Returns the number of entries
 * (up to max are written). */
enum { OMNI_VB_NONE = -1, OMNI_VB_HBLOCK = 0, OMNI_VB_SBLOCK = 1, OMNI_VB_MBLOCK = 2, OMNI_VB_PW_MFMA3 = 3, OMNI_VB_VALU = 4 };
enum { OMNI_VLAD_STEM_OWN = 0, OMNI_VLAD_STEM_WITH_B0 = 1, OMNI_VLAD_STEM_LAYERS = 2 };
int omni_vlad_block_paths(const omni_vlad* v, int* paths, int max);

/* ---- global-descriptor index: faiss::IndexFlatIP(d) --------------------------------------------------------- */
omni_index* omni_index_create(omni_ctx* ctx, int dim, int storage, int64_t initial_capacity_rows);
void        omni_index_destroy(omni_index* idx);
int         omni_index_add(omni_index* idx, int64_t n, const float* x_host);       /* IndexFlatIP::add(n, x) */
int         omni_index_add_dev(omni_index* idx, int64_t n, const float* x_dev);
int64_t     omni_index_ntotal(const omni_index* idx);                              /* .ntotal */
int         omni_index_dim(const omni_index* idx);                                 /* .d */
int         omni_index_reset(omni_index* idx);
/* drop the rows appended last so that ntotal == n_rows again (undo of appends enqueued ahead by a batched caller that failed) */
int         omni_index_truncate(omni_index* idx, int64_t n_rows);
/* OMNI_STORE_F32 shards keep an fp16 mirror of their rows (+50 % HBM; OMNI_INDEX_MIRROR=0 disables it): a batch of >= 4 queries is scored
 * against the mirror in one matrix-core pass, the best k+24 candidates per query are re-scored exactly against the fp32 rows, and a per-query
 * certificate proves the result is the exact fp32 top-k (scores bit-identical to the single-query path); uncertified queries are re-run with
 * the exact scan (so are all queries over rows fp16 cannot hold, norm >= 6e4, and a query whose largest element lies outside [1e-15, 1e15]).  Counters since creation: queries answered through the mirror / of those, the ones that needed the exact re-run. */
int         omni_index_cert_stats(omni_index* idx, int64_t* searches, int64_t* fallbacks);
/* IndexFlatIP::search(nq, q, k, D, I): exact inner product, k best descending, ties -> lower row id,
 * missing results padded with I = -1, D = -FLT_MAX.  k <= 1024 (the reference caps at 1000, loop_detector.cpp:200). */
int         omni_index_search(omni_index* idx, int nq, const float* q_host, int k, float* D, int64_t* I);
int         omni_index_search_dev(omni_index* idx, int nq, const float* q_dev, int k, float* D_dev, int64_t* I_dev);
/* search_dev restricted to the first n_limit local rows (the index as it was when it held n_limit rows).  Lets a caller enqueue
 * "add, query, add, query, ..." for several key frames -- LoopDetector::on_image_recv adds a frame's rows BEFORE querying
 * (loop_detector.cpp:89-98) -- on the stream without a host synchronisation in between: all adds first, then every query with the
 * ntotal it would have seen.  An empty prefix (n_limit == 0) fills the outputs with I = -1, D = -FLT_MAX. */
int         omni_index_search_prefix_dev(omni_index* idx, int nq, const float* q_dev, int k, int64_t n_limit, float* D_dev,
                                         int64_t* I_dev);
/* Several prefix searches in ONE pass over the shard (a micro-batch of key frames: every frame's query must see exactly the rows that
 * were in the index at its turn, loop_detector.cpp:89-98, but the rows are read from HBM once for all of them).  Query q is row
 * row_idx[q] of rows_dev (row_idx == NULL: rows 0..nq-1) and sees local rows [0, n_limits[q]) only; row_idx / n_limits are HOST arrays
 * read before the call returns.  nq <= 64.  Results as nq independent omni_index_search_prefix_dev calls would give them.
 * Ordering: rows_dev must be complete with respect to the index context's stream (e.g. the producer was waited for, or it ran on that
 * stream); the same holds for omni_index_add_dev / omni_index_search*_dev. */
int         omni_index_search_batch_prefix_dev(omni_index* idx, int nq, const float* rows_dev, const int64_t* row_idx, int k,
                                               const int64_t* n_limits, float* D_dev, int64_t* I_dev);
/* row sharding across GPUs: this handle holds rows g with g % world == rank at local slot g / world;
 * search then reports GLOBAL ids (local * world + rank).  Default rank 0, world 1. */
int         omni_index_set_shard(omni_index* idx, int rank, int world);   /* (an fp32 shard gives up its fp16 mirror: its batched searches must not wait on the host) */
/* host-side merge of per-shard top-k lists (after the all-gather): lists [n_lists][nq][k_each] -> [nq][k_out],
 * same ordering rule (score desc, id asc), entries with I < 0 ignored */
int         omni_topk_merge(int n_lists, int nq, int k_each, const float* D_lists, const int64_t* I_lists,
                            int k_out, float* D, int64_t* I);
/* Shard checkpoint (new -- the reference keeps its database in RAM only and loses it on restart):
 * "OMNX1" file = header {magic, dim, storage, ntotal} + the raw row matrix as stored (fp32 or fp16), streamed through a pinned
 * staging buffer.  load() replaces the handle's contents; dim and storage must match the handle. */
int         omni_index_save(omni_index* idx, const char* path);
int         omni_index_load(omni_index* idx, const char* path);
/* Test hook: ONE named scan kernel over local rows [0, n) (1 <= n <= ntotal), every raw 64-bit key back on the host -- keys_host [nq][n], undecoded
 * (csrc/common.h omni_make_key: high word = the order-preserving map of the fp32 score, low word = 0xFFFFFFFF - row; 0 = the empty key of a row at or beyond
 * its query's limit).  What a search shows of a scan is the best k of its scores; this shows all of them.  The kernel is launched by the search's own launch
 * functions with the search's grid and arguments; `which`:
 *   OMNI_SCAN_F32        ip_scan_kernel<float, nq>          fp32 rows, nq <= 8 (and nq x dim x 4 <= 128 KB, the search's query block)
 *   OMNI_SCAN_F32_ROWS   ip_scan_rows_kernel<nq, 4>         fp32 rows, 4 <= nq <= 8
 *   OMNI_SCAN_T16        ip_scan_t16_kernel<nq>             fp16 rows, nq <= 8
 *   OMNI_SCAN_MQ         mq_prep_kernel + ip_scan_mq_kernel fp16 rows, nq <= 64
 *   OMNI_SCAN_MQ_MIRROR  the same over an fp32 shard's fp16 mirror (the first pass of its batched search), nq <= 64
 * limits (host, [nq], or NULL): query q sees rows [0, limits[q]).  rotate: the matrix-core kernel's k-slice rotation (what OMNI_MQ_ROT sets for a search), 0 / 1.
 * OMNI_ERR_INVALID for a `which` that does not fit the handle's storage or nq.  Takes the handle's lock; uses buffers of its own: omni_index_cert_stats,
 * omni_index_last_scan_ms and the results of other searches are as they were without the call. */
enum { OMNI_SCAN_F32 = 0, OMNI_SCAN_F32_ROWS = 1, OMNI_SCAN_T16 = 2, OMNI_SCAN_MQ = 3, OMNI_SCAN_MQ_MIRROR = 4 };
int         omni_index_debug_scan(omni_index* idx, int which, int nq, const float* q_host, int64_t n, const int64_t* limits, int rotate,
                                  uint64_t* keys_host);
/* device time of the dominant scan kernel for the last search on this handle (HIP events on the ctx stream) */
int         omni_index_last_scan_ms(omni_index* idx, float* ms);

/* ---- the database row-sharded over the GPUs of one node: one process per GPU, RCCL over xGMI (new: the reference is single-GPU;
 * SURVEY.md 8e, BASELINE configs[3]/[4]).  Global row g lives on rank g % world at local slot g / world; every rank ends up with the
 * faiss::IndexFlatIP::search result of the UNSHARDED index (global ids, score desc, ties -> lower id).  RCCL is resolved at run time
 * (dlopen librccl.so.1); the launcher only has to carry the 128-byte unique id from rank 0 to the other ranks (any channel). */
#define OMNI_SHARD_ID_BYTES 128
/* the file the collective entry points (ncclAllGather ...) were resolved from: librccl of the process's ROCm stack, or what OMNI_RCCL_LIB names */
int         omni_shard_library_path(char* out, int cap);
int         omni_shard_unique_id(char* id_out /* [OMNI_SHARD_ID_BYTES], ncclGetUniqueId */);
/* collective: every rank calls it with the same id; `local` must be an empty index on ctx; its rows/ids are managed by the shard from here on */
omni_shard* omni_shard_create(omni_ctx* ctx, omni_index* local, int dim, int rank, int world, const char* unique_id);
void        omni_shard_destroy(omni_shard* s);
int64_t     omni_shard_ntotal(const omni_shard* s);                       /* GLOBAL row count */
int         omni_shard_preload_local(omni_shard* s, const float* rows_host, int64_t n_local, int64_t ntotal_global);
/* collective: F consecutive key-frame steps of every rank as ONE exchange unit.  rows_dev [F][m][dim] (HBM): this rank's m new rows of each
 * of its next F key frames.  Step f's rows of all ranks get the global ids ntotal + (f*world + r)*m + j; rank r's query of step f is its row
 * query_row of that step and sees exactly the rows up to and including step f (add before query, loop_detector.cpp:89-98).  Two
 * ncclAllGather (rows; per-shard top-k), one pass over the shard, one D2H; D_host / I_host [F][k] = this rank's merged results. */
int         omni_shard_step_batch_dev(omni_shard* s, int F, int m, const float* rows_dev, int query_row, int k, float* D_host, int64_t* I_host);
/* the same in two halves: _enqueue puts the whole unit -- both collectives, the scan, the copy of the lists to the host -- on the shard's stream
 * WITHOUT waiting (the caller goes on enqueuing CNN work); _rows_consumed blocks until rows_dev has been gathered and may be overwritten;
 * _wait blocks on the unit's completion event, merges this rank's results and moves the global row count.  One unit in flight at a time. */
int         omni_shard_step_enqueue(omni_shard* s, int F, int m, const float* rows_dev, int query_row, int k);
int         omni_shard_rows_consumed(omni_shard* s);
int         omni_shard_step_wait(omni_shard* s, float* D_host, int64_t* I_host);
/* device time (HIP events on the shard's stream, microseconds) of the two collectives of the exchange omni_shard_step_wait collected last: the all-gather
 * of every rank's new rows and the all-gather of the per-shard top-k lists (the one exchange step of the path) */
int         omni_shard_last_exchange_us(omni_shard* s, float* rows_gather_us, float* topk_gather_us);
/* collective: the same nq <= 64 queries on every rank -> the unsharded index's top-k on every rank */
int         omni_shard_search(omni_shard* s, int nq, const float* q_host, int k, float* D, int64_t* I);

/* ---- local-descriptor matcher: cv::BFMatcher(cv::NORM_L2, crossCheck=true).match(query, train, matches) -----
 * out arrays sized >= nq; matches ordered by query index; *n_matches = count.  dim <= 256. */
int omni_bf_match(omni_ctx* ctx, const float* q_host, int nq, const float* t_host, int nt, int dim, int mode,
                  int* q_idx, int* t_idx, float* dist, int* n_matches);
/* several pairs from host pointers in ONE upload / launch pair / download (the geometric verification matches up to four direction pairs per
 * loop candidate, loop_detector.cpp:431-537): outputs [n_pairs][max_n], n_matches [n_pairs]; nq[p], nt[p] <= max_n; n_pairs <= 64. */
int omni_bf_match_multi(omni_ctx* ctx, int n_pairs, const float* const* q_host, const int* nq, const float* const* t_host, const int* nt, int dim,
                        int mode, int max_n, int* q_idx, int* t_idx, float* dist, int* n_matches);
/* batched, HBM-resident: pair p uses q = q_dev + p*q_stride (floats), nq = nq_dev[p], likewise t.
 * outputs (device): q_idx/t_idx/dist [n_pairs][max_n], n_matches [n_pairs]. */
int omni_bf_match_batched_dev(omni_ctx* ctx, int n_pairs, int max_n, int dim, int mode,
                              const float* q_dev, int64_t q_stride, const int* nq_dev,
                              const float* t_dev, int64_t t_stride, const int* nt_dev,
                              int* q_idx_dev, int* t_idx_dev, float* dist_dev, int* n_matches_dev);

/* ---- fisheye flattening: FisheyeUndist::undist_all_cuda = cv::cuda::remap(INTER_LINEAR) per virtual pinhole view
 * (swarm_localization/test/fisheye_undist.hpp:57-90; VINS-Fisheye runs that class in front of swarm_loop).
 * map_xy[v] = the view's undistortion map [view_h][view_w][2] float (source x, y per output pixel: genOneUndistMap, :188-215; made on the host,
 * host/fisheye_flatten.hpp).  One launch remaps `batch` fisheye images into all views; image b's views are written back to back at
 * out_dev + b * omni_flatten_out_bytes(): view v at its running offset, rows packed -- ready for omni_sp_enqueue_dev / omni_cam_enqueue_dev.
 * Bilinear taps as cv::cuda's LinearFilter, border constant 0, round half to even. */
omni_flatten* omni_flatten_create(omni_ctx* ctx, int src_width, int src_height, int n_views, const int* view_w, const int* view_h,
                                  const float* const* map_xy);
void          omni_flatten_destroy(omni_flatten* f);
int64_t       omni_flatten_out_bytes(const omni_flatten* f);       /* bytes of all views of ONE source image */
int           omni_flatten_enqueue_dev(omni_flatten* f, const uint8_t* src_dev, int src_stride, int batch, uint8_t* out_dev);   /* asynchronous */

/* ---- camera-size frames -> network-size images: the cv::resize(input, _input, cv::Size(width, height)) of both reference engines (superpoint_tensorrt.cpp:123-125,
 * mobilenetvlad_tensorrt.cpp:6-8; INTER_LINEAR on CV_8UC1), on the GPU.  The arithmetic is a fixed integer spec restated from OpenCV 3.4's own resize
 * (csrc/resize_plan.h; OpenCV is un-vendored: parity unpinned): equal sizes copy, an exact 2x reduction on both axes is the rounded 2 x 2 mean (OpenCV's switch to
 * INTER_AREA), anything else two-tap linear with 11-bit coefficients.  The object holds the tables of ONE source size -> destination size in HBM.  Source at
 * least 2 wide, destination width a multiple of 4 (there is no tail path; the networks take multiples of 8), every side <= 32768.
 * omni_resize_enqueue_dev: `batch` frames (u8, src_stride, frame i at + i * src_stride * src_height) -> images of dst_width x dst_height written back to back,
 * rows packed, at out_dev (4-byte aligned) -- ready for omni_sp_enqueue_dev / omni_cam_enqueue_dev.  Asynchronous on the object's context. */
omni_resize* omni_resize_create(omni_ctx* ctx, int src_width, int src_height, int dst_width, int dst_height);
void         omni_resize_destroy(omni_resize* r);
int          omni_resize_mode(const omni_resize* r);              /* 0 copy, 1 area 2x, 2 linear; -1 for NULL */
int          omni_resize_enqueue_dev(omni_resize* r, const uint8_t* src_dev, int src_stride, int batch, uint8_t* out_dev);

/* ---- key-frame frontend: the device work of LoopCam::on_flattened_images (swarm_loop/src/loop_cam.cpp:178-229;
 * generate_stereo_image_descriptor :341-523, extractor_img_desc_deepnet :525-585, match_HFNet_local_features :141-174)
 * as one asynchronous unit: SuperPoint on the 2*n_dirs images (up cameras first, then down), MobileNetVLAD on the n_dirs
 * up images, BFMatcher(L2, crossCheck) up <-> down per direction, and the D2H copy of every result into one pinned block.
 * The handles are borrowed (sp created with max_batch >= 2*n_dirs on sp_ctx, vlad with max_batch >= n_dirs on vlad_ctx,
 * both contexts on the same device).  Camera lifting / triangulation (:73-106, 405-454, 558-576): inside the unit for the model set with
 * omni_cam_set_stereo_model and the lens set with omni_cam_set_camera_model (below: camodocal's PINHOLE with distortion and MEI; the ideal pinhole unless set). */
typedef struct omni_cam_result {      /* pointers into the handle's pinned host block; valid until its next enqueue */
    int n_dirs, max_num, desc_dim, global_dim;
    const float* kps_xy;      /* [2*n_dirs][max_num][2] */
    const int*   n_kps;       /* [2*n_dirs] */
    const float* desc;        /* [2*n_dirs][max_num][desc_dim] */
    const float* scores;      /* [2*n_dirs][max_num] */
    const float* global_desc; /* [n_dirs][global_dim] */
    const int*   match_up;    /* [n_dirs][max_num]  key-point index in the up image   (cv::DMatch::queryIdx) */
    const int*   match_down;  /* [n_dirs][max_num]  key-point index in the down image (cv::DMatch::trainIdx) */
    const float* match_dist;  /* [n_dirs][max_num] */
    const int*   n_matches;   /* [n_dirs] */
    int n_images;             /* 2*n_dirs (omni_cam_create) or n_dirs (omni_cam_create_mono): the leading dimension of kps_xy / n_kps / desc / scores */
} omni_cam_result;
omni_cam* omni_cam_create(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_dirs, int max_num,
                          int global_dim, int bf_mode);
/* CameraConfig::PINHOLE_DEPTH (loop_cam.cpp:190-194; generate_gray_depth_image_descriptor :231-339; launch/realsense.launch): ONE camera per
 * image -- SuperPoint and MobileNetVLAD on each of the n_images images, no up/down match (n_matches = 0, the match arrays unused), the arrays
 * of omni_cam_result sized [n_images].  sp with max_batch >= n_images, vlad with max_batch >= n_images.  The landmarks come from the depth
 * image: inside the unit for the model set with omni_cam_set_depth_model (below: csrc/depth_landmarks.hip), on the host otherwise (host/loop_geometry.hpp
 * fill_depth_landmarks); pass fisheye_mask = 0 to the enqueue calls (:536 masks STEREO_FISHEYE only). */
omni_cam* omni_cam_create_mono(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_images, int max_num, int global_dim);
void      omni_cam_destroy(omni_cam* cam);
int       omni_cam_enqueue_dev(omni_cam* cam, const uint8_t* gray_dev, int stride, int fisheye_mask);   /* no host sync */
/* same with the images in HOST memory, image i at gray_host + i*stride*height (the reference hands every engine call a host cv::Mat
 * and copies it up synchronously, tensorrt_generic.cpp:58-75): ONE asynchronous upload of the 2*n_dirs images into a staging buffer
 * owned by the handle, then the work of omni_cam_enqueue_dev.  gray_host should be pinned (omni_host_alloc) and must stay untouched
 * until omni_cam_wait returns. */
int       omni_cam_enqueue_host(omni_cam* cam, const uint8_t* gray_host, int stride, int width, int height, int fisheye_mask);
/* the same from segments of (pinned) host memory, rows packed: the up cameras' images = the concatenation of n_up parts of up_images[i] images each, the down
 * cameras' likewise (n_down = 0 for a mono handle); the totals must be the unit's active size (omni_cam_set_active).  One asynchronous copy per part. */
int       omni_cam_enqueue_host_parts(omni_cam* cam, const uint8_t* const* up, const int* up_images, int n_up, const uint8_t* const* down, const int* down_images,
                                      int n_down, int width, int height, int fisheye_mask);
/* A unit of RAW fisheye frames: the flattening (FisheyeUndist::undist_all_cuda in front of LoopCam::on_flattened_images) runs inside the unit.  n_keyframes frames
 * of the up camera and as many of the down camera (u8, src_stride; frame i at + i * src_stride * source height), `up` / `down` = the two cameras' maps.  Views
 * [first_view, n_views) of every frame become the unit's directions (first_view = 1 for the reference's rig: LoopCam never reads the top view 0, loop_cam.h:64-73),
 * in the order of omni_cam_enqueue_dev: [up: frame 0's views, frame 1's, ... | down: the same].  n_keyframes * (n_views - first_view) must be the unit's active size
 * (omni_cam_set_active) and every such view of both objects of the networks' size; stereo handles only.  fisheye_mask != 0: the rows omni_fisheye_mask_rows names
 * are written as zeros without being computed (both networks blank them anyway).  Bytes = omni_flatten_enqueue_dev's.  Asynchronous, no host synchronisation; the
 * remap runs on the unit's SuperPoint stream, so keep `up` and `down` alive until omni_cam_wait.
 * _host: the frames in (pinned) host memory, untouched until omni_cam_wait returns: one asynchronous upload per camera into a staging buffer owned by the handle. */
int       omni_cam_enqueue_fisheye_dev(omni_cam* cam, omni_flatten* up, omni_flatten* down, const uint8_t* up_dev, const uint8_t* down_dev, int src_stride,
                                       int n_keyframes, int first_view, int fisheye_mask);
int       omni_cam_enqueue_fisheye_host(omni_cam* cam, omni_flatten* up, omni_flatten* down, const uint8_t* up_host, const uint8_t* down_host, int src_stride,
                                        int n_keyframes, int first_view, int fisheye_mask);
/* A unit of RAW stereo-pinhole frames (CameraConfig::STEREO_PINHOLE: generate_stereo_image_descriptor for one direction, loop_cam.cpp:189-196; the left and right
 * cameras take the roles of up and down): n_keyframes left frames and as many right frames of the CAMERA's size (u8, src_stride; frame i at + i * src_stride *
 * source height); the resize to the networks' size (`resize`, above) runs inside the unit, on its SuperPoint stream, MobileNetVLAD starts behind the left camera,
 * and no rows are blanked (:536 masks STEREO_FISHEYE only).  With one direction the unit's active size counts key frames: n_keyframes must equal it
 * (omni_cam_set_active).  Refused before anything is enqueued: a mono handle, a resize object whose destination is not the networks' size or that lives on
 * another device, src_stride below the source width, a unit in flight.  Keep `resize` alive until omni_cam_wait.
 * _host: the frames in (pinned) host memory, untouched until omni_cam_wait returns: one asynchronous upload per camera into a staging buffer owned by the handle.
 * _host_parts: each camera's frames as the concatenation of parts (part i: *_images[i] frames), as omni_cam_enqueue_host_parts. */
int       omni_cam_enqueue_raw_dev(omni_cam* cam, omni_resize* resize, const uint8_t* left_dev, const uint8_t* right_dev, int src_stride, int n_keyframes);
int       omni_cam_enqueue_raw_host(omni_cam* cam, omni_resize* resize, const uint8_t* left_host, const uint8_t* right_host, int src_stride, int n_keyframes);
int       omni_cam_enqueue_raw_host_parts(omni_cam* cam, omni_resize* resize, const uint8_t* const* left, const int* left_images, int n_left,
                                          const uint8_t* const* right, const int* right_images, int n_right, int src_stride);
/* The first `bytes` of the handle's own input block -- the images the last omni_cam_enqueue_host / _host_parts / _fisheye_* / _raw_* unit fed to the networks, [image][H][W],
 * before the networks' own masking -- copied to out_host (blocking; for tests and for `show`-style debugging, loop_cam.cpp:471-515).  OMNI_ERR_INVALID while a unit
 * is pending, or when the last unit read a caller's buffer through omni_cam_enqueue_dev. */
int       omni_cam_get_input(omni_cam* cam, uint8_t* out_host, int64_t bytes);
int       omni_cam_wait(omni_cam* cam, omni_cam_result* out);
/* A unit smaller than the handle was created for (a partly filled micro-batch of key frames that must not wait any longer): the next enqueues read
 * cams * n_dirs images -- the up cameras' first, the down cameras' right behind them -- and every array of omni_cam_result has that leading dimension.
 * 1 <= n_dirs <= the n_dirs of omni_cam_create; not while a unit is in flight. */
int       omni_cam_set_active(omni_cam* cam, int n_dirs);
/* non-blocking: *ready = 1 when omni_cam_wait would return at once (hipEventQuery on the unit's two events), or when nothing is pending */
int       omni_cam_ready(omni_cam* cam, int* ready);
/* Units in flight, oldest first: whatever is enqueued on `later` from now on starts behind the CONVOLUTION STACK of `earlier`'s last enqueue (an event
 * on the device; the host does not wait).  Without it the units' CU-filling kernels take turns, every unit finishes late and together; with it the
 * oldest unit finishes first while the next one's convolutions run under its small-grid tail (NMS, descriptor sampling, matcher).
 * streams: 1 = `later`'s SuperPoint stream waits, 2 = its MobileNetVLAD stream too, 0 = no-op. */
int       omni_cam_order_after(omni_cam* later, omni_cam* earlier, int streams);

/* ---- stereo landmarks: the lifting and the up/down triangulation of generate_stereo_image_descriptor (loop_cam.cpp:397-444; triangulatePoint :73-106; the lifted
 * key points of extractor_img_desc_deepnet :558-566) -- the flattened fisheye views (ideal pinholes) and the stereo-pinhole pair with the lens model of
 * omni_camera_model, below (the ideal pinhole unless one is given).  The arithmetic is stated once, in csrc/landmark_plan.h and csrc/camera_plan.h: f64, every product and sum rounded on its own, the same operations in the same order as host/geometry.hpp (triangulate_point,
 * stereo_landmarks) and host/loop_geometry.hpp (fill_stereo_landmarks).  Poses and extrinsics are xyz + quaternion wxyz (7 doubles; the quaternion is normalised
 * on the way in).  The match lists must be one-to-one (every matcher mode of this library); a match whose index is outside its image's key points is skipped. */
#define OMNI_STEREO_MAX_DIRS 8
typedef struct omni_stereo_model {
    double fx, fy, cx, cy;            /* of the network-size image: the lift starts as ((double)x - cx) / fx, ((double)y - cy) / fy and, for the ideal pinhole, ends there;
                                         with an omni_camera_model, below, the undistortion follows; MEI: gamma1, gamma2, u0, v0 */
    double triangle_thres;            /* a match is dropped when err > triangle_thres || the point lies behind the up camera */
    int accept_min_3d_pts;            /* no landmarks at all unless the up image has MORE key points than this (loop_cam.cpp:385) */
    int dirs_per_keyframe;            /* 1 .. OMNI_STEREO_MAX_DIRS: image pair p belongs to key frame p / dirs_per_keyframe, direction p % dirs_per_keyframe */
    double up_extrinsic[OMNI_STEREO_MAX_DIRS][7], down_extrinsic[OMNI_STEREO_MAX_DIRS][7];   /* body -> camera, per direction */
} omni_stereo_model;
/* The stage on HBM-resident arrays laid out as the key-frame unit's, [up images | down images]: kps_xy_dev [2*n_pairs][max_num][2], n_kps_dev [2*n_pairs],
 * match_up_dev / match_down_dev [n_pairs][max_num], n_matches_dev [n_pairs], poses7_dev [n_pairs / dirs_per_keyframe][7] (pose_drone per key frame).
 * Outputs (device): norm2d_out [2*n_pairs][max_num][2] float (zeros behind an image's last key point), l3d_out [2*n_pairs][max_num][3] float,
 * flag_out [2*n_pairs][max_num] u8, count_out [n_pairs] (count_3d).  dirs_per_keyframe must be the model's and divide n_pairs; max_num <= 1024.
 * Asynchronous on the context's stream. */
int omni_landmarks_enqueue_dev(omni_ctx* ctx, const omni_stereo_model* model, const double* poses7_dev, int n_pairs, int dirs_per_keyframe, int max_num,
                               const float* kps_xy_dev, const int* n_kps_dev, const int* match_up_dev, const int* match_down_dev, const int* n_matches_dev,
                               float* norm2d_out, float* l3d_out, uint8_t* flag_out, int* count_out);
/* The same stage inside the key-frame unit: with a model set, every unit runs the kernel on its SuperPoint stream right behind the up/down match and copies the
 * four arrays into the handle's pinned block in front of the unit's event.  model == NULL switches the stage off again.  Refused: a mono handle, a
 * dirs_per_keyframe that does not divide the handle's n_dirs, a unit in flight. */
int omni_cam_set_stereo_model(omni_cam* cam, const omni_stereo_model* model);
/* pose_drone of the n_keyframes key frames of the NEXT unit (poses7 [n_keyframes][7], host memory, copied before the call returns; uploaded on the SuperPoint
 * stream at enqueue).  Refused with a unit in flight or without a model.  While a model is set EVERY enqueue entry (_dev, _host, _host_parts, _fisheye_*, _raw_*)
 * refuses, before anything is enqueued, a unit whose active size is not n_keyframes * dirs_per_keyframe -- also one whose poses were not set since the last unit. */
int omni_cam_set_poses(omni_cam* cam, const double* poses7, int n_keyframes);
typedef struct omni_cam_landmarks_result {      /* pointers into the handle's pinned host block; valid after omni_cam_wait until the handle's next enqueue */
    int n_images, n_dirs, max_num;              /* of that unit: n_images = 2 * n_dirs (a mono unit with a depth model: n_images = n_dirs) */
    const float*   norm2d;                      /* [n_images][max_num][2]  the message's landmarks_2d_norm */
    const float*   landmarks_3d;                /* [n_images][max_num][3] */
    const uint8_t* landmarks_flag;              /* [n_images][max_num] */
    const int*     count_3d;                    /* [n_dirs] (a mono unit with a depth model: one per image) */
} omni_cam_landmarks_result;
/* OMNI_ERR_INVALID while a unit is pending, and when the last unit ran without a model (a stereo model, or a mono handle's depth model: omni_cam_set_depth_model) */
int omni_cam_landmarks(omni_cam* cam, omni_cam_landmarks_result* out);

/* ---- the lens model of the lift: what the reference's camodocal camera (camera_config_path, loop_cam.cpp:31-33) does in cam->liftProjective before the division by z
 * (:403-407, :289-291, :558-569).  The arithmetic is stated once, in csrc/camera_plan.h (f64, every product and sum rounded on its own): the distorted
 * normalised point from the intrinsics, camodocal's fixed number of undistortion rounds (8 for PINHOLE, 6 for MEI, no convergence test), then the ray divided by
 * its z.  camodocal is not vendored: the header's formulas are the specification and parity with camodocal itself is UNPINNED.  The intrinsics stay where they
 * were -- omni_stereo_model's fx fy cx cy (for MEI they hold gamma1, gamma2, u0, v0).  PINHOLE with all four coefficients exactly 0 is the ideal pinhole: the
 * rounds are skipped (camodocal's m_noDistortion) and the result has the bits of ((double)x - cx) / fx.  Nothing is clamped: an iteration that diverges or a
 * negative radicand gives inf / NaN, on the device as on the host. */
#define OMNI_CAMERA_PINHOLE 0
#define OMNI_CAMERA_MEI 1
typedef struct omni_camera_model { int type; double k1, k2, p1, p2, xi; } omni_camera_model;
/* omni_landmarks_enqueue_dev with a lens model (camera == NULL: the ideal pinhole, which is what omni_landmarks_enqueue_dev passes).  Refused before anything is
 * launched: an unknown type, a non-finite coefficient, MEI with xi <= 0. */
int omni_landmarks_enqueue_dev_camera(omni_ctx* ctx, const omni_stereo_model* model, const omni_camera_model* camera, const double* poses7_dev, int n_pairs,
                                      int dirs_per_keyframe, int max_num, const float* kps_xy_dev, const int* n_kps_dev, const int* match_up_dev, const int* match_down_dev,
                                      const int* n_matches_dev, float* norm2d_out, float* l3d_out, uint8_t* flag_out, int* count_out);
/* The lens model of the unit's stereo-landmark stage (camera == NULL: ideal again).  It is kept next to the stereo model, not inside it: a later
 * omni_cam_set_stereo_model leaves it as it is.  Refused: a mono handle, a unit in flight, what omni_landmarks_enqueue_dev_camera refuses. */
int omni_cam_set_camera_model(omni_cam* cam, const omni_camera_model* camera);
/* csrc/camera_plan.h on the host, no GPU, no context: n pixels xy [n][2] float -> out_xy_f64 [n][2] lifted and divided by z (camera == NULL: ideal);
 * intrinsics4 = fx fy cx cy (gamma1 gamma2 u0 v0).  _project_host is the forward model (tests, synthetic data): xyz [n][3] double -> pixels [n][2] double. */
int omni_camera_lift_host(const omni_camera_model* camera, const double* intrinsics4, const float* xy, int n, double* out_xy_f64);
int omni_camera_project_host(const omni_camera_model* camera, const double* intrinsics4, const double* xyz, int n, double* out_xy_f64);

/* ---- depth landmarks: what generate_gray_depth_image_descriptor does between the networks and the frame message (CameraConfig::PINHOLE_DEPTH, loop_cam.cpp:260-304; the
 * lifted key points of :558-566).  The arithmetic is stated once, in csrc/depth_plan.h (the lens: csrc/camera_plan.h; the pose algebra: csrc/landmark_plan.h): f64, every
 * product and sum rounded on its own, the same operations in the same order as host/loop_geometry.hpp's fill_image_descriptor + fill_depth_landmarks -- including the
 * latter's recorded deviation: a key point the reference's 640 x 480 gate lets through but which lies outside THIS depth image gets no landmark.  Per image: no landmarks at
 * all unless it has MORE than accept_min_3d_pts key points and a depth frame; a key point gets one when its depth (u16 millimetres under the pixel rounded half to
 * even, / 1000.0) lies strictly between depth_near and depth_far: pose_drone * extrinsic * (lifted pixel * depth), as floats, flag 1. */
typedef struct omni_depth_model {
    double fx, fy, cx, cy;            /* of the network-size image, as omni_stereo_model's (MEI: gamma1, gamma2, u0, v0) */
    double depth_near, depth_far;     /* metres (DEPTH_NEAR_THRES / DEPTH_FAR_THRES) */
    int accept_min_3d_pts;            /* no landmarks at all unless the image has MORE key points than this (loop_cam.cpp:266-270) */
    int depth_width, depth_height;    /* of every depth image */
    double extrinsic[7];              /* body -> camera, xyz + quaternion wxyz (normalised on the way in) */
} omni_depth_model;
/* The stage on HBM-resident arrays: kps_xy_dev [n_images][max_num][2], n_kps_dev [n_images], poses7_dev [n_images][7] (pose_drone of each image's key frame),
 * depth_dev: image i at depth_dev + i * depth_stride_elems * depth_height (u16, stride in ELEMENTS), have_dev [n_images] u8 (0: the image has no depth frame and gets
 * no landmarks; NULL: every image has one).  Outputs (device): norm2d_out [n_images][max_num][2] float (zeros behind an image's last key point), l3d_out
 * [n_images][max_num][3] float, flag_out [n_images][max_num] u8, count_out [n_images] (count_3d).  camera == NULL: the ideal pinhole.  Refused before anything is
 * launched: a null argument, max_num outside 1..1024, a zero or NaN focal length, what omni_landmarks_enqueue_dev_camera refuses of a lens, depth_width / depth_height
 * below 1, a stride below the width, a NaN depth_near or depth_far.  Asynchronous on the context's stream. */
int omni_depth_landmarks_enqueue_dev(omni_ctx* ctx, const omni_depth_model* model, const omni_camera_model* camera, const double* poses7_dev, int n_images, int max_num,
                                     const float* kps_xy_dev, const int* n_kps_dev, const uint16_t* depth_dev, int depth_stride_elems, const uint8_t* have_dev,
                                     float* norm2d_out, float* l3d_out, uint8_t* flag_out, int* count_out);
/* the same arguments in HOST memory, csrc/depth_plan.h compiled by g++: no GPU, no context.  The same refusals. */
int omni_depth_landmarks_host(const omni_depth_model* model, const omni_camera_model* camera, const double* poses7, int n_images, int max_num, const float* kps_xy,
                              const int* n_kps, const uint16_t* depth, int depth_stride_elems, const uint8_t* have, float* norm2d_out, float* l3d_out, uint8_t* flag_out,
                              int* count_out);
/* The same stage inside a MONO key-frame unit (omni_cam_create_mono): with a model set, every unit runs the kernel on its SuperPoint stream behind the key points and
 * copies the four arrays into the handle's pinned block in front of the unit's event; omni_cam_landmarks then serves the unit with n_images == n_dirs and count_3d
 * [n_images].  The lens travels in this call (camera == NULL: the ideal pinhole): omni_cam_set_camera_model keeps refusing mono handles.  model == NULL switches the
 * stage off again.  Refused: a stereo handle, a unit in flight, what omni_depth_landmarks_enqueue_dev refuses of a model and a lens.
 * With a depth model omni_cam_set_poses is accepted on the mono handle: one key frame per image, n_keyframes = the unit's active size. */
int omni_cam_set_depth_model(omni_cam* cam, const omni_depth_model* model, const omni_camera_model* camera);
/* The depth frames of the NEXT unit, in host memory: frames[i] = image i's depth_height rows of stride_elems u16 elements, or NULL -- this key frame has no depth
 * image and gets no landmarks.  Copied into the handle's pinned block before the call returns; uploaded on the SuperPoint stream at enqueue, next to the poses.
 * _dev: the frames are in HBM already (image i at depth_dev + i * stride_elems * depth_height), BORROWED until omni_cam_wait; have_host [n_images] u8 or NULL (all).
 * Refused: no depth model, a unit in flight, n_images outside 1 .. the handle's size, a stride below depth_width.  While a depth model is set every enqueue entry a
 * mono handle accepts (_dev, _host, _host_parts, _jpeg_host with right_files = NULL) refuses, before anything is enqueued, a unit whose poses or depth frames were
 * not set since the last unit, or were set for another size than the unit's active size. */
int omni_cam_set_depth_host(omni_cam* cam, const uint16_t* const* frames, int stride_elems, int n_images);
int omni_cam_set_depth_dev(omni_cam* cam, const uint16_t* depth_dev, int stride_elems, const uint8_t* have_host, int n_images);

/* ---- loop verification: the homography RANSAC of compute_correspond_features (loop_detector.cpp:574-598: the 3-D-flag filter, then
 * cv::findHomography(old_2d, new_2d, RANSAC, 3, mask)) on the GPU, f64 (csrc/homography.hip; the arithmetic: csrc/ransac_plan.h, operation for operation
 * that of host/geometry.hpp's find_homography_ransac -- the same mask, the same best model).  Per pair:
 *   status  OMNI_HG_UNFILTERED  fewer than 4 points: nothing was estimated (the reference keeps the flagged matches as they are);
 *           OMNI_HG_OK          mask[i] = 1 for the inliers of the best model, H = that model (9 doubles, row major, H[8] = 1);
 *           OMNI_HG_NO_MODEL    the host function's `false`: mask all 0;
 *           OMNI_HG_HOST        the device gave up on degenerate input (more than 256 attempts for one subset, or more than 262 144 random numbers):
 *                               run the host function for this pair.
 *   info    {count, iterations run, iteration of the best model (-1: none), inliers of the best model}. */
#define OMNI_HG_UNFILTERED 0
#define OMNI_HG_OK 1
#define OMNI_HG_NO_MODEL 2
#define OMNI_HG_HOST 3
/* The RANSAC kernel alone on point lists from the host: src_xy / dst_xy [n_pairs][max_n][2] float (pair p: the OLD and the NEW image's pixels of its count[p]
 * correspondences), count [n_pairs] in [0, max_n].  Outputs (host): status [n_pairs], mask [n_pairs][max_n] u8 (zeros behind count), H [n_pairs][9],
 * info [n_pairs][4].  1 <= n_pairs <= 64, 1 <= max_n <= 1024.  Blocking. */
int omni_homography_ransac_multi(omni_ctx* ctx, int n_pairs, int max_n, const float* src_xy, const float* dst_xy, const int* count, int* status, uint8_t* mask,
                                 double* H, int* info);
/* omni_bf_match_multi followed, in the same round trip (one upload, four launches, one download), by the flag filter and the RANSAC of every pair: besides
 * omni_bf_match_multi's arguments, per pair q_xy[p] [nq[p]][2] / t_xy[p] [nt[p]][2] = landmarks_2d of the new (query) and the old (train) image and
 * q_flags[p] [n_flags[p]] = landmarks_flag of the new image (n_flags[p] in [0, max_n]; q_flags[p] may be NULL when it is 0).  Match i of pair p is kept
 * when q_idx[i] < n_flags[p] && q_flags[p][q_idx[i]], in match order.  Further outputs (host): kept [n_pairs][max_n] = the positions in the match list of
 * the n_kept[p] matches kept; mask [n_pairs][max_n] over the KEPT list; H, info, status as above (count = n_kept[p]).  The stop rule's table (count x inliers
 * -> iterations, evaluated on the host with its own pow / log) is kept in HBM per context and grows with the largest max_n seen. */
int omni_bf_match_homography_multi(omni_ctx* ctx, int n_pairs, const float* const* q_host, const int* nq, const float* const* t_host, const int* nt, int dim,
                                   int mode, int max_n, const float* const* q_xy, const float* const* t_xy, const uint8_t* const* q_flags, const int* n_flags,
                                   int* q_idx, int* t_idx, float* dist, int* n_matches, int* kept, int* n_kept, uint8_t* mask, double* H, int* info, int* status);

/* ---- loop verification: the correspondences of a candidate, assembled behind the homography kernels in the same round trip (csrc/corr_assemble.hip; the
 * arithmetic: csrc/corr_plan.h, operation for operation that of the two compute_correspond_features of host/loop_geometry.hpp, loop_detector.cpp:431-624).
 * A candidate owns pair_count <= 4 consecutive pairs of the call, in the order of the direction pairing.  Per pair: the flag filter, then the compaction by the
 * homography mask (a pair with fewer than 4 flagged matches keeps them all); per candidate the concatenation over its pairs of X = landmarks_3d of the new
 * image and u = landmarks_2d_norm of the old image rotated by the pair's dq_old and cast to float -- the layout omni_pnp_ransac_multi takes.  gate:
 *   OMNI_CORR_OK      compute_correspond_features' `true` and compute_loop_core's size gate (:291) passed: compute_relative_pose is next;
 *   OMNI_CORR_REJECT  one of the two failed: not a loop;
 *   OMNI_CORR_HOST    one of the candidate's pairs came back OMNI_HG_HOST: run the host functions for this candidate. */
#define OMNI_CORR_OK 0
#define OMNI_CORR_REJECT 1
#define OMNI_CORR_HOST 2
typedef struct omni_corr_cand {
    int32_t pair_first, pair_count;                         /* its pairs: pair_first .. pair_first + pair_count - 1 of the call */
    int32_t min_match_pre_dir, min_direction_loop;          /* MIN_MATCH_PRE_DIR, MIN_DIRECTION_LOOP */
    int32_t min_loop_num, init_mode_min_loop_num, init_mode; /* MIN_LOOP_NUM, INIT_MODE_MIN_LOOP_NUM, and whether the candidate runs in init_mode */
    int32_t reserved;
} omni_corr_cand;
/* Everything the stage reads and writes, all in host memory (omni_corr_assemble_host) or all in device memory (the kernel).  Per pair p, rows of max_n: q_idx /
 * t_idx [n_pairs][max_n] and n_matches = the matcher's list; q_flags [n_pairs][max_n] and n_flags = landmarks_flag of the new image; nq / nt = the two images' key
 * points; mask [n_pairs][max_n] over the FLAGGED matches and hg_status = the homography stage's; q_3d [n_pairs][max_n][3] = landmarks_3d of the new image; t_norm
 * [n_pairs][max_n][2] = landmarks_2d_norm of the old one; dq_old [n_pairs][4] = (w, x, y, z).  Out: X [n_cands][cap][3], u [n_cands][cap][2] (cap >= pair_count *
 * max_n), n_corr, matched_dir_count, gate [n_cands]; new_idx / old_idx [n_pairs][max_n] and n_pair_corr [n_pairs] = the key-point indices of every pair's
 * correspondences. */
typedef struct omni_corr_io {
    int32_t n_cands, n_pairs, max_n, cap;
    const omni_corr_cand* cands;
    const int32_t *q_idx, *t_idx, *n_matches;
    const uint8_t* q_flags;
    const int32_t *n_flags, *nq, *nt;
    const uint8_t* mask;
    const int32_t* hg_status;
    const float *q_3d, *t_norm;
    const double* dq_old;
    float *X, *u;
    int32_t *n_corr, *matched_dir_count, *gate, *new_idx, *old_idx, *n_pair_corr;
} omni_corr_io;
/* csrc/corr_plan.h compiled by g++ into the library: the stage on the host, the same bits, without a GPU and without a context.  1 <= n_cands <= 64,
 * 0 <= n_pairs <= 64, 1 <= max_n <= 1024, 1 <= cap <= 4096.  Refused: a null argument, a candidate with more than 4 pairs or pairs outside the call's, cap below
 * pair_count * max_n. */
int omni_corr_assemble_host(const omni_corr_io* io);
/* The kernel alone on arrays from the host (omni_homography_ransac_multi's counterpart): io as above, every pointer in host memory; one upload, one launch, one
 * download.  The same refusals (OMNI_ERR_CAPACITY for the sizes).  *kernel_us, when not NULL: the launch's device time between two events.  Blocking. */
int omni_corr_assemble_multi(omni_ctx* ctx, const omni_corr_io* io, float* kernel_us);
/* omni_bf_match_homography_multi followed, in the same round trip (one more upload, one more launch, the same download), by the stage above: besides its
 * arguments the candidates (n_cands, cands, cap), per pair q_3d[p] [nq[p]][3], t_norm[p] [nt[p]][2] and dq_old [n_pairs][4], and the stage's outputs (host). */
int omni_bf_match_homography_corr_multi(omni_ctx* ctx, int n_pairs, const float* const* q_host, const int* nq, const float* const* t_host, const int* nt, int dim,
                                        int mode, int max_n, const float* const* q_xy, const float* const* t_xy, const uint8_t* const* q_flags, const int* n_flags,
                                        int n_cands, const omni_corr_cand* cands, int cap, const float* const* q_3d, const float* const* t_norm, const double* dq_old,
                                        int* q_idx, int* t_idx, float* dist, int* n_matches, int* kept, int* n_kept, uint8_t* mask, double* H, int* info, int* status,
                                        float* X, float* u, int* n_corr, int* matched_dir_count, int* gate, int* new_idx, int* old_idx, int* n_pair_corr);

/* ---- loop verification: the RANSAC half of compute_relative_pose (loop_detector.cpp:355-413: cv::solvePnPRansac over EPnP models of 5 points, reprojection
 * error 3, confidence 0.99) on the GPU, f64 (csrc/pnp.hip; the arithmetic: csrc/pnp_plan.h, operation for operation that of host/geometry.hpp's
 * ransac_run<PnPModel> -- the same mask, the same best model).  The refit on the inliers (geom::pnp_refit) stays with the caller.  Per candidate:
 *   status  OMNI_PNP_SKIPPED   fewer than 6 correspondences: solve_pnp_ransac returns false without drawing;
 *           OMNI_PNP_OK        the best model has at least 6 inliers: mask[i] = 1 for them, Rt = that model (R row major, then t: X_cam = R X + t);
 *           OMNI_PNP_NO_MODEL  the host function's `false` (no model, or a best model with five inliers): mask all 0, Rt all 0;
 *           OMNI_PNP_HOST      the device gave up (more than 256 random numbers for one group of five distinct indices): run the host function.
 *   info    {count, iterations run, iteration of the best model (-1: none), inliers of the best model}. */
#define OMNI_PNP_SKIPPED 0
#define OMNI_PNP_OK 1
#define OMNI_PNP_NO_MODEL 2
#define OMNI_PNP_HOST 3
/* X_xyz [n_cands][max_n][3] / u_xy [n_cands][max_n][2] float (candidate c: the 3-D points and the normalised image points of its count[c] correspondences),
 * count [n_cands] in [0, max_n], max_iters [n_cands] in [1, 1000] (compute_relative_pose: 100, 1 000 in init_mode).  Outputs (host): status [n_cands],
 * mask [n_cands][max_n] u8 (zeros behind count), Rt [n_cands][12], info [n_cands][4].  1 <= n_cands <= 64, 1 <= max_n <= 2048.  One upload, one launch, one
 * download; blocking.  The stop rule's table rows (inliers -> iterations, evaluated on the host with its own pow / log) are kept per context and travel with
 * the upload. */
int omni_pnp_ransac_multi(omni_ctx* ctx, int n_cands, int max_n, const float* X_xyz, const float* u_xy, const int* count, const int* max_iters, int* status,
                          uint8_t* mask, double* Rt, int* info);

/* ---- send_img: the main image of every direction as a baseline JPEG, what encode_image's cv::imencode(".jpg", img, {IMWRITE_JPEG_QUALITY, JPG_QUALITY}) asks of
 * libjpeg (loop_cam.cpp:56-71, 306-308, 463-469), on the GPU (csrc/jpeg.hip).  The arithmetic is stated once, in csrc/jpeg_plan.h: one 8-bit component, the IJG
 * luminance table scaled by the quality, jfdctint's integer DCT, the standard Huffman tables, JFIF APP0 -- libjpeg's defaults, PINNED byte for byte against Pillow
 * (libjpeg-turbo) by the CPU tests.  What cv::imencode adds beyond those defaults is UNPINNED: OpenCV is not vendored.
 * Per image: status OMNI_JPEG_OK and size = the file's bytes; or OMNI_JPEG_TRUNCATED and size 0 when the file exceeds the capacity -- nothing is ever written
 * past the capacity, and what a truncated image leaves below it is unspecified.  zero_from_row: rows at or beyond it are read as 0 (height: none) -- the rows the
 * fisheye mask blanks. */
#define OMNI_JPEG_OK 0
#define OMNI_JPEG_TRUNCATED 1
#define OMNI_JPEG_HEADER_BYTES 328   /* SOI, APP0, DQT, SOF0, DHT DC, DHT AC, SOS: the scan starts here */
typedef struct omni_jpeg omni_jpeg;
/* A handle owns the tables of one quality, the header of one size and all device scratch for up to max_images images of width x height.  1 <= width, height <=
 * 65535 (and at most 2^21 blocks of 8 x 8), max_images >= 1, quality clamped to 1..100, capacity_per_image >= OMNI_JPEG_HEADER_BYTES + 2. */
omni_jpeg* omni_jpeg_create(omni_ctx* ctx, int width, int height, int max_images, int quality, int64_t capacity_per_image);
void       omni_jpeg_destroy(omni_jpeg* j);
/* n_images images (u8, `stride` bytes between rows, image i at gray_dev + i * stride * height) -> out_dev [n_images][capacity_per_image], sizes_dev [n_images] int32,
 * status_dev [n_images] int32.  Asynchronous on the context's stream, no host synchronisation.  Refused before anything is launched: n_images outside
 * [1, max_images], stride below the width, zero_from_row outside [0, height]. */
int        omni_jpeg_enqueue_dev(omni_jpeg* j, const uint8_t* gray_dev, int stride, int n_images, int zero_from_row, uint8_t* out_dev, int* sizes_dev, int* status_dev);
/* everything in front of the scan: OMNI_JPEG_HEADER_BYTES bytes to out_host (no GPU) */
int        omni_jpeg_header(int width, int height, int quality, uint8_t* out_host);
/* csrc/jpeg_plan.h compiled by g++ into the library: the same bytes without a GPU.  *size and *status as above; OMNI_ERR_INVALID for sizes outside 1..65535,
 * a stride below the width, a capacity below OMNI_JPEG_HEADER_BYTES + 2, zero_from_row outside [0, height]. */
int        omni_jpeg_encode_host(const uint8_t* gray, int stride, int width, int height, int quality, int zero_from_row, uint8_t* out, int64_t capacity,
                                 int64_t* size, int* status);
/* The same stage inside the key-frame unit: with a quality set, every enqueue entry (_dev, _host, _host_parts, _fisheye_*, _raw_*; mono and stereo) also encodes the
 * unit's MAIN images -- on a stereo handle the up / left images [0, n_dirs) (image_left, :463-468; LOWER_CAM_AS_MAIN is false in this build), on a mono handle all
 * n_images images (:306-308) -- on the MobileNetVLAD stream behind that stream's read of the same images, and copies bytes, sizes and statuses into the handle's
 * pinned block in front of the unit's event.  A unit enqueued with fisheye_mask != 0 encodes with zero_from_row = omni_fisheye_mask_rows' first row: the reference
 * blanks those rows in the very pixels it encodes (loop_cam.cpp:536-539 writes through a cv::Mat that shares its data with msg.left_images[vcam_id]).
 * quality 0 switches the stage off again.  Refused with a unit in flight, and for a capacity below OMNI_JPEG_HEADER_BYTES + 2. */
int        omni_cam_set_jpeg(omni_cam* cam, int quality, int64_t capacity_per_image);
typedef struct omni_cam_jpeg_result {           /* pointers into the handle's pinned host block; valid after omni_cam_wait until the handle's next enqueue */
    int n_images;                               /* the main images of that unit */
    int64_t capacity;                           /* bytes between two images in `bytes` */
    const uint8_t* bytes;                       /* [n_images][capacity] */
    const int*     sizes;                       /* [n_images] */
    const int*     status;                      /* [n_images] OMNI_JPEG_OK / OMNI_JPEG_TRUNCATED */
} omni_cam_jpeg_result;
/* OMNI_ERR_INVALID while a unit is pending, and when the last unit ran with the stage off */
int        omni_cam_jpeg(omni_cam* cam, omni_cam_jpeg_result* out);

/* ---- is_compressed_images: camera frames that arrive as JPEG files (sensor_msgs::CompressedImage; swarm_loop.cpp:72-89, 291-292, 341-360) become gray images,
 * what cv::imdecode(data, cv::IMREAD_GRAYSCALE) asks of libjpeg (loop_utils.cpp:8), on the GPU (csrc/jpeg_dec.hip).  The arithmetic is stated once, in
 * csrc/jpeg_dec_plan.h: the first component alone, dequantised, jidctint's islow IDCT, range limit -- libjpeg-turbo's JCS_GRAYSCALE output, PINNED pixel for
 * pixel against Pillow (Image.draft('L') for colour files) by the CPU tests.  cv::imdecode itself is UNPINNED: OpenCV is not vendored, and that it asks libjpeg
 * for JCS_GRAYSCALE is read from knowledge, not run.
 * A file is classified as
 *   OMNI_JPEGDEC_OK           baseline, one scan, no restart interval, the first component sampled {1,2} x {1,2} and the others 1 x 1: decoded by the kernels
 *   OMNI_JPEGDEC_HOST         a valid baseline file the kernels do not take (restart interval, several scans, other sampling, a file above the handle's capacity):
 *                             decoded on the calling thread by the g++ build, its pixels uploaded
 *   OMNI_JPEGDEC_UNSUPPORTED  progressive, arithmetic, lossless, 12-bit, 16-bit quantisation tables, a component count other than 1 or 3: refused
 *   OMNI_JPEGDEC_CORRUPT      not a decodable file, or a scan that errs or ends before the picture's last block: the picture is ALL ZEROS
 * Restart intervals: OMNI_JPEGDEC_RESTART_WGS (0..64, default 0), as it is when the handle is created.  0: as listed above.  W >= 1: a file whose ONLY obstacle is
 * its restart interval (DRI) is decoded by the kernels and reports OMNI_JPEGDEC_OK; its intervals -- independent streams: byte-aligned, known entry state, DC
 * predictor zero, known first block -- are spread over at most W workgroups balanced by bits.  The pixels are the same.  Such a file stays HOST when it cannot be
 * planned (more intervals in one workgroup's share than that workgroup holds subsequences: 4096), and is CORRUPT when its scan holds fewer restart markers than
 * ceil(MCUs / interval) - 1 or when an interval's bits end before its blocks do (there the host decoder reads on into the next interval: the one divergence;
 * libjpeg's own resynchronisation is UNPINNED either way).  Surplus markers are ignored.
 * Files without a restart interval: OMNI_JPEGDEC_PLAIN_WGS (0..64, default 0), as it is when the handle is created.  0 or 1: one workgroup of the entropy kernel
 * decodes such a picture.  W >= 2: an OMNI_JPEGDEC_OK file is decoded over min(W, subsequences) chunks of consecutive subsequences that relax on their own, a seam
 * relaxation over the whole picture that repairs what the seams between chunks got wrong, and a write pass of one subsequence per lane; the subsequence length
 * is OMNI_JPEGDEC_SUBSEQ_BITS doubled only until W chunks of 4096 subsequences hold the picture.  No workgroup waits for another.  Same pixels, same status, the
 * classification untouched; the two switches are independent and one batch may hold both kinds of file.
 * Unstuffing: OMNI_JPEGDEC_UNSTUFF_DEV (0 or 1, default 0), as it is when the handle is created.  0: the calling thread removes the 0xFF00 stuffing and the restart
 * markers of every scan the kernels decode, byte by byte, and uploads the clean scans.  1: it visits the 0xFF bytes alone (the scan's end, the clean length, the
 * restart offsets, the clean offset of every tile of 4096 raw bytes), uploads the scans as they stand in the files, and one kernel in front of the others compacts
 * them tile by tile; the handle's device block and pinned block grow by max_images x (capacity_per_image + 32) bytes and the tile tables.  Same pixels, same
 * status, same statistics; independent of the two switches above. */
#define OMNI_JPEGDEC_OK 0
#define OMNI_JPEGDEC_HOST 1
#define OMNI_JPEGDEC_UNSUPPORTED 2
#define OMNI_JPEGDEC_CORRUPT 3
typedef struct omni_jpegdec omni_jpegdec;
/* A handle owns the pinned staging block and all device scratch for up to max_images files of at most capacity_per_image bytes whose pictures are width x height.
 * 1 <= width, height <= 65535 (at most 2^20 blocks of 8 x 8), 1 <= max_images <= 65535, 1024 <= capacity_per_image <= 2^28.  The subsequence length of the
 * entropy kernel is OMNI_JPEGDEC_SUBSEQ_BITS (a power of two) as it is when the handle is created. */
omni_jpegdec* omni_jpegdec_create(omni_ctx* ctx, int width, int height, int max_images, int64_t capacity_per_image);
void          omni_jpegdec_destroy(omni_jpegdec* d);
/* n_images files -> out_dev: picture i at out_dev + i * out_stride * height, out_stride bytes between rows (bytes between the rows' ends are not touched);
 * status_dev [n_images] int32 OMNI_JPEGDEC_OK / HOST / CORRUPT.  Parses on the calling thread, packs descriptors + unstuffed scans (+ the pixels of HOST files)
 * into ONE pinned block, one asynchronous upload, then the kernels on the context's stream; the files may be released on return.
 * Refused before anything is enqueued: an UNSUPPORTED file, a file whose picture is not width x height, n_images outside [1, max_images], out_stride < width. */
int           omni_jpegdec_enqueue_host(omni_jpegdec* d, const uint8_t* const* files, const int64_t* sizes, int n_images, uint8_t* out_dev, int out_stride,
                                        int* status_dev);
/* Of the handle's last enqueue, after a synchronisation with the context's stream: per image the relaxation rounds that changed something, the number of
 * subsequences and their length in bits (0 0 0 for an image the kernels did not decode).  Each output [n_images] or null. */
int           omni_jpegdec_last_stats(omni_jpegdec* d, int* rounds, int* n_subseq, int* subseq_bits);
/* ... and the workgroups of the entropy kernel that decoded a share of each image (counted on the GPU): 1, or the chunks of a restart-interval file, or the
 * chunks of a picture spread by OMNI_JPEGDEC_PLAIN_WGS; 0 for an image the kernels did not decode.  A restart-interval file's rounds above are the maximum over
 * its chunks, its subsequences their total; a spread picture's rounds are the maximum over its chunks + the seam relaxation's.  chunks [n_images] */
int           omni_jpegdec_last_chunks(omni_jpegdec* d, int* chunks);
/* ... and of a picture spread by OMNI_JPEGDEC_PLAIN_WGS the seam relaxation's rounds that changed something and the subsequences it changed at least once (0 0
 * for every other image, and on a handle whose switch is 0 or 1).  Each output [n_images] or null. */
int           omni_jpegdec_last_seam(omni_jpegdec* d, int* seam_rounds, int* seam_changed);
/* MEASUREMENT: of the handle's last enqueue, once it has run: the time of its upload and of everything behind it (memsets + kernels) on the GPU, and the bytes it
 * uploaded (tools/jpegdec_timing.py) */
int           omni_jpegdec_last_ms(omni_jpegdec* d, float* upload_ms, float* kernels_ms, int64_t* uploaded_bytes);
/* TEST INFRASTRUCTURE: the device addresses and sizes of the coefficient and the DC buffer; each is followed by OMNI_JPEGDEC_GUARD_BYTES bytes of 0xA5 that
 * nothing ever writes */
#define OMNI_JPEGDEC_GUARD_BYTES 256
int           omni_jpegdec_debug_buffers(omni_jpegdec* d, void** coef_dev, int64_t* coef_bytes, void** dc_dev, int64_t* dc_bytes);
/* ... and of the state arrays of a handle whose OMNI_JPEGDEC_PLAIN_WGS is W >= 2 (max_images x W x 4096 x 8 bytes, the same guard behind them); NULL and 0 on
 * every other handle: nothing is allocated there */
int           omni_jpegdec_debug_state_buffer(omni_jpegdec* d, void** state_dev, int64_t* state_bytes);
/* Of the handle's last enqueue on a handle whose OMNI_JPEGDEC_UNSTUFF_DEV is 1: the pictures whose scan the device unstuffed, the raw scan bytes uploaded for
 * them and the clean bytes those became; 0 0 0 on a handle with the switch off */
int           omni_jpegdec_last_unstuff(omni_jpegdec* d, int* device_pictures, int64_t* raw_bytes, int64_t* clean_bytes);
/* TEST INFRASTRUCTURE: the device address behind the last clean area of the last enqueue (OMNI_JPEGDEC_UNSTUFF_DEV = 1) and the number of 0xA5 bytes that stand
 * there, written on the stream in front of the unstuff kernel; NULL and 0 with the switch off */
int           omni_jpegdec_debug_in_buffer(omni_jpegdec* d, void** clean_end_dev, int64_t* guard_bytes);
/* TEST INFRASTRUCTURE: the unstuff kernel alone on an arbitrary byte string taken as a scan: survey on the host, upload, the kernel, download.  out_host
 * [out_cap >= clean bytes + 16]: the clean bytes and the 16 zero bytes behind them, from a device block that was all 0xA5; *n_clean their number.  OMNI_ERR_HIP
 * when anything behind the padding was written */
int           omni_jpegdec_unstuff_dev(omni_ctx* ctx, const uint8_t* scan, int64_t n, uint8_t* out_host, int64_t out_cap, int64_t* n_clean);
/* TEST INFRASTRUCTURE, no GPU: csrc/jpeg_dec_plan.h's unstuffing compiled by g++.  omni_jpeg_unstuff_tile_bytes: raw bytes per tile.  omni_jpeg_unstuff_host: the
 * byte-wise pass (unstuff) over scan[0..n) -> out [out_cap >= n + 16]: the clean bytes + 16 zero bytes, *n_clean, and the clean offset behind every restart
 * marker (rst [max_rst], *n_rst).  omni_jpeg_unstuff_tiled_host: survey + every tile compacted on its own (unstuff_tiled_host), out filled with 0xA5 beforehand;
 * also *raw_end (where the scan's data end), *surveyed_clean (survey's count; *n_clean is the end of the last tile), tile_off [max_tiles >= n / tile + 1] and
 * *n_tiles.  omni_jpeg_scan_end: scan_end() from `from`; -1 for bad arguments */
int           omni_jpeg_unstuff_tile_bytes(void);
int           omni_jpeg_unstuff_host(const uint8_t* scan, int64_t n, uint8_t* out, int64_t out_cap, int64_t* n_clean, int64_t* rst, int64_t max_rst, int64_t* n_rst);
int           omni_jpeg_unstuff_tiled_host(const uint8_t* scan, int64_t n, uint8_t* out, int64_t out_cap, int64_t* n_clean, int64_t* rst, int64_t max_rst, int64_t* n_rst,
                                           int64_t* raw_end, int64_t* surveyed_clean, uint32_t* tile_off, int64_t max_tiles, int64_t* n_tiles);
int64_t       omni_jpeg_scan_end(const uint8_t* file, int64_t size, int64_t from);
/* the classification of a file without a capacity, and its picture's size (0 x 0 when no frame header can be read); no GPU */
int           omni_jpegdec_classify(const uint8_t* file, int64_t size, int* width, int* height);
/* csrc/jpeg_dec_plan.h's sequential decoder compiled by g++ into the library, next to omni_jpeg_encode_host: the same pixels without a GPU, restart intervals
 * and the other HOST files included.  out: the picture (its size: omni_jpegdec_classify), `stride` bytes between rows.  *status = the classification, or
 * OMNI_JPEGDEC_CORRUPT with the picture zeroed; an UNSUPPORTED file writes nothing.  OMNI_ERR_INVALID for null arguments and a stride below the width. */
int           omni_jpeg_decode_host(const uint8_t* file, int64_t size, uint8_t* out, int stride, int* width, int* height, int* status);
/* TEST INFRASTRUCTURE: the CPU stand-in for the kernels (csrc/jpeg_dec_plan.h decode_planned_host: the phase functions driven by plain loops over the picture's
 * interval table and chunk bounds, as the kernels see it) under the switches of each of three entries.  This one: both switches off, one chunk, subseq_bits per
 * subsequence; stats[4] = subsequences, their length, relaxation rounds that changed something, subsequences whose first-pass exit state was wrong
 * (wrong_after_first) */
int           omni_jpeg_decode_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, uint8_t* out, int stride, int* width, int* height, int* status,
                                             int* stats);
/* TEST INFRASTRUCTURE: the CPU stand-in for the kernels of a handle with OMNI_JPEGDEC_RESTART_WGS = restart_wgs (1..64), where a workgroup holds at most max_subseq
 * subsequences (the kernels: 4096): decode_planned_host over the chunk plan's interval table and chunks.  A file without a restart
 * interval goes the way of omni_jpeg_decode_parallel_host.  stats[4] = subsequences, their length, chunks, the maximum over the chunks of the relaxation rounds
 * that changed something (0 0 0 0 for a file the plan leaves to the host) */
int           omni_jpeg_decode_restart_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, int restart_wgs, int max_subseq, uint8_t* out, int stride,
                                                     int* width, int* height, int* status, int* stats);
/* TEST INFRASTRUCTURE: the CPU stand-in for the kernels of a handle with OMNI_JPEGDEC_PLAIN_WGS = plain_wgs (1..64), where a workgroup holds at most max_subseq
 * subsequences (the kernels: 4096): decode_planned_host over one interval cut into plain_chunks' chunks -- the chunk relaxation, then the seam
 * relaxation.  Every file that is not OMNI_JPEGDEC_OK goes the way of omni_jpeg_decode_parallel_host.  stats[7] = subsequences, their
 * length, chunks, the maximum over the chunks of the relaxation rounds that changed something, the seam relaxation's rounds that changed something, the
 * subsequences it changed at least once, the chunks those lie in (all 0 for a file that is not OK) */
int           omni_jpeg_decode_plain_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, int plain_wgs, int max_subseq, uint8_t* out, int stride,
                                                   int* width, int* height, int* status, int* stats);

/* The same stage inside the key-frame unit: a unit whose frames arrive as JPEG files.  The decode runs on the unit's SuperPoint stream in front of the resize, and
 * the decoded frames take the place of omni_cam_enqueue_raw_*'s: n_keyframes left files and as many right files for a stereo handle (STEREO_PINHOLE), left files
 * alone (right_files = right_sizes = NULL) for a mono handle (PINHOLE_DEPTH's gray image; the depth image stays uncompressed).  resize: camera-size pictures ->
 * the networks' size; NULL: the files hold network-size pictures, decoded straight into the unit's input block.  Everything behind is the existing unit, no
 * fisheye mask (the reference has no compressed path for STEREO_FISHEYE); omni_cam_get_input shows the block the networks read.  The handle makes its decoder at
 * first use for the pictures' size (capacity: width x height / 2 bytes per file; a larger file is decoded on the calling thread).  Refused before anything is
 * enqueued: an UNSUPPORTED file, a picture of another size, a unit in flight, n_keyframes other than the active size.  A CORRUPT frame is all zeros: no key
 * points, landmark_num 0, and the reference's own rule drops the frame. */
int        omni_cam_enqueue_jpeg_host(omni_cam* cam, omni_resize* resize_or_null, const uint8_t* const* left_files, const int64_t* left_sizes,
                                      const uint8_t* const* right_files_or_null, const int64_t* right_sizes, int n_keyframes);
/* after omni_cam_wait: OMNI_JPEGDEC_OK / HOST / CORRUPT of every frame of that unit, [left frames | right frames]; n_frames = cams x the unit's active size.
 * OMNI_ERR_INVALID while a unit is pending, and when the last unit did not come as files */
int        omni_cam_jpegdec_status(omni_cam* cam, int* status, int n_frames);
/* STEREO_FISHEYE frames as JPEG files: omni_cam_enqueue_fisheye_host with each camera's n_keyframes RAW frames given as files (what the reference's upstream,
 * VINS-Fisheye, decodes from the compressed fisheye topics in front of its own flattening; the reference itself has no such path).  ONE decode of
 * [up frames | down frames] on the unit's SuperPoint stream into the staging block omni_cam_enqueue_fisheye_host uploads into, then that entry's two remaps and the
 * unit, MobileNetVLAD behind the up camera's views.  The decoder is made at first use for the flatten objects' source size -- both must have the same --, for
 * 2 x (the handle's capacity / directions) pictures and src_w x src_h / 2 bytes per file (a larger file: HOST, same pixels).  omni_cam_jpegdec_status reports
 * 2 x n_keyframes statuses, [up frames | down frames]; a CORRUPT frame is an all-zero fisheye frame and so all-zero views; omni_cam_get_input shows the
 * flattened block.  Refused before anything is enqueued: what omni_cam_enqueue_fisheye_host refuses (a mono handle, a wrong active size, views of another size),
 * different source sizes, a unit in flight, an UNSUPPORTED file, a picture of another size. */
int        omni_cam_enqueue_fisheye_jpeg_host(omni_cam* cam, omni_flatten* up, omni_flatten* down, const uint8_t* const* up_files, const int64_t* up_sizes,
                                              const uint8_t* const* down_files, const int64_t* down_sizes, int n_keyframes, int first_view, int fisheye_mask);

/* ---- PCA fit: components_.csv / mean_.csv from the key-frame stream (csrc/pca_plan.h) ------------------------------------------------------------------------
 * The reference dumps every key point's 256-d descriptor to a text file (OUTPUT_RAW_SUPERPOINT_DESC, loop_cam.cpp:51-53, 577-582) and fits
 * sklearn.decomposition.PCA(64) on the dump in a notebook.  Here the fit's moments -- the count n, the sum s [256] and the second-moment matrix S [256][256], f64
 * -- are accumulated in HBM from what every SuperPoint pass leaves there, and only they cross PCIe.  A row is the descriptor a handle WITHOUT PCA returns
 * (raw / the channel's norm across the image's key points, f32, widened to f64); rows with a non-finite element (a channel that is zero at every key point of
 * an image: 0/0, in the reference too) are left out and counted in `skipped`.  Per kept row, in stream order: n += 1, s[c] += x[c], S[i][j] = fma(x[i], x[j],
 * S[i][j]) -- one chain per entry, so the moments depend on the row sequence alone, not on batch sizes or on how the stream was cut into calls, and equal
 * omni_pca_moments_host bit for bit. */
typedef struct omni_pcafit omni_pcafit;
omni_pcafit* omni_pcafit_create(omni_ctx* ctx);            /* an empty accumulator in HBM on ctx's device */
void         omni_pcafit_destroy(omni_pcafit* fit);        /* waits for its work; a handle it is still attached to lets go of it first */
int          omni_pcafit_reset(omni_pcafit* fit);          /* waits for what is enqueued, then n = skipped = 0, s = S = 0 */
/* the rows of one pass: raw_desc [batch][max_num][256] f32, norm_partial [batch][8][256] f32 (per-channel sums of squares over eight key-point segments),
 * n_kps [batch] (clamped to 0 .. max_num).  Asynchronous on the fit's context; batch >= 1, 1 <= max_num <= 1024 */
int          omni_pcafit_enqueue_rows_dev(omni_pcafit* fit, const float* raw_desc_dev, const float* norm_partial_dev, const int* n_kps_dev, int batch, int max_num);
/* With a fit attached every forward pass of the handle (omni_sp_infer, omni_sp_enqueue_dev, a key-frame unit that runs on the handle) enqueues the accumulation
 * on the pass's own stream behind the channel norms; results of the pass are unchanged.  NULL detaches: the pass then launches what it launched before, and so
 * does destroying either of the two.  The fit must have been created on the handle's own context (one stream: nothing to order between the pass, other enqueues
 * and the fit's readers), and one fit serves one handle at a time.  OMNI_ERR_INVALID when the fit's context is on another device, is another context of the
 * same device, or the fit is attached to another handle.  (omni_sp_postprocess_dense, a test hook, never accumulates.) */
int          omni_sp_set_pcafit(omni_sp* sp, omni_pcafit* fit_or_null);
/* both wait for the fit's work.  S_full [256][256] is handed out mirrored to a full symmetric matrix */
int          omni_pcafit_stats(omni_pcafit* fit, int64_t* n, int64_t* skipped);
int          omni_pcafit_moments(omni_pcafit* fit, double* s256, double* S_full);
/* two accumulators on the host (as omni_pcafit_moments hands them out): *n += n_right, s += s_right, S += S_right element-wise */
int          omni_pcafit_merge_host(int64_t* n, double* s256, double* S_full, int64_t n_right, const double* s256_right, const double* S_full_right);
/* C = (S - s s^T / n) / (n - 1), mean = s / n, cyclic Jacobi in f64 on the host; eigenvalues descending (ties to the lower index), the first pca_dim eigenvectors
 * are the rows of components [pca_dim][256], each with its entry of largest magnitude positive (ties to the lowest column).  Any output may be NULL:
 * components / mean in f64 and f32, explained_variance [pca_dim], *total_variance = trace(C).  OMNI_ERR_INVALID with a message for n < 2, pca_dim outside
 * 1 .. 256, n <= pca_dim */
int          omni_pca_solve_host(int64_t n, const double* s256, const double* S_full, int pca_dim, double* components, float* components_f32, double* mean,
                                 float* mean_f32, double* explained_variance, double* total_variance);
int          omni_pcafit_solve(omni_pcafit* fit, int pca_dim, double* components, float* components_f32, double* mean, float* mean_f32,
                               double* explained_variance, double* total_variance);      /* = omni_pcafit_stats + omni_pcafit_moments + omni_pca_solve_host */
/* csrc/pca_plan.h compiled by g++ into the library: omni_pcafit_enqueue_rows_dev on host arrays, without a GPU.  *n, *skipped, s256 and S_full are read and
 * updated (zeros for a new accumulator; of S_full the upper triangle is read, and it is mirrored on return) */
int          omni_pca_moments_host(const float* raw_desc, const float* norm_partial, const int* n_kps, int batch, int max_num, int64_t* n, int64_t* skipped,
                                   double* s256, double* S_full);
/* components_.csv (one component per line, comma separated) and mean_.csv (one value per line), "%.9g": what every SuperPoint handle here loads, read back to
 * the same f32 (a denormal value is written as 0: the handles' reader refuses denormals) */
int          omni_pca_write_csv(const char* comp_path, const char* mean_path, const float* components_f32, const float* mean_f32, int pca_dim);

/* ---- LoopNet wire: a key frame's images as the packets of LoopNet::broadcast_fisheye_desc (swarm_loop/src/loop_net.cpp:19-101), packed on the GPU -----------------
 * The byte layout is csrc/wire_plan.h's, which restates host/loop_net_wire.hpp's wire::encode: per image one VIOKF_HEADER packet of OMNI_WIRE_HEADER_BYTES and one
 * VIOKF_LANDMARKS packet of OMNI_WIRE_LANDMARK_BYTES per sent landmark (landmark i < n_kps is sent when flag[i] > 0 || send_all_features, in index order; the
 * header's feature_num counts the flagged ones either way; an image without key points gets no packets).  msg_id of every packet and header_id of the landmark
 * packets are left ZERO: the host numbers a frame's packets when it takes them.  Every other scalar field comes from one record per image: */
#define OMNI_WIRE_HEADER_BYTES 16545         /* 161 + 4 * 4096 */
#define OMNI_WIRE_LANDMARK_BYTES 324         /* 36 + 28 + 4 + 4 * 64 */
#define OMNI_WIRE_HEADER_OFFSET 3            /* where an image's header packet starts in its buffer: its float area then starts on a 4-byte boundary */
typedef struct omni_wire_image_meta {
    double  timestamp;
    int64_t frame_id;
    int32_t drone_id, direction, prevent_adding_db, reserved;
    double  pose_drone[7];                   /* xyz + quaternion wxyz, as sent */
    double  camera_extrinsic[7];
} omni_wire_image_meta;
/* An image's buffer: omni_wire_packet_capacity(max_num) = 3 + 16545 + 324 * max_num bytes (0 for max_num outside 1..1024); the header packet at byte 3, landmark
 * packet k at 16548 + 324 * k; bytes behind the last packet are not written.  An image's table: omni_wire_table_ints(max_num) = 2 + 2 * (1 + max_num) ints:
 * [0] packets, [1] bytes used, then (offset, size) per packet, the header first; unused entries are written as zero. */
int64_t omni_wire_packet_capacity(int max_num);
int     omni_wire_table_ints(int max_num);
/* Inputs (device), laid out as a key-frame unit's arrays: kps_xy [n_images][max_num][2] f32, n_kps [n_images] (clamped to 0..max_num), desc [n_images][max_num][64],
 * norm2d [n_images][max_num][2], l3d [n_images][max_num][3], flag [n_images][max_num] u8, global [n_images][4096], meta [n_images].  Outputs (device): packets_out
 * [n_images][capacity] (4-byte aligned), table_out [n_images][table_ints].  One workgroup per image, asynchronous on ctx's stream.  Refused before anything is
 * launched: a null argument, n_images outside 1..65535, max_num outside 1..1024, desc_dim != 64, global_dim != 4096, a misaligned packets_out. */
int     omni_wire_pack_enqueue_dev(omni_ctx* ctx, int n_images, int max_num, int desc_dim, int global_dim, int send_all_features, const float* kps_xy_dev,
                                   const int* n_kps_dev, const float* desc_dev, const float* norm2d_dev, const float* l3d_dev, const uint8_t* flag_dev,
                                   const float* global_dev, const omni_wire_image_meta* meta_dev, uint8_t* packets_out_dev, int* table_out_dev);
/* csrc/wire_plan.h compiled by g++ into the library: the same arguments in host memory, the same bytes and tables, without a GPU (no alignment asked) */
int     omni_wire_pack_host(int n_images, int max_num, int desc_dim, int global_dim, int send_all_features, const float* kps_xy, const int* n_kps, const float* desc,
                            const float* norm2d, const float* l3d, const uint8_t* flag, const float* global, const omni_wire_image_meta* meta, uint8_t* packets_out,
                            int* table_out);
/* The third packet of an image, the whole ImageDescriptor_t (channel SWARM_LOOP_IMG_DES, loop_net.cpp:37-41, 103-116; wire::encode(ImageDescriptor, with_features) of
 * host/loop_net_wire.hpp, restated in csrc/wire_plan.h): a head of 177 bytes with every scalar and every length member, then image_desc, feature_descriptor (with
 * with_features; otherwise its length member is 0), landmarks_2d_norm, landmarks_2d, landmarks_3d of ALL n_kps landmarks, then the flag bytes and the JPEG file.
 * On top of the inputs above: jpeg [n_images][jpeg_capacity] u8, jpeg_sizes [n_images], jpeg_status [n_images] as omni_jpeg_enqueue_dev leaves them (image_size is the
 * size clamped to 0..jpeg_capacity for a file of status OMNI_JPEG_OK, 0 otherwise, and 0 for every image when with_image is 0), and the images' width and height.
 * Outputs: packets_out [n_images][omni_wire_image_capacity(max_num, jpeg_capacity)] -- the packet at byte 3, so that its float area starts on a 4-byte boundary;
 * written are the packet and zeros up to the next 4-byte boundary, nothing behind that -- and sizes_out [n_images][2] = (offset, size), (0, 0) for an image without
 * key points, which is not sent.  msg_id is left ZERO (the host writes the image's id, its header packet's).  omni_wire_image_capacity = 180 + 4 * (4096 + 71 *
 * max_num) + (max_num + jpeg_capacity rounded up to 4); 0 for max_num outside 1..1024 or a jpeg_capacity that is negative, above 2^30 or no multiple of 4.
 * Refused before anything is launched: what omni_wire_pack_enqueue_dev refuses, such a jpeg_capacity, JPEG pointers that are not all null with with_image == 0 or
 * not all set with with_image != 0, a misaligned packets_out or jpeg. */
int64_t omni_wire_image_capacity(int max_num, int64_t jpeg_capacity);
int     omni_wire_pack_image_enqueue_dev(omni_ctx* ctx, int n_images, int max_num, int desc_dim, int global_dim, int with_features, int with_image,
                                         const float* kps_xy_dev, const int* n_kps_dev, const float* desc_dev, const float* norm2d_dev, const float* l3d_dev,
                                         const uint8_t* flag_dev, const float* global_dev, const omni_wire_image_meta* meta_dev, const uint8_t* jpeg_dev,
                                         const int* jpeg_sizes_dev, const int* jpeg_status_dev, int64_t jpeg_capacity, int image_width, int image_height,
                                         uint8_t* packets_out_dev, int* sizes_out_dev);
int     omni_wire_pack_image_host(int n_images, int max_num, int desc_dim, int global_dim, int with_features, int with_image, const float* kps_xy, const int* n_kps,
                                  const float* desc, const float* norm2d, const float* l3d, const uint8_t* flag, const float* global, const omni_wire_image_meta* meta,
                                  const uint8_t* jpeg, const int* jpeg_sizes, const int* jpeg_status, int64_t jpeg_capacity, int image_width, int image_height,
                                  uint8_t* packets_out, int* sizes_out);
/* The same stage inside a key-frame unit.  omni_cam_set_wire(cam, 1, send_all_features): every following unit runs the kernel on its SuperPoint stream behind the
 * landmark stage (stereo model or depth model) and behind MobileNetVLAD's rows, and copies the buffers and tables of its MAIN images -- [0, n_dirs) on a stereo
 * handle, all images on a mono handle -- into a pinned block of the handle in front of the unit's event; on = 0 switches it off again, and a unit then launches
 * exactly what it launched before.  omni_cam_set_wire_meta hands over the records of the NEXT unit's main images (copied before the call returns, as
 * omni_cam_set_poses' poses); omni_cam_wire serves the unit after omni_cam_wait.  Refused: a handle without a landmark model (the stage packs landmarks the device
 * made), descriptors other than 64 or global descriptors other than 4096 floats, a unit in flight; at enqueue, records that were not set or were set for another size. */
int     omni_cam_set_wire(omni_cam* cam, int on, int send_all_features);
int     omni_cam_set_wire_meta(omni_cam* cam, const omni_wire_image_meta* records, int n_images);
typedef struct omni_cam_wire_result {           /* pointers into the handle's pinned host block; valid after omni_cam_wait until the handle's next enqueue */
    int n_images, max_num, table_ints;
    int64_t capacity;                           /* omni_wire_packet_capacity(max_num) */
    const uint8_t* packets;                     /* [n_images][capacity] */
    const int*     table;                       /* [n_images][table_ints] */
} omni_cam_wire_result;
int     omni_cam_wire(omni_cam* cam, omni_cam_wire_result* out);
/* The whole descriptor inside the unit, behind the stage above.  omni_cam_set_wire_image(cam, with_features, with_image): every following unit runs
 * wire_pack_image_kernel on its SuperPoint stream behind wire_pack_kernel -- with_image: also behind an event the MobileNetVLAD stream records after the JPEG stage
 * (omni_cam_set_jpeg), whose files it reads where that stage left them in HBM -- on the same main images, arrays and records, with the handle's image size as
 * image_width / image_height when the file travels (0 x 0 otherwise: encode_image sets them, loop_cam.cpp:67-70), and copies buffers and sizes into a pinned block of the handle in front of the unit's event.  Both flags 0 switch it off again (the
 * default), and a unit then launches exactly what it launched before; omni_cam_set_wire(cam, 0, ..) switches it off too.  Refused: with the wire stage off,
 * with_image on a handle that encodes no JPEG files or whose JPEG capacity per image is no multiple of 4, a unit in flight; at enqueue, with_image when the JPEG
 * stage was switched off or given another capacity since. */
int     omni_cam_set_wire_image(omni_cam* cam, int with_features, int with_image);
typedef struct omni_cam_wire_image_result {     /* pointers into the handle's pinned host block; valid after omni_cam_wait until the handle's next enqueue */
    int n_images, with_features, with_image;
    int64_t capacity;                           /* omni_wire_image_capacity(max_num, the JPEG stage's capacity or 0) */
    const uint8_t* packets;                     /* [n_images][capacity] */
    const int*     sizes;                       /* [n_images][2] = (offset, size); (0, 0): not sent */
} omni_cam_wire_image_result;
int     omni_cam_wire_image(omni_cam* cam, omni_cam_wire_image_result* out);

/* ---- rows of a mixed detector batch: one contiguous [n_rows][dim] fp32 block in frame order out of rows that lie in three places ------------------------------
 * The plan is csrc/rows_plan.h's: output row r is row table[r].index of the block table[r].source names -- a key-frame unit's rows already in HBM (e.g.
 * MobileNetVLAD's output buffer), rows staged on the host and uploaded next to the table (the global descriptors of frames other drones sent), or zeros.  A bitwise
 * copy: NaN payloads survive.  Source rows may repeat. */
#define OMNI_ROW_UNIT 0
#define OMNI_ROW_STAGED 1
#define OMNI_ROW_ZERO 2
typedef struct omni_row_source { int32_t source; int32_t index; } omni_row_source;
/* One launch per batch, one workgroup of 256 lanes per output row, asynchronous on ctx's stream; table_dev [n_rows], unit_rows_dev [n_unit_rows][dim], staged_rows_dev
 * [n_staged_rows][dim] and out_dev [n_rows][dim] are device memory (a block of no rows may be NULL; out_dev overlaps neither input).  dim % 4 == 0 with all three
 * bases 16-byte aligned moves 16 bytes per lane and step, everything else dwords.  Refused before anything is launched: a null ctx, table or output, a missing
 * block with rows, n_rows < 1, dim < 1, a negative row count, a base that is not 4-byte aligned.  The table is in device memory: whoever made it has checked its
 * entries (omni_rows_assemble_host refuses the same table; csrc/rows_plan.h refusal); an entry out of range reads nothing and its row comes out zero. */
int     omni_rows_assemble_enqueue_dev(omni_ctx* ctx, int64_t n_rows, int dim, const omni_row_source* table_dev, const float* unit_rows_dev, int64_t n_unit_rows,
                                       const float* staged_rows_dev, int64_t n_staged_rows, float* out_dev);
/* csrc/rows_plan.h compiled by g++ into the library: the same arguments in host memory, the same bits, without a GPU and without a context.  Refuses besides: an
 * unknown source, an index outside its block. */
int     omni_rows_assemble_host(int64_t n_rows, int dim, const omni_row_source* table, const float* unit_rows, int64_t n_unit_rows, const float* staged_rows,
                                int64_t n_staged_rows, float* out);
/* PINNED host memory -> device on the context's stream, without waiting (omni_memcpy_d2h_async's twin): src_pinned stays untouched until the copy has run */
int     omni_memcpy_h2d_async(omni_ctx* ctx, void* dst_dev, const void* src_pinned, size_t bytes);

/* ---- pairwise consistency of loop edges (PCM): SwarmLocalOutlierRejection::OutlierRejectionLoopEdgesPCM, swarm_localization/src/swarm_outlier_rejection/
 * swarm_outlier_rejection.cpp:173-298, the consistency rows on the GPU and the clique heuristic on the host -----------------------------------------------------------
 * The arithmetic is csrc/pcm_plan.h's and nothing else restates it: per pair of edges four pose compositions in f64, the log map of
 * LoopGeometry::check_loop_odometry_consistency with the header's OWN arctangent, and the squared Mahalanobis distance under summed diagonal covariances.  swarm_msgs
 * (Swarm::Pose, DroneTrajectory) is not vendored: parity with the reference is unpinned and the header is the specification.  An edge: */
typedef struct omni_pcm_edge {
    int64_t id;
    int32_t drone_a, drone_b;
    double  relative_pose[7];                /* xyz + quaternion wxyz (unit): b's frame in a's, as LoopEdge::relative_pose */
    double  self_pose_a[7], self_pose_b[7];  /* each drone's own odometry pose at the edge's frame */
    double  arc_a, arc_b;                    /* cumulative path length of drone a / b at the edge's frame (metres) */
    double  pos_cov[3], ang_cov[3];          /* the edge's covariance diagonal */
} omni_pcm_edge;
typedef struct omni_pcm_params {
    double pcm_thres;                        /* a pair is consistent iff smd < pcm_thres (0.6: swarm_localization_node.cpp:475) */
    double pos_covariance_per_meter;         /* cov(odom) = |arc difference| * (pos x3, yaw x3)   (0.01 / 0.003: swarm_loop.cpp:247-248) */
    double yaw_covariance_per_meter;
} omni_pcm_params;
#define OMNI_PCM_FULL 100                    /* omni_pcm_add: the handle cannot take n more edges; nothing was changed (a status, not an error: no message is set) */
#define OMNI_PCM_MAX_ADD 64
#define OMNI_PCM_MIN_CAPACITY 64
#define OMNI_PCM_MAX_CAPACITY 32768
#define OMNI_PCM_DEFAULT_CAPACITY 4096
typedef struct omni_pcm omni_pcm;
/* A handle owns one graph in HBM: the edges as structure-of-arrays and a square bit matrix of `capacity` rows of capacity / 64 words (bit j & 63 of word j >> 6 of row
 * i: edges i and j are consistent; the diagonal is 0).  capacity: a multiple of 64 in 64 .. 32768. */
int          omni_pcm_create(omni_ctx* ctx, int capacity, const omni_pcm_params* params, omni_pcm** out);
void         omni_pcm_destroy(omni_pcm* pcm);
int          omni_pcm_size(const omni_pcm* pcm);
int          omni_pcm_capacity(const omni_pcm* pcm);
/* Appends n edges (1 .. 64) as vertices size .. size + n - 1 and compares each with EVERY earlier one, those of this call included: one upload, four launches (the
 * records into the arrays; one lane per pair and a ballot per row word; the mirrored bits; the block that travels back), one download.  Blocking.  degrees_out [size + n]: every vertex's degree
 * after the call.  rows_out [n][capacity / 64]: the new vertices' rows after the call, both triangles.  *kernel_us (may be NULL): the launches' time between two events.
 * Returns OMNI_PCM_FULL when size + n > capacity.  Refused: a null argument, n outside 1..64. */
int          omni_pcm_add(omni_pcm* pcm, const omni_pcm_edge* edges, int n, int32_t* degrees_out, uint64_t* rows_out, float* kernel_us);
/* rows [first, first + n_rows) of the bit matrix and the degrees of the first size vertices (either output may be NULL), for tests */
int          omni_pcm_adjacency(omni_pcm* pcm, int first, int n_rows, uint64_t* rows_out, int32_t* degrees_out);
/* csrc/pcm_plan.h compiled by g++ into the library: edges [n_total] in host memory, vertices [first, n_total) are the new ones.  rows_out [n_total - first][stride_words]
 * (stride_words * 64 >= n_total): their rows, both triangles; degree_add [n_total]: the consistent pairs this call found at each vertex (first == 0: the degrees).
 * smd_out (may be NULL) [n_total - first][n_total]: the distance of every pair (i, j < i), NaN bits included, 0 where same_robot_pair is 0 or j >= i.  No GPU, no context. */
int          omni_pcm_rows_host(const omni_pcm_edge* edges, int n_total, int first, const omni_pcm_params* params, int stride_words, uint64_t* rows_out,
                                int32_t* degree_add, double* smd_out);
/* The clique heuristic of csrc/pcm_plan.h on the rows of n vertices (row v at rows + v * stride_words; bits at or above n must be 0): clique_out [n] receives the
 * vertices of the clique found, the start vertex first, *size_out their number. */
int          omni_pcm_max_clique_host(const uint64_t* rows, int n, int stride_words, int32_t* clique_out, int* size_out);
/* the header's arctangent (tests): atan2(y, x) */
double       omni_pcm_atan2(double y, double x);

/* ---- 4-DoF pose graph over odometry and loop edges: the loop + ego-motion part of swarm_localization's sliding-window problem (swarm_localization_solver.cpp
 * :1064-1100, :1156-1213, :1668-1712; RelativePoseFactor4d of swarm_localization_factors.hpp) ---------------------------------------------------------------------------
 * The arithmetic is csrc/pgo_plan.h's and nothing else restates it: residual r = sqrt_inf o (z - DeltaPose(p_i, p_j)) with the header's OWN sine and cosine, analytic
 * Jacobians, Huber(1) as Ceres corrects a block, and Levenberg-Marquardt over block-Jacobi conjugate gradients with every sum in a fixed order.  Ceres, Eigen and
 * swarm_msgs are not vendored: parity with the reference is unpinned and the header is the specification.  A pose is double[4]: x y z yaw. */
typedef struct omni_pgo_edge {
    int32_t i, j;                            /* the two poses: z measures DeltaPose(pose i, pose j) */
    double  z[4];                            /* x y z yaw of pose j in pose i's yaw frame */
    double  sqrt_inf[4];                     /* the diagonal of the square-root information: 1 / sqrt(cov) over (pos_cov xyz, ang_cov[2]) */
    int32_t robust;                          /* != 0: HuberLoss(1.0) (loop edges); 0: no loss (ego motion) */
    int32_t reserved;
} omni_pgo_edge;
typedef struct omni_pgo_params {
    int32_t max_iterations;                  /* outer Levenberg-Marquardt iterations (50) */
    int32_t max_cg_iterations;               /* conjugate-gradient steps per linear solve; 0: 4 x the number of free poses */
    int32_t max_lambda_retries;              /* enlargements of lambda after a rejected step before the solve gives up (16) */
    int32_t reserved;
    double  initial_lambda;                  /* 1e-4 */
    double  function_tolerance;              /* CONVERGED when an accepted step lowers the cost by no more than this x the cost (1e-6) */
    double  parameter_tolerance;             /* CONVERGED when |step| <= this x (|free poses| + this) (1e-8) */
    double  cg_tolerance;                    /* a linear solve ends when r.z <= this^2 x its first value (1e-6) */
} omni_pgo_params;
typedef struct omni_pgo_stats {
    double  initial_cost, final_cost;        /* the sum over edges of rho(|r|^2) / 2 at the start and at the poses returned */
    int32_t iterations, cg_iterations;       /* outer iterations begun; conjugate-gradient steps over all linear solves */
    int32_t status;                          /* OMNI_PGO_* */
    int32_t reserved;
} omni_pgo_stats;
#define OMNI_PGO_CONVERGED 0
#define OMNI_PGO_MAX_ITERATIONS 1            /* a cap was reached: max_iterations, or max_lambda_retries without an accepted step */
#define OMNI_PGO_NONFINITE 2                 /* a NaN or inf in a cost or a step: the poses are returned as they came */
#define OMNI_PGO_EMPTY 3                     /* no free pose with an edge, or no edge: the poses are returned as they came, both costs are 0 */
#define OMNI_PGO_MAX_POSES 4096
#define OMNI_PGO_MAX_EDGES 16384
#define OMNI_PGO_MAX_STARTS 64
typedef struct omni_pgo omni_pgo;
int          omni_pgo_default_params(omni_pgo_params* out);
int          omni_pgo_create(omni_ctx* ctx, omni_pgo** out);
void         omni_pgo_destroy(omni_pgo* pgo);
/* Solves n_starts (1 .. 64) initial pose sets of ONE graph, one workgroup per start, in one launch between one upload and one download (solve_with_multiple_init,
 * swarm_localization_solver.cpp:781-846).  poses_in / poses_out [n_starts][n_poses][4]; fixed [n_poses] bytes (!= 0: the pose is constant); edges [n_edges];
 * stats_out [n_starts]; *best: the start with the lowest final cost among those that ended CONVERGED or MAX_ITERATIONS, the lower index on a tie, -1 when there is
 * none; *kernel_us (may be NULL): the launch's time between two events.  Blocking.  Refused before any launch: a null argument, n_poses outside 1..4096, n_edges
 * outside 0..16384, n_starts outside 1..64, an edge whose i or j is outside 0..n_poses-1 or whose i equals j, a parameter that is negative or not finite. */
int          omni_pgo_solve_multi(omni_pgo* pgo, const omni_pgo_params* params, const double* poses_in, const uint8_t* fixed, const omni_pgo_edge* edges, int n_poses,
                                  int n_edges, int n_starts, double* poses_out, omni_pgo_stats* stats_out, int* best, float* kernel_us);
/* csrc/pgo_plan.h compiled by g++ into the library: the same arguments, the same refusals, the same bits, one start after the other on the calling thread.  No GPU,
 * no context. */
int          omni_pgo_solve_host(const omni_pgo_params* params, const double* poses_in, const uint8_t* fixed, const omni_pgo_edge* edges, int n_poses, int n_edges,
                                 int n_starts, double* poses_out, omni_pgo_stats* stats_out, int* best);
/* For tests: per edge the residual after the loss's correction res_out [n_edges][4], the corrected Jacobians jac_i_out / jac_j_out [n_edges][4][4] (row = residual,
 * column = x y z yaw of pose i / j) and the cost cost_out [n_edges]; any output may be NULL.  The refusals of the graph are those above. */
int          omni_pgo_residuals_host(const double* poses, const omni_pgo_edge* edges, int n_poses, int n_edges, double* res_out, double* jac_i_out, double* jac_j_out,
                                     double* cost_out);
/* For tests: the incidence lists of pgo::plan_graph.  offsets_out [n_poses + 1], incident_out [2 n_edges] (2 x edge + side, side 1: the pose is the edge's j),
 * active_out [n_poses] bytes (free and with an edge), *n_active_out their number. */
int          omni_pgo_plan_graph_host(const uint8_t* fixed, const omni_pgo_edge* edges, int n_poses, int n_edges, int32_t* offsets_out, int32_t* incident_out,
                                      uint8_t* active_out, int* n_active_out);
/* the header's sine and cosine, NormalizeAngle and the fixed-shape sum (tests) */
void         omni_pgo_sincos(double yaw, double* sin_out, double* cos_out);
double       omni_pgo_normalize_angle(double a);
double       omni_pgo_sum_host(const double* v, int n);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HIP_H */
