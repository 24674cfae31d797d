// omni_cam_*: the CNN + matching part of one fisheye key frame as ONE asynchronous unit -- the device-side work of
//   LoopCam::on_flattened_images / generate_stereo_image_descriptor / extractor_img_desc_deepnet / match_HFNet_local_features
//   (swarm_loop/src/loop_cam.cpp:178-229, 341-523, 525-585, 141-174).
// The reference runs 8 SuperPoint + 4 MobileNetVLAD engine calls and 4 BFMatcher calls strictly one after another, each
// with its own H2D / D2H and a blocking stream sync.  Here enqueue() puts on the GPU, without any host
// synchronisation:  SuperPoint(2n images) -> BF cross-check of the n up/down descriptor sets   on the SuperPoint stream,
//                   MobileNetVLAD(n images)                                                    on the MobileNetVLAD stream,
// plus the D2H copies of every result into ONE pinned host block, and records one event per stream.  wait() blocks on the
// two events and hands out pointers into the pinned block (valid until the next enqueue on this handle).  Several handles
// (each with its own SuperPoint / MobileNetVLAD instance) keep several key frames in flight.
#include "common.h"
#include "camera_plan.h"
#include <string.h>

struct omni_cam {
    omni_sp* sp = nullptr;
    omni_vlad* vlad = nullptr;
    omni_ctx *c1 = nullptr, *c2 = nullptr;
    int n = 0, n_cap = 0, cams = 2, M = 0, D = 0, out_dim = 0, bf_mode = 0, W = 0, H = 0;   // cams: 2 = up + down camera per direction, 1 = one camera (no stereo match)
      // n: directions of the NEXT enqueue (omni_cam_set_active), n_cap: what the handle and its networks were created for
      // W x H: the size the SuperPoint handle (and MobileNetVLAD) was created for
    int *d_qidx = nullptr, *d_tidx = nullptr, *d_nm = nullptr;
    float* d_dist = nullptr;
    const float *kps_dev = nullptr, *desc_dev = nullptr, *sc_dev = nullptr, *g_dev = nullptr;
    const int* n_dev = nullptr;
    char* host = nullptr;
    size_t off_kps = 0, off_n = 0, off_desc = 0, off_sc = 0, off_g = 0, off_q = 0, off_t = 0, off_d = 0, off_nm = 0, host_bytes = 0;
    hipEvent_t e1 = nullptr, e2 = nullptr, e_up = nullptr;
    uint8_t* d_gray = nullptr;        // staging for omni_cam_enqueue_host: the key frame's images, rows packed to `width`
    size_t d_gray_bytes = 0;
    size_t input_bytes = 0;           // what the last unit read from d_gray (0: it read a caller's buffer): omni_cam_get_input
    uint8_t* d_raw = nullptr;         // staging for omni_cam_enqueue_fisheye_host / _raw_host: the raw frames of the up (left) cameras, then of the down (right) cameras
                                      // (uploaded, or decoded there: omni_cam_enqueue_jpeg_host, omni_cam_enqueue_fisheye_jpeg_host)
    size_t d_raw_bytes = 0;
    bool pending = false;
    // stereo landmarks inside the unit (omni_cam_set_stereo_model; landmarks.hip): the model, the NEXT unit's poses (pinned staging in `host`, uploaded at enqueue),
    // the stage's device outputs -- laid out as the key points, [up images | down images] of the active size
    bool lm_on = false, lm_unit = false;      // lm_unit: the unit enqueued last ran the stage (omni_cam_landmarks)
    omni_stereo_model model;
    omni_camera_model camera = omni::cam::ideal();      // the lens of the stage's lifts (omni_cam_set_camera_model): kept over omni_cam_set_stereo_model
    int n_poses = 0;                          // key frames omni_cam_set_poses set since the last unit (0: none)
    int lm_n = 0;                             // directions of the unit that ran the stage last
    double* d_poses = nullptr;
    char* d_lm = nullptr;                     // ONE block laid out as host + off_norm .. off_lm_end: norm2d | landmarks_3d | flags | count_3d (one copy down)
    size_t off_poses = 0, off_norm = 0, off_l3d = 0, off_flag = 0, off_cnt = 0, off_lm_end = 0;
    // depth landmarks inside a MONO unit (omni_cam_set_depth_model; depth_landmarks.hip): the same poses staging, the same block of four arrays (one image per
    // direction, count_3d per image), plus the NEXT unit's depth frames -- h_depth (pinned): [n_cap] frames of depth_width x depth_height u16, rows packed, then
    // (at depth_have) have [n_cap] u8; d_depth: the same layout in HBM.  omni_cam_set_depth_dev borrows the frames instead (depth_ext) and sets have only
    bool dp_on = false;
    omni_depth_model dmodel;
    omni_camera_model dcamera = omni::cam::ideal();
    int n_depth = 0;                          // images omni_cam_set_depth_host / _dev set since the last unit (0: none)
    const uint16_t* depth_ext = nullptr;      // != nullptr: the next unit reads these frames (HBM, borrowed until omni_cam_wait) with depth_ext_stride
    int depth_ext_stride = 0;
    uint8_t *h_depth = nullptr, *d_depth = nullptr;
    size_t depth_have = 0, depth_bytes = 0;
    // send_img inside the unit (omni_cam_set_jpeg; jpeg.hip): the unit's main images [0, n) as JPEG files, on the MobileNetVLAD stream.  d_jpeg / h_jpeg: the
    // images' bytes [n_cap][jpeg_cap], then (at jpeg_meta) sizes [n_cap] and statuses [n_cap] -- a block of its own, pinned on the host side
    omni_jpeg* jpeg = nullptr;
    int jpeg_quality = 0;                     // 0: the stage is off
    int64_t jpeg_cap = 0;
    size_t jpeg_meta = 0;
    uint8_t *d_jpeg = nullptr, *h_jpeg = nullptr;
    bool jpeg_unit = false;                   // the unit enqueued last ran the stage (omni_cam_jpeg)
    int jpeg_n = 0;                           // main images of that unit
    // is_compressed_images (omni_cam_enqueue_jpeg_host; jpeg_dec.hip): the unit's frames arrive as JPEG files and are decoded on the SuperPoint stream in front of
    // the resize.  The decoder is made at first use for the frames' size; statuses [cams * n_cap] go down into a pinned block of their own
    omni_jpegdec* jdec = nullptr;
    int jdec_w = 0, jdec_h = 0, jdec_max = 0;      // jdec_max: pictures the decoder was made for
    int *d_jdec_status = nullptr, *h_jdec_status = nullptr;
    int jdec_n = 0;                           // frames of the unit enqueued last if it came as files (omni_cam_jpegdec_status), else 0
    std::mutex mu;
};

extern "C" {

static omni_cam* cam_create(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_dirs, int cams, int max_num, int global_dim, int bf_mode);

omni_cam* omni_cam_create(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_dirs, int max_num, int global_dim,
                          int bf_mode) {
    return cam_create(sp_ctx, sp, vlad_ctx, vlad, n_dirs, 2, max_num, global_dim, bf_mode);
}

// CameraConfig::PINHOLE_DEPTH (loop_cam.cpp:190-194, generate_gray_depth_image_descriptor :231-339): ONE camera per image, both networks on every
// image, no up/down match; the landmarks come from the depth image: inside the unit with a depth model (omni_cam_set_depth_model, depth_landmarks.hip), else on
// the host (loop_geometry.hpp fill_depth_landmarks)
omni_cam* omni_cam_create_mono(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_images, int max_num, int global_dim) {
    return cam_create(sp_ctx, sp, vlad_ctx, vlad, n_images, 1, max_num, global_dim, 0);
}

static omni_cam* cam_create(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_dirs, int cams, int max_num, int global_dim,
                            int bf_mode) {
    if (!sp_ctx || !sp || !vlad_ctx || !vlad) { omni::set_error("null handle"); return nullptr; }
    if (n_dirs < 1 || n_dirs > 64 || max_num < 1 || max_num > 1024 || global_dim < 1) { omni::set_error("bad n_dirs/max_num/global_dim"); return nullptr; }
    if (sp_ctx->device != vlad_ctx->device) { omni::set_error("SuperPoint and MobileNetVLAD contexts are on different devices"); return nullptr; }
    (void)hipSetDevice(sp_ctx->device);
    omni_cam* c = new omni_cam();
    c->sp = sp; c->vlad = vlad; c->c1 = sp_ctx; c->c2 = vlad_ctx; c->n = c->n_cap = n_dirs; c->cams = cams; c->M = max_num; c->D = omni_sp_desc_dim(sp);
    c->out_dim = global_dim; c->bf_mode = bf_mode;
    (void)omni_sp_image_size(sp, &c->W, &c->H);
    const size_t n = n_dirs, M = max_num, D = c->D, ni = (size_t)cams * n;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    c->off_kps = o; o += al(ni * M * 2 * 4);
    c->off_n = o;   o += al(ni * 4);
    c->off_desc = o; o += al(ni * M * D * 4);
    c->off_sc = o;  o += al(ni * M * 4);
    c->off_g = o;   o += al(n * (size_t)global_dim * 4);
    c->off_q = o;   o += al(n * M * 4);
    c->off_t = o;   o += al(n * M * 4);
    c->off_d = o;   o += al(n * M * 4);
    c->off_nm = o;  o += al(n * 4);
    {                                                                         // the landmark stage's part of the block (a few kilobytes per image; mono: the depth landmarks')
        c->off_poses = o; o += al(n * 7 * 8);
        c->off_norm = o;  o += al(ni * M * 2 * 4);
        c->off_l3d = o;   o += al(ni * M * 3 * 4);
        c->off_flag = o;  o += al(ni * M);
        c->off_cnt = o;   o += al(n * 4);
        c->off_lm_end = o;
    }
    c->host_bytes = o;
    bool ok = hipHostMalloc((void**)&c->host, o, hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void**)&c->d_qidx, n * M * 4) == hipSuccess && hipMalloc((void**)&c->d_tidx, n * M * 4) == hipSuccess &&
              hipMalloc((void**)&c->d_dist, n * M * 4) == hipSuccess && hipMalloc((void**)&c->d_nm, n * 4) == hipSuccess &&
              hipMalloc((void**)&c->d_poses, n * 7 * 8) == hipSuccess && hipMalloc((void**)&c->d_lm, c->off_lm_end - c->off_norm) == hipSuccess &&
              hipEventCreateWithFlags(&c->e1, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->e2, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->e_up, hipEventDisableTiming) == hipSuccess &&
              omni_sp_dev_outputs(sp, &c->kps_dev, &c->n_dev, &c->desc_dev, &c->sc_dev) == OMNI_OK &&
              omni_vlad_dev_output(vlad, &c->g_dev) == OMNI_OK;
    if (!ok) { omni::set_error("omni_cam_create: allocation failed"); omni_cam_destroy(c); return nullptr; }
    memset(c->host, 0, o);
    return c;
}

void omni_cam_destroy(omni_cam* c) {
    if (!c) return;
    (void)hipSetDevice(c->c1->device);
    (void)hipStreamSynchronize(c->c1->stream);
    (void)hipStreamSynchronize(c->c2->stream);
    void* ptrs[] = {c->d_qidx, c->d_tidx, c->d_dist, c->d_nm, c->d_gray, c->d_raw, c->d_poses, c->d_lm, c->d_depth};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (c->jpeg) omni_jpeg_destroy(c->jpeg);
    if (c->jdec) omni_jpegdec_destroy(c->jdec);
    if (c->d_jdec_status) (void)hipFree(c->d_jdec_status);
    if (c->h_jdec_status) (void)hipHostFree(c->h_jdec_status);
    if (c->d_jpeg) (void)hipFree(c->d_jpeg);
    if (c->h_jpeg) (void)hipHostFree(c->h_jpeg);
    if (c->h_depth) (void)hipHostFree(c->h_depth);
    if (c->host) (void)hipHostFree(c->host);
    if (c->e1) (void)hipEventDestroy(c->e1);
    if (c->e2) (void)hipEventDestroy(c->e2);
    if (c->e_up) (void)hipEventDestroy(c->e_up);
    delete c;
}

static int cam_enqueue_locked(omni_cam* c, const uint8_t* gray_dev, int stride, int fisheye_mask);

// a staging buffer of the handle (d_gray, d_raw) that holds `need` bytes: grown behind whatever the unit's two streams still read from the old one
static int cam_staging(omni_cam* c, uint8_t*& buf, size_t& have, size_t need) {
    if (have >= need) return OMNI_OK;
    (void)hipStreamSynchronize(c->c1->stream);
    (void)hipStreamSynchronize(c->c2->stream);
    if (buf) (void)hipFree(buf);
    buf = nullptr; have = 0;
    OMNI_HIP_TRY(hipMalloc((void**)&buf, need));
    have = need;
    return OMNI_OK;
}

// with a stereo model set, a unit needs the poses of ITS key frames: checked by every enqueue entry before anything is enqueued (c->mu held)
static int cam_poses_check(omni_cam* c) {
    if (c->dp_on) {                                                           // a mono unit with a depth model: the poses AND the depth frames of its images, one key frame per image
        OMNI_REQUIRE(c->n_poses > 0, OMNI_ERR_INVALID, "a depth model is set but the unit's poses are not (omni_cam_set_poses before every enqueue)");
        OMNI_REQUIRE(c->n_poses == c->n, OMNI_ERR_INVALID, "poses of %d key frames for a unit of %d images (omni_cam_set_poses, omni_cam_set_active)", c->n_poses, c->n);
        OMNI_REQUIRE(c->n_depth > 0, OMNI_ERR_INVALID, "a depth model is set but the unit's depth frames are not (omni_cam_set_depth_host / _dev before every enqueue)");
        OMNI_REQUIRE(c->n_depth == c->n, OMNI_ERR_INVALID, "depth frames of %d images for a unit of %d images (omni_cam_set_depth_host / _dev, omni_cam_set_active)", c->n_depth, c->n);
        return OMNI_OK;
    }
    if (!c->lm_on) return OMNI_OK;
    OMNI_REQUIRE(c->n_poses > 0, OMNI_ERR_INVALID, "a stereo model is set but the unit's poses are not (omni_cam_set_poses before every enqueue)");
    OMNI_REQUIRE(c->n_poses * c->model.dirs_per_keyframe == c->n, OMNI_ERR_INVALID, "poses of %d key frames x %d directions for a unit of %d (omni_cam_set_poses, omni_cam_set_active)",
                 c->n_poses, c->model.dirs_per_keyframe, c->n);
    return OMNI_OK;
}

int omni_cam_enqueue_dev(omni_cam* c, const uint8_t* gray_dev, int stride, int fisheye_mask) {
    omni::TraceRange trace_range("omni_cam_enqueue_dev");
    OMNI_REQUIRE(c && gray_dev, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_poses_check(c))) return rc;
    (void)hipSetDevice(c->c1->device);
    return cam_enqueue_locked(c, gray_dev, stride, fisheye_mask);
}

int omni_cam_enqueue_host(omni_cam* c, const uint8_t* gray_host, int stride, int width, int height, int fisheye_mask) {
    omni::TraceRange trace_range("omni_cam_enqueue_host (upload + unit)");
    OMNI_REQUIRE(c && gray_host, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(width > 0 && height > 0 && stride >= width, OMNI_ERR_INVALID, "bad image geometry %dx%d stride %d", width, height, stride);
    // the networks read cams * n images of THEIR size from the staging buffer: any other size would run them past its end
    OMNI_REQUIRE(width == c->W && height == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_host: images are %dx%d but the networks were created for %dx%d", width, height, c->W, c->H);
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_poses_check(c))) return rc;
    (void)hipSetDevice(c->c1->device);
    if ((rc = cam_staging(c, c->d_gray, c->d_gray_bytes, (size_t)c->cams * c->n * width * height))) return rc;
    // the reference uploads one image per engine call and blocks (tensorrt_generic.cpp:58-75); here the key frame's 2n images go up as one
    // asynchronous copy on the SuperPoint stream (pinned source: the copy engine runs it next to the other pipelines' kernels) and the
    // MobileNetVLAD stream waits for it on the device
    // (two copies for a stereo rig: MobileNetVLAD only reads the up cameras' images -- the first half -- and starts as soon as they are up, while the
    // down cameras' half is still on the bus; SuperPoint's stream carries both copies and so waits for all of it)
    // (packed rows -- stride == width, what the key-frame pipeline hands over -- go up as plain 1-D copies: 56 GB/s against 50 GB/s for the 2-D form of the same
    // bytes, tools/probes/h2d_probe.hip)
    const size_t rows_up = (size_t)c->n * height, rows_all = (size_t)c->cams * c->n * height;
    auto upload = [&](size_t row0, size_t rows) -> hipError_t {
        if (stride == width) return hipMemcpyAsync(c->d_gray + row0 * width, gray_host + row0 * width, rows * width, hipMemcpyHostToDevice, c->c1->stream);
        return hipMemcpy2DAsync(c->d_gray + row0 * width, (size_t)width, gray_host + row0 * stride, (size_t)stride, (size_t)width, rows, hipMemcpyHostToDevice, c->c1->stream);
    };
    OMNI_HIP_TRY(upload(0, rows_up));
    OMNI_HIP_TRY(hipEventRecord(c->e_up, c->c1->stream));
    OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->e_up, 0));
    if (rows_all > rows_up) OMNI_HIP_TRY(upload(rows_up, rows_all - rows_up));
    return cam_enqueue_locked(c, c->d_gray, width, fisheye_mask);
}

// The same from SEGMENTS of host memory: the up cameras' n images are the concatenation of n_up parts (up[i]: up_images[i] images, rows packed), the down
// cameras' likewise (n_down = 0 for a mono handle).  What a key-frame loop needs to cut a run of key frames into units of ITS choice out of blocks laid out
// for another unit size (KeyframePipeline::run): every part is one asynchronous 1-D copy; MobileNetVLAD starts behind the up cameras' parts.
int omni_cam_enqueue_host_parts(omni_cam* c, const uint8_t* const* up, const int* up_images, int n_up, const uint8_t* const* down, const int* down_images, int n_down,
                                int width, int height, int fisheye_mask) {
    omni::TraceRange trace_range("omni_cam_enqueue_host_parts (upload + unit)");
    OMNI_REQUIRE(c && up && up_images && n_up > 0 && (n_down == 0 || (down && down_images)), OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);                 // (before anything of the handle is read: omni_cam_set_active writes c->n under this lock)
    OMNI_REQUIRE(width == c->W && height == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_host_parts: images are %dx%d but the networks were created for %dx%d", width, height, c->W, c->H);
    int nu = 0, nd = 0;
    for (int i = 0; i < n_up; ++i) { OMNI_REQUIRE(up[i] && up_images[i] > 0, OMNI_ERR_INVALID, "omni_cam_enqueue_host_parts: empty part"); nu += up_images[i]; }
    for (int i = 0; i < n_down; ++i) { OMNI_REQUIRE(down[i] && down_images[i] > 0, OMNI_ERR_INVALID, "omni_cam_enqueue_host_parts: empty part"); nd += down_images[i]; }
    OMNI_REQUIRE(nu == c->n && nd == (c->cams - 1) * c->n, OMNI_ERR_INVALID, "omni_cam_enqueue_host_parts: %d + %d images for a unit of %d x %d", nu, nd, c->cams, c->n);
    int rc;
    if ((rc = cam_poses_check(c))) return rc;
    (void)hipSetDevice(c->c1->device);
    const size_t img = (size_t)width * height;
    if ((rc = cam_staging(c, c->d_gray, c->d_gray_bytes, (size_t)c->cams * c->n * img))) return rc;
    size_t at = 0;
    for (int i = 0; i < n_up; ++i) { OMNI_HIP_TRY(hipMemcpyAsync(c->d_gray + at, up[i], up_images[i] * img, hipMemcpyHostToDevice, c->c1->stream)); at += up_images[i] * img; }
    OMNI_HIP_TRY(hipEventRecord(c->e_up, c->c1->stream));
    OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->e_up, 0));
    for (int i = 0; i < n_down; ++i) { OMNI_HIP_TRY(hipMemcpyAsync(c->d_gray + at, down[i], down_images[i] * img, hipMemcpyHostToDevice, c->c1->stream)); at += down_images[i] * img; }
    return cam_enqueue_locked(c, c->d_gray, width, fisheye_mask);
}

// A key frame's two RAW fisheye frames instead of its flattened views: the remap (flatten.hip) runs inside the unit, on the SuperPoint stream, and writes the
// unit's own input block.  n_keyframes up frames and as many down frames (u8, src_stride, frame i at + i * src_stride * source height); `up` / `down` hold the
// two cameras' maps, of which views [first_view, n_views) are the unit's directions: n_keyframes * (n_views - first_view) = the unit's active size, each view of
// the networks' size.  The maps are read on the unit's streams, never on the flatten objects' own: keep both objects alive until omni_cam_wait.
static int cam_fisheye_check(omni_cam* c, const omni_flatten* up, const omni_flatten* down, int src_stride, int n_keyframes, int first_view, int* dirs) {
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: a mono handle has no up / down camera pair");
    OMNI_REQUIRE(n_keyframes >= 1 && first_view >= 0 && first_view < up->n_views && up->n_views == down->n_views, OMNI_ERR_INVALID,
                 "omni_cam_enqueue_fisheye: %d key frames, first view %d of %d (up) / %d (down)", n_keyframes, first_view, up->n_views, down->n_views);
    *dirs = up->n_views - first_view;
    OMNI_REQUIRE((int64_t)n_keyframes * *dirs == c->n, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: %d key frames x %d directions for a unit of %d (omni_cam_set_active)",
                 n_keyframes, *dirs, c->n);
    for (const omni_flatten* f : {up, down}) {
        OMNI_REQUIRE(f->ctx->device == c->c1->device, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: maps on device %d, the unit on device %d", f->ctx->device, c->c1->device);
        OMNI_REQUIRE(src_stride >= f->src_w, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: stride %d for frames %d wide", src_stride, f->src_w);
        for (int v = first_view; v < f->n_views; ++v)
            OMNI_REQUIRE(f->vw[v] == c->W && f->vh[v] == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: view %d is %dx%d but the networks were created for %dx%d", v,
                         f->vw[v], f->vh[v], c->W, c->H);
    }
    return cam_poses_check(c);
}

// up camera first and MobileNetVLAD behind it, then the down camera: the overlap omni_cam_enqueue_host arranges for its two uploads.  *_host != nullptr: the raw
// frames go up first, one asynchronous copy per camera in front of its remap
static int cam_fisheye_locked(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* up_dev, const uint8_t* down_dev, const uint8_t* up_host,
                              const uint8_t* down_host, int src_stride, int n_keyframes, int first_view, int fisheye_mask) {
    int rc, dirs = 0;
    if ((rc = cam_fisheye_check(c, up, down, src_stride, n_keyframes, first_view, &dirs))) return rc;
    (void)hipSetDevice(c->c1->device);
    const size_t half = (size_t)c->n * c->W * c->H;
    if ((rc = cam_staging(c, c->d_gray, c->d_gray_bytes, 2 * half))) return rc;
    auto raw_bytes = [&](const omni_flatten* f) { return ((size_t)n_keyframes * f->src_h - 1) * src_stride + f->src_w; };      // (the last row may end at its width)
    const size_t down_at = (raw_bytes(up) + 255) & ~(size_t)255;
    if (up_host) {
        if ((rc = cam_staging(c, c->d_raw, c->d_raw_bytes, down_at + raw_bytes(down)))) return rc;
        up_dev = c->d_raw; down_dev = c->d_raw + down_at;
    }
    hipStream_t s1 = c->c1->stream;
    if (up_host) OMNI_HIP_TRY(hipMemcpyAsync(c->d_raw, up_host, raw_bytes(up), hipMemcpyHostToDevice, s1));
    if ((rc = omni::flatten_unit_launch(up, s1, up_dev, src_stride, n_keyframes, first_view, dirs, c->W, c->H, fisheye_mask, c->d_gray))) return rc;
    OMNI_HIP_TRY(hipEventRecord(c->e_up, s1));
    OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->e_up, 0));
    if (down_host) OMNI_HIP_TRY(hipMemcpyAsync(c->d_raw + down_at, down_host, raw_bytes(down), hipMemcpyHostToDevice, s1));
    if ((rc = omni::flatten_unit_launch(down, s1, down_dev, src_stride, n_keyframes, first_view, dirs, c->W, c->H, fisheye_mask, c->d_gray + half))) return rc;
    return cam_enqueue_locked(c, c->d_gray, c->W, fisheye_mask);
}

int omni_cam_enqueue_fisheye_dev(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* up_dev, const uint8_t* down_dev, int src_stride, int n_keyframes,
                                 int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c && up && down && up_dev && down_dev, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_fisheye_dev (flatten + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_fisheye_locked(c, up, down, up_dev, down_dev, nullptr, nullptr, src_stride, n_keyframes, first_view, fisheye_mask);
}

int omni_cam_enqueue_fisheye_host(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* up_host, const uint8_t* down_host, int src_stride, int n_keyframes,
                                  int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c && up && down && up_host && down_host, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_fisheye_host (upload + flatten + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_fisheye_locked(c, up, down, nullptr, nullptr, up_host, down_host, src_stride, n_keyframes, first_view, fisheye_mask);
}

// the handle's decoder, made at first use for frames of sw x sh (and made again for another size or more pictures); its statuses [cams * n_cap] go down into a
// pinned block of their own.  c->mu held, no unit in flight
static int cam_jdec_ensure(omni_cam* c, int sw, int sh, int max_images) {
    if (!c->jdec || c->jdec_w != sw || c->jdec_h != sh || c->jdec_max < max_images) {
        if (c->jdec) omni_jpegdec_destroy(c->jdec);
        c->jdec = nullptr;
        const int64_t cap = (int64_t)sw * sh / 2 > 1024 ? (int64_t)sw * sh / 2 : 1024;       // (a larger file is decoded on the calling thread: same pixels)
        c->jdec = omni_jpegdec_create(c->c1, sw, sh, max_images, cap);
        if (!c->jdec) return OMNI_ERR_INVALID;
        c->jdec_w = sw; c->jdec_h = sh; c->jdec_max = max_images;
    }
    if (!c->d_jdec_status) {
        OMNI_HIP_TRY(hipMalloc((void**)&c->d_jdec_status, (size_t)c->cams * c->n_cap * sizeof(int)));
        OMNI_HIP_TRY(hipHostMalloc((void**)&c->h_jdec_status, (size_t)c->cams * c->n_cap * sizeof(int), hipHostMallocDefault));
    }
    return OMNI_OK;
}

// The same with each camera's n_keyframes RAW frames given as JPEG files (the compressed fisheye topics the reference's upstream, VINS-Fisheye, decodes in front of
// its own flattening): ONE decode of [up frames | down frames] (jpeg_dec.hip) on the SuperPoint stream into d_raw, rows packed, where omni_cam_enqueue_fisheye_host
// uploads them; the two remaps and the unit follow as there, MobileNetVLAD behind the up camera's views.  A CORRUPT file is an all-zero frame and so all-zero views.
int omni_cam_enqueue_fisheye_jpeg_host(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* const* up_files, const int64_t* up_sizes,
                                       const uint8_t* const* down_files, const int64_t* down_sizes, int n_keyframes, int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c && up && down && up_files && up_sizes && down_files && down_sizes, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_fisheye_jpeg_host (decode + flatten + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye_jpeg_host with a unit in flight (omni_cam_wait first)");
    c->jdec_n = 0;                                                            // (as omni_cam_enqueue_jpeg_host)
    OMNI_REQUIRE(up->src_w == down->src_w && up->src_h == down->src_h, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye_jpeg_host: up frames of %dx%d, down frames of %dx%d (one decoder: one size)",
                 up->src_w, up->src_h, down->src_w, down->src_h);
    const int sw = up->src_w, sh = up->src_h;
    int rc, dirs = 0;
    if ((rc = cam_fisheye_check(c, up, down, sw, n_keyframes, first_view, &dirs))) return rc;
    int row0 = 0, row1 = 0;                                                   // flatten_unit_launch's own refusal, in front of the decode
    omni_fisheye_mask_rows(c->H, fisheye_mask, &row0, &row1);
    OMNI_REQUIRE(c->W % 4 == 0 && row1 == c->H && sw >= 2, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye_jpeg_host: %dx%d views, frames %d wide", c->W, c->H, sw);
    (void)hipSetDevice(c->c1->device);
    if ((rc = cam_jdec_ensure(c, sw, sh, 2 * (c->n_cap / dirs)))) return rc;
    const int nf = 2 * n_keyframes;
    const size_t half = (size_t)c->n * c->W * c->H, frame = (size_t)sw * sh;
    if ((rc = cam_staging(c, c->d_gray, c->d_gray_bytes, 2 * half))) return rc;
    if ((rc = cam_staging(c, c->d_raw, c->d_raw_bytes, (size_t)nf * frame))) return rc;
    std::vector<const uint8_t*> files(up_files, up_files + n_keyframes);
    std::vector<int64_t> sizes(up_sizes, up_sizes + n_keyframes);
    files.insert(files.end(), down_files, down_files + n_keyframes);
    sizes.insert(sizes.end(), down_sizes, down_sizes + n_keyframes);
    hipStream_t s1 = c->c1->stream;
    // (an UNSUPPORTED file or a picture of another size is refused here, nothing enqueued)
    if ((rc = omni::jpegdec_enqueue_on(c->jdec, s1, files.data(), sizes.data(), nf, c->d_raw, sw, c->d_jdec_status))) return rc;
    OMNI_HIP_TRY(hipMemcpyAsync(c->h_jdec_status, c->d_jdec_status, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost, s1));
    if ((rc = omni::flatten_unit_launch(up, s1, c->d_raw, sw, n_keyframes, first_view, dirs, c->W, c->H, fisheye_mask, c->d_gray))) return rc;
    OMNI_HIP_TRY(hipEventRecord(c->e_up, s1));
    OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->e_up, 0));
    if ((rc = omni::flatten_unit_launch(down, s1, c->d_raw + (size_t)n_keyframes * frame, sw, n_keyframes, first_view, dirs, c->W, c->H, fisheye_mask, c->d_gray + half)))
        return rc;
    rc = cam_enqueue_locked(c, c->d_gray, c->W, fisheye_mask);
    c->jdec_n = rc == OMNI_OK ? nf : 0;
    return rc;
}

// A key frame's two RAW stereo-pinhole frames (CameraConfig::STEREO_PINHOLE: generate_stereo_image_descriptor for ONE direction, loop_cam.cpp:189-196) of the
// camera's size instead of network-size images: the resize both reference engines run on the host in front of their networks (resize.hip) runs inside the unit,
// on the SuperPoint stream, and writes the unit's own input block.  With one direction the unit's active size counts key frames: n_keyframes left frames (the
// "up" role) and as many right frames.  The tables are read on the unit's streams, never on the resize object's own: keep it alive until omni_cam_wait.
static int cam_raw_check(omni_cam* c, const omni_resize* r, int src_stride, int n_keyframes) {
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: a mono handle has no left / right camera pair");
    OMNI_REQUIRE(r->dst_w == c->W && r->dst_h == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: the resize object makes %dx%d images but the networks were created for %dx%d",
                 r->dst_w, r->dst_h, c->W, c->H);
    OMNI_REQUIRE(r->ctx->device == c->c1->device, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: resize tables on device %d, the unit on device %d", r->ctx->device, c->c1->device);
    OMNI_REQUIRE(n_keyframes == c->n, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: %d key frames for a unit of %d (omni_cam_set_active)", n_keyframes, c->n);
    OMNI_REQUIRE(src_stride >= r->src_w, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: stride %d for frames %d wide", src_stride, r->src_w);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_enqueue_raw with a unit in flight (omni_cam_wait first)");
    return cam_poses_check(c);
}

// left camera first and MobileNetVLAD behind it, then the right camera: the order of cam_fisheye_locked.  n_left > 0: the frames are in host memory, each camera's
// n_keyframes frames the concatenation of its parts (part i: images[i] frames, src_stride); they go up into d_raw, one asynchronous copy per part, in front of
// the camera's resize
static int cam_raw_locked(omni_cam* c, omni_resize* r, const uint8_t* left_dev, const uint8_t* right_dev, const uint8_t* const* left, const int* left_images, int n_left,
                          const uint8_t* const* right, const int* right_images, int n_right, int src_stride, int n_keyframes) {
    int rc;
    if ((rc = cam_raw_check(c, r, src_stride, n_keyframes))) return rc;
    (void)hipSetDevice(c->c1->device);
    const size_t half = (size_t)c->n * c->W * c->H, frame = (size_t)src_stride * r->src_h;
    auto raw_bytes = [&](int frames) { return ((size_t)frames * r->src_h - 1) * src_stride + r->src_w; };      // (the last row may end at its width)
    if ((rc = cam_staging(c, c->d_gray, c->d_gray_bytes, 2 * half))) return rc;
    const size_t right_at = (raw_bytes(n_keyframes) + 255) & ~(size_t)255;
    if (n_left) {
        if ((rc = cam_staging(c, c->d_raw, c->d_raw_bytes, right_at + raw_bytes(n_keyframes)))) return rc;
        left_dev = c->d_raw; right_dev = c->d_raw + right_at;
    }
    hipStream_t s1 = c->c1->stream;
    auto upload = [&](uint8_t* dst, const uint8_t* const* parts, const int* images, int n_parts) -> hipError_t {
        for (int i = 0, at = 0; i < n_parts; at += images[i], ++i) {
            const hipError_t e = hipMemcpyAsync(dst + at * frame, parts[i], raw_bytes(images[i]), hipMemcpyHostToDevice, s1);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    OMNI_HIP_TRY(upload(c->d_raw, left, left_images, n_left));
    if ((rc = omni::resize_unit_launch(r, s1, left_dev, src_stride, n_keyframes, c->d_gray))) return rc;
    OMNI_HIP_TRY(hipEventRecord(c->e_up, s1));
    OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->e_up, 0));
    OMNI_HIP_TRY(upload(c->d_raw + right_at, right, right_images, n_right));
    if ((rc = omni::resize_unit_launch(r, s1, right_dev, src_stride, n_keyframes, c->d_gray + half))) return rc;
    return cam_enqueue_locked(c, c->d_gray, c->W, 0);                         // loop_cam.cpp:536 blanks rows for STEREO_FISHEYE only
}

int omni_cam_enqueue_raw_dev(omni_cam* c, omni_resize* r, const uint8_t* left_dev, const uint8_t* right_dev, int src_stride, int n_keyframes) {
    OMNI_REQUIRE(c && r && left_dev && right_dev, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_raw_dev (resize + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_raw_locked(c, r, left_dev, right_dev, nullptr, nullptr, 0, nullptr, nullptr, 0, src_stride, n_keyframes);
}

int omni_cam_enqueue_raw_host(omni_cam* c, omni_resize* r, const uint8_t* left_host, const uint8_t* right_host, int src_stride, int n_keyframes) {
    OMNI_REQUIRE(c && r && left_host && right_host, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_raw_host (upload + resize + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_raw_locked(c, r, nullptr, nullptr, &left_host, &n_keyframes, 1, &right_host, &n_keyframes, 1, src_stride, n_keyframes);
}

// the same from segments of host memory (what KeyframePipeline::run needs to cut units of its choice out of blocks laid out for another unit size, as
// omni_cam_enqueue_host_parts): the totals of both cameras' parts are the unit's active size
int omni_cam_enqueue_raw_host_parts(omni_cam* c, omni_resize* r, const uint8_t* const* left, const int* left_images, int n_left, const uint8_t* const* right,
                                    const int* right_images, int n_right, int src_stride) {
    OMNI_REQUIRE(c && r && left && left_images && right && right_images && n_left > 0 && n_right > 0, OMNI_ERR_INVALID, "null argument");
    int nl = 0, nr = 0;
    for (int i = 0; i < n_left; ++i) { OMNI_REQUIRE(left[i] && left_images[i] > 0, OMNI_ERR_INVALID, "omni_cam_enqueue_raw_host_parts: empty part"); nl += left_images[i]; }
    for (int i = 0; i < n_right; ++i) { OMNI_REQUIRE(right[i] && right_images[i] > 0, OMNI_ERR_INVALID, "omni_cam_enqueue_raw_host_parts: empty part"); nr += right_images[i]; }
    OMNI_REQUIRE(nl == nr, OMNI_ERR_INVALID, "omni_cam_enqueue_raw_host_parts: %d left frames, %d right frames", nl, nr);
    omni::TraceRange trace_range("omni_cam_enqueue_raw_host_parts (upload + resize + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_raw_locked(c, r, nullptr, nullptr, left, left_images, n_left, right, right_images, n_right, src_stride, nl);
}

// A unit whose frames arrive as JPEG files (is_compressed_images: comp_stereo_images_callback / comp_depth_images_callback, swarm_loop.cpp:72-89, each frame through
// cv::imdecode(data, IMREAD_GRAYSCALE)): the decode (jpeg_dec.hip) runs inside the unit, on the SuperPoint stream, in front of the resize, and the decoded frames
// take the place of omni_cam_enqueue_raw_*'s.  n_keyframes left files (all files of a mono handle: right_files = NULL) and as many right files; `resize` NULL:
// the files hold network-size pictures and are decoded straight into the unit's input block.  Everything behind is the existing unit.
int omni_cam_enqueue_jpeg_host(omni_cam* c, omni_resize* r, const uint8_t* const* left_files, const int64_t* left_sizes, const uint8_t* const* right_files,
                               const int64_t* right_sizes, int n_keyframes) {
    OMNI_REQUIRE(c && left_files && left_sizes && (!right_files == !right_sizes), OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_jpeg_host (decode + resize + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE((c->cams == 2) == (right_files != nullptr), OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host: a stereo handle takes left and right files, a mono handle left files only");
    OMNI_REQUIRE(n_keyframes == c->n, OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host: %d key frames for a unit of %d (omni_cam_set_active)", n_keyframes, c->n);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host with a unit in flight (omni_cam_wait first)");
    c->jdec_n = 0;                                                            // (no unit is in flight: whatever fails below, an earlier unit's statuses are not handed out for this one)
    if (r) {
        OMNI_REQUIRE(r->dst_w == c->W && r->dst_h == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host: the resize object makes %dx%d images but the networks were created for %dx%d",
                     r->dst_w, r->dst_h, c->W, c->H);
        OMNI_REQUIRE(r->ctx->device == c->c1->device, OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host: resize tables on device %d, the unit on device %d", r->ctx->device, c->c1->device);
    }
    int rc;
    if ((rc = cam_poses_check(c))) return rc;
    (void)hipSetDevice(c->c1->device);
    const int sw = r ? r->src_w : c->W, sh = r ? r->src_h : c->H, n = c->n, ni = c->cams * n;
    if ((rc = cam_jdec_ensure(c, sw, sh, c->cams * c->n_cap))) return rc;
    const size_t half = (size_t)n * c->W * c->H, frame = (size_t)sw * sh;
    if ((rc = cam_staging(c, c->d_gray, c->d_gray_bytes, (size_t)c->cams * half))) return rc;
    if (r && (rc = cam_staging(c, c->d_raw, c->d_raw_bytes, (size_t)ni * frame))) return rc;
    std::vector<const uint8_t*> files(left_files, left_files + n);
    std::vector<int64_t> sizes(left_sizes, left_sizes + n);
    if (right_files) {
        files.insert(files.end(), right_files, right_files + n);
        sizes.insert(sizes.end(), right_sizes, right_sizes + n);
    }
    hipStream_t s1 = c->c1->stream;
    // all frames of the unit in one decode: [left frames | right frames], rows packed (an UNSUPPORTED file or another size is refused here, nothing enqueued)
    uint8_t* dec = r ? c->d_raw : c->d_gray;
    if ((rc = omni::jpegdec_enqueue_on(c->jdec, s1, files.data(), sizes.data(), ni, dec, sw, c->d_jdec_status))) return rc;
    OMNI_HIP_TRY(hipMemcpyAsync(c->h_jdec_status, c->d_jdec_status, (size_t)ni * sizeof(int), hipMemcpyDeviceToHost, s1));
    if (r && (rc = omni::resize_unit_launch(r, s1, c->d_raw, sw, n, c->d_gray))) return rc;
    OMNI_HIP_TRY(hipEventRecord(c->e_up, s1));
    OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->e_up, 0));
    if (r && c->cams == 2 && (rc = omni::resize_unit_launch(r, s1, c->d_raw + (size_t)n * frame, sw, n, c->d_gray + half))) return rc;
    rc = cam_enqueue_locked(c, c->d_gray, c->W, 0);                                          // (no compressed path for STEREO_FISHEYE: no mask)
    c->jdec_n = rc == OMNI_OK ? ni : 0;
    return rc;
}

// the OMNI_JPEGDEC_* status of every frame of the last unit, [left frames | right frames]; after omni_cam_wait
int omni_cam_jpegdec_status(omni_cam* c, int* status, int n_frames) {
    OMNI_REQUIRE(c && status, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_jpegdec_status with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->jdec_n > 0, OMNI_ERR_INVALID, "omni_cam_jpegdec_status: the last unit did not come as JPEG files");
    OMNI_REQUIRE(n_frames == c->jdec_n, OMNI_ERR_INVALID, "omni_cam_jpegdec_status: %d frames asked for, the last unit had %d", n_frames, c->jdec_n);
    memcpy(status, c->h_jdec_status, (size_t)n_frames * sizeof(int));
    return OMNI_OK;
}

// the handle's own input block as the last unit's networks read it (the fisheye mask is applied inside the networks, not here: a unit of flattened views shows
// them as uploaded, a unit of raw frames as flatten_unit_kernel wrote them)
int omni_cam_get_input(omni_cam* c, uint8_t* out_host, int64_t bytes) {
    OMNI_REQUIRE(c && out_host && bytes > 0, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_get_input with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->input_bytes > 0, OMNI_ERR_INVALID, "omni_cam_get_input: the last unit read the caller's buffer, not the handle's");
    OMNI_REQUIRE((size_t)bytes <= c->input_bytes, OMNI_ERR_INVALID, "omni_cam_get_input: %lld bytes of an input block of %zu", (long long)bytes, c->input_bytes);
    (void)hipSetDevice(c->c1->device);
    OMNI_HIP_TRY(hipMemcpyAsync(out_host, c->d_gray, (size_t)bytes, hipMemcpyDeviceToHost, c->c1->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(c->c1->stream));
    return OMNI_OK;
}

static int cam_enqueue_locked(omni_cam* c, const uint8_t* gray_dev, int stride, int fisheye_mask) {
    const int n = c->n, M = c->M, D = c->D, ni = c->cams * c->n;
    int rc;
    c->input_bytes = gray_dev == c->d_gray ? (size_t)ni * c->W * c->H : 0;
    // images 0..n-1 = "up" (main) camera of each direction, n..2n-1 = "down" camera (loop_cam.cpp:350-351)
    if ((rc = omni_sp_enqueue_dev(c->sp, gray_dev, stride, ni, fisheye_mask))) return rc;
    if ((rc = omni_vlad_enqueue_dev(c->vlad, gray_dev, stride, n, fisheye_mask))) return rc;       // main camera only (:553-556)
    // match_HFNet_local_features: up = query, down = train (:147-150); pair p = direction p
    if (c->cams == 2 &&
        (rc = omni_bf_match_batched_dev(c->c1, n, M, D, c->bf_mode, c->desc_dev, (int64_t)M * D, c->n_dev,
                                        c->desc_dev + (size_t)n * M * D, (int64_t)M * D, c->n_dev + n, c->d_qidx, c->d_tidx, c->d_dist, c->d_nm)))
        return rc;
    hipStream_t s1 = c->c1->stream, s2 = c->c2->stream;
    char* h = c->host;
    OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_kps, c->kps_dev, (size_t)ni * M * 2 * 4, hipMemcpyDeviceToHost, s1));
    OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_n, c->n_dev, (size_t)ni * 4, hipMemcpyDeviceToHost, s1));
    OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_desc, c->desc_dev, (size_t)ni * M * D * 4, hipMemcpyDeviceToHost, s1));
    OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_sc, c->sc_dev, (size_t)ni * M * 4, hipMemcpyDeviceToHost, s1));
    if (c->cams == 2) {                                                       // (one camera: n_matches stays 0, as the block was zeroed at creation)
        OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_q, c->d_qidx, (size_t)n * M * 4, hipMemcpyDeviceToHost, s1));
        OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_t, c->d_tidx, (size_t)n * M * 4, hipMemcpyDeviceToHost, s1));
        OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_d, c->d_dist, (size_t)n * M * 4, hipMemcpyDeviceToHost, s1));
        OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_nm, c->d_nm, (size_t)n * 4, hipMemcpyDeviceToHost, s1));
    }
    c->lm_unit = false;
    if (c->lm_on) {
        // generate_stereo_image_descriptor's lifting and triangulation (loop_cam.cpp:397-444), right behind the up <-> down match it reads; its four arrays go
        // down in front of the unit's event.  (The down images' key points lie right behind the up images' in the network's output, as the outputs here.)
        const size_t half = (size_t)n * M;
        float *d_norm = reinterpret_cast<float*>(c->d_lm), *d_l3d = reinterpret_cast<float*>(c->d_lm + (c->off_l3d - c->off_norm));
        uint8_t* d_flag = reinterpret_cast<uint8_t*>(c->d_lm + (c->off_flag - c->off_norm));
        int* d_cnt = reinterpret_cast<int*>(c->d_lm + (c->off_cnt - c->off_norm));
        OMNI_HIP_TRY(hipMemcpyAsync(c->d_poses, h + c->off_poses, (size_t)c->n_poses * 7 * 8, hipMemcpyHostToDevice, s1));
        if ((rc = omni::landmarks_launch(s1, c->model, c->camera, c->d_poses, n, M, c->kps_dev, c->kps_dev + half * 2, c->n_dev, c->n_dev + n, c->d_qidx, c->d_tidx, c->d_nm, d_norm,
                                         d_norm + half * 2, d_l3d, d_l3d + half * 3, d_flag, d_flag + half, d_cnt)))
            return rc;
        // (the whole block in one copy, a few hundred kilobytes at most; a smaller unit leaves the tail of each array as it was)
        OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_norm, c->d_lm, c->off_lm_end - c->off_norm, hipMemcpyDeviceToHost, s1));
        c->lm_unit = true; c->lm_n = n;
        c->n_poses = 0;                                                       // (consumed: the next unit needs its own)
    }
    if (c->dp_on) {
        // generate_gray_depth_image_descriptor's landmarks (loop_cam.cpp:260-304) behind the key points they read: the unit's poses, have flags and (unless they
        // are in HBM already) depth frames go up on this stream, the kernel follows, its four arrays go down in front of the unit's event
        const omni_depth_model& dm = c->dmodel;
        const size_t frame = (size_t)dm.depth_width * dm.depth_height * sizeof(uint16_t);
        float *d_norm = reinterpret_cast<float*>(c->d_lm), *d_l3d = reinterpret_cast<float*>(c->d_lm + (c->off_l3d - c->off_norm));
        uint8_t* d_flag = reinterpret_cast<uint8_t*>(c->d_lm + (c->off_flag - c->off_norm));
        int* d_cnt = reinterpret_cast<int*>(c->d_lm + (c->off_cnt - c->off_norm));
        OMNI_HIP_TRY(hipMemcpyAsync(c->d_poses, h + c->off_poses, (size_t)n * 7 * 8, hipMemcpyHostToDevice, s1));
        OMNI_HIP_TRY(hipMemcpyAsync(c->d_depth + c->depth_have, c->h_depth + c->depth_have, (size_t)n, hipMemcpyHostToDevice, s1));
        if (!c->depth_ext) OMNI_HIP_TRY(hipMemcpyAsync(c->d_depth, c->h_depth, (size_t)n * frame, hipMemcpyHostToDevice, s1));
        const uint16_t* depth = c->depth_ext ? c->depth_ext : reinterpret_cast<const uint16_t*>(c->d_depth);
        if ((rc = omni::depth_landmarks_launch(s1, dm, c->dcamera, c->d_poses, n, M, c->kps_dev, c->n_dev, depth, c->depth_ext ? c->depth_ext_stride : dm.depth_width,
                                               c->d_depth + c->depth_have, d_norm, d_l3d, d_flag, d_cnt)))
            return rc;
        OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_norm, c->d_lm, c->off_lm_end - c->off_norm, hipMemcpyDeviceToHost, s1));
        c->lm_unit = true; c->lm_n = n;
        c->n_poses = 0; c->n_depth = 0; c->depth_ext = nullptr;              // (consumed: the next unit needs its own)
    }
    OMNI_HIP_TRY(hipEventRecord(c->e1, s1));
    OMNI_HIP_TRY(hipMemcpyAsync(h + c->off_g, c->g_dev, (size_t)n * c->out_dim * 4, hipMemcpyDeviceToHost, s2));
    c->jpeg_unit = false;
    c->jdec_n = 0;                                                            // (omni_cam_enqueue_jpeg_host sets it behind this call)
    if (c->jpeg_quality) {
        // encode_image on the main image of every direction (loop_cam.cpp:306-308, 463-469): behind MobileNetVLAD's read of the same n images on ITS stream, next
        // to the SuperPoint stack.  The reference blanks the mask's rows in the very pixels it encodes (:536-539 through a cv::Mat that shares its data); the
        // unit's input block keeps them, so the kernel reads those rows as zeros
        int row0 = c->H, row1 = c->H;
        if (fisheye_mask) omni_fisheye_mask_rows(c->H, fisheye_mask, &row0, &row1);
        int* d_meta = reinterpret_cast<int*>(c->d_jpeg + c->jpeg_meta);
        if ((rc = omni::jpeg_check_enqueue(c->jpeg, stride, n, row0))) return rc;
        if ((rc = omni::jpeg_launch(c->jpeg, s2, gray_dev, stride, n, row0, c->d_jpeg, d_meta, d_meta + c->n_cap))) return rc;
        OMNI_HIP_TRY(hipMemcpyAsync(c->h_jpeg, c->d_jpeg, (size_t)n * c->jpeg_cap, hipMemcpyDeviceToHost, s2));
        OMNI_HIP_TRY(hipMemcpyAsync(c->h_jpeg + c->jpeg_meta, d_meta, (size_t)2 * c->n_cap * 4, hipMemcpyDeviceToHost, s2));
        c->jpeg_unit = true; c->jpeg_n = n;
    }
    OMNI_HIP_TRY(hipEventRecord(c->e2, s2));
    c->pending = true;
    return OMNI_OK;
}

int omni_cam_order_after(omni_cam* later, omni_cam* earlier, int streams) {
    OMNI_REQUIRE(later && earlier, OMNI_ERR_INVALID, "null argument");
    if (later == earlier || streams <= 0) return OMNI_OK;
    OMNI_REQUIRE(later->c1->device == earlier->c1->device, OMNI_ERR_INVALID, "omni_cam_order_after: two units of one device");
    (void)hipSetDevice(later->c1->device);
    hipEvent_t ev = omni_sp_convs_event(earlier->sp);
    OMNI_REQUIRE(ev, OMNI_ERR_INVALID, "omni_cam_order_after: no event");
    OMNI_HIP_TRY(hipStreamWaitEvent(later->c1->stream, ev, 0));          // (an event that was never recorded does not block)
    if (streams >= 2 && later->c2 != later->c1) OMNI_HIP_TRY(hipStreamWaitEvent(later->c2->stream, ev, 0));
    return OMNI_OK;
}

// a unit smaller than the handle was created for (a partly filled micro-batch that must not wait any longer): the next enqueues read cams * n_dirs
// images -- up cameras first, the down cameras right behind them -- and every array of omni_cam_result has that leading dimension
int omni_cam_set_active(omni_cam* c, int n_dirs) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(n_dirs >= 1 && n_dirs <= c->n_cap, OMNI_ERR_INVALID, "omni_cam_set_active: %d directions, the handle holds 1..%d", n_dirs, c->n_cap);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_active with a unit in flight (omni_cam_wait first)");
    c->n = n_dirs;
    return OMNI_OK;
}

// ---- stereo landmarks inside the unit ----------------------------------------------------------------------------------------------------------------
int omni_cam_set_stereo_model(omni_cam* c, const omni_stereo_model* model) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_stereo_model with a unit in flight (omni_cam_wait first)");
    if (!model) { c->lm_on = false; c->n_poses = 0; return OMNI_OK; }
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_set_stereo_model: a mono handle has no up / down camera pair to triangulate from");
    int rc;
    if ((rc = omni::landmarks_check_model(model))) return rc;
    OMNI_REQUIRE(c->n_cap % model->dirs_per_keyframe == 0, OMNI_ERR_INVALID, "omni_cam_set_stereo_model: %d directions per key frame do not divide the handle's %d",
                 model->dirs_per_keyframe, c->n_cap);
    c->model = *model;
    c->lm_on = true;
    c->n_poses = 0;
    return OMNI_OK;
}

int omni_cam_set_camera_model(omni_cam* c, const omni_camera_model* camera) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_camera_model with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_set_camera_model: a mono handle runs no stereo-landmark stage to lift in");
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    int rc;
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    c->camera = cm;
    return OMNI_OK;
}

int omni_cam_set_poses(omni_cam* c, const double* poses7, int n_keyframes) {
    OMNI_REQUIRE(c && poses7, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_poses with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->lm_on || c->dp_on, OMNI_ERR_INVALID, "omni_cam_set_poses without a stereo model (omni_cam_set_stereo_model)");
    const int dirs = c->dp_on ? 1 : c->model.dirs_per_keyframe;              // (a mono unit with a depth model: one key frame per image)
    OMNI_REQUIRE(n_keyframes >= 1 && (int64_t)n_keyframes * dirs <= c->n_cap, OMNI_ERR_INVALID,
                 "omni_cam_set_poses: %d key frames x %d directions, the handle holds %d directions", n_keyframes, dirs, c->n_cap);
    memcpy(c->host + c->off_poses, poses7, (size_t)n_keyframes * 7 * sizeof(double));
    c->n_poses = n_keyframes;
    return OMNI_OK;
}

int omni_cam_landmarks(omni_cam* c, omni_cam_landmarks_result* out) {
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_landmarks with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->lm_unit, OMNI_ERR_INVALID, "omni_cam_landmarks: the last unit ran without a stereo model (omni_cam_set_stereo_model)");
    const char* h = c->host;
    out->n_images = c->cams * c->lm_n; out->n_dirs = c->lm_n; out->max_num = c->M;      // (a mono unit: the depth landmarks, count_3d per image)
    out->norm2d = reinterpret_cast<const float*>(h + c->off_norm);
    out->landmarks_3d = reinterpret_cast<const float*>(h + c->off_l3d);
    out->landmarks_flag = reinterpret_cast<const uint8_t*>(h + c->off_flag);
    out->count_3d = reinterpret_cast<const int*>(h + c->off_cnt);
    return OMNI_OK;
}

// ---- depth landmarks inside a mono unit ----------------------------------------------------------------------------------------------------------------
int omni_cam_set_depth_model(omni_cam* c, const omni_depth_model* model, const omni_camera_model* camera) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_depth_model with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->cams == 1, OMNI_ERR_INVALID, "omni_cam_set_depth_model: a stereo handle triangulates its landmarks (omni_cam_set_stereo_model), it reads no depth image");
    if (!model) { c->dp_on = false; c->n_poses = 0; c->n_depth = 0; c->depth_ext = nullptr; return OMNI_OK; }
    int rc;
    if ((rc = omni::depth_check_model(model))) return rc;
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    (void)hipSetDevice(c->c1->device);
    const size_t have_at = ((size_t)c->n_cap * model->depth_width * model->depth_height * sizeof(uint16_t) + 255) & ~(size_t)255, bytes = have_at + (size_t)c->n_cap;
    if (bytes != c->depth_bytes || have_at != c->depth_have) {                // (set-up time: no unit is in flight, the frees below wait for nothing of this handle)
        c->dp_on = false;
        if (c->d_depth) (void)hipFree(c->d_depth);
        if (c->h_depth) (void)hipHostFree(c->h_depth);
        c->d_depth = c->h_depth = nullptr; c->depth_bytes = 0;
        OMNI_HIP_TRY(hipMalloc((void**)&c->d_depth, bytes));
        OMNI_HIP_TRY(hipHostMalloc((void**)&c->h_depth, bytes, hipHostMallocDefault));
        memset(c->h_depth, 0, bytes);
        c->depth_bytes = bytes; c->depth_have = have_at;
    }
    c->dmodel = *model; c->dcamera = cm;
    c->dp_on = true;
    c->n_poses = 0; c->n_depth = 0; c->depth_ext = nullptr;
    return OMNI_OK;
}

static int cam_depth_check(omni_cam* c, const char* who, int stride_elems, int n_images) {
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "%s with a unit in flight (omni_cam_wait first)", who);
    OMNI_REQUIRE(c->dp_on, OMNI_ERR_INVALID, "%s without a depth model (omni_cam_set_depth_model)", who);
    OMNI_REQUIRE(n_images >= 1 && n_images <= c->n_cap, OMNI_ERR_INVALID, "%s: %d images, the handle holds 1..%d", who, n_images, c->n_cap);
    OMNI_REQUIRE(stride_elems >= c->dmodel.depth_width, OMNI_ERR_INVALID, "%s: a stride of %d elements for depth images %d wide", who, stride_elems, c->dmodel.depth_width);
    return OMNI_OK;
}

int omni_cam_set_depth_host(omni_cam* c, const uint16_t* const* frames, int stride_elems, int n_images) {
    OMNI_REQUIRE(c && frames, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_depth_check(c, "omni_cam_set_depth_host", stride_elems, n_images))) return rc;
    const int w = c->dmodel.depth_width, hgt = c->dmodel.depth_height;
    uint16_t* dst = reinterpret_cast<uint16_t*>(c->h_depth);
    uint8_t* have = c->h_depth + c->depth_have;
    for (int i = 0; i < n_images; ++i) {
        have[i] = frames[i] != nullptr;
        if (!frames[i]) continue;                                             // (the kernel does not read the frame of an image without one)
        uint16_t* d = dst + (size_t)i * w * hgt;
        if (stride_elems == w) memcpy(d, frames[i], (size_t)w * hgt * sizeof(uint16_t));
        else for (int y = 0; y < hgt; ++y) memcpy(d + (size_t)y * w, frames[i] + (size_t)y * stride_elems, (size_t)w * sizeof(uint16_t));
    }
    c->n_depth = n_images; c->depth_ext = nullptr;
    return OMNI_OK;
}

int omni_cam_set_depth_dev(omni_cam* c, const uint16_t* depth_dev, int stride_elems, const uint8_t* have_host, int n_images) {
    OMNI_REQUIRE(c && depth_dev, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_depth_check(c, "omni_cam_set_depth_dev", stride_elems, n_images))) return rc;
    uint8_t* have = c->h_depth + c->depth_have;
    for (int i = 0; i < n_images; ++i) have[i] = have_host ? have_host[i] != 0 : 1;
    c->n_depth = n_images; c->depth_ext = depth_dev; c->depth_ext_stride = stride_elems;
    return OMNI_OK;
}

// ---- send_img inside the unit --------------------------------------------------------------------------------------------------------------------------
int omni_cam_set_jpeg(omni_cam* c, int quality, int64_t capacity_per_image) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_jpeg with a unit in flight (omni_cam_wait first)");
    if (quality == 0) { c->jpeg_quality = 0; return OMNI_OK; }
    OMNI_REQUIRE(quality >= 1 && quality <= 100, OMNI_ERR_INVALID, "omni_cam_set_jpeg: quality %d outside 1..100 (0: off)", quality);
    OMNI_REQUIRE(capacity_per_image >= OMNI_JPEG_HEADER_BYTES + 2 && capacity_per_image <= 0x7fffffff, OMNI_ERR_INVALID,
                 "omni_cam_set_jpeg: a capacity of %lld bytes, the header and EOI alone take %d", (long long)capacity_per_image, OMNI_JPEG_HEADER_BYTES + 2);
    if (c->jpeg && quality == c->jpeg_quality && capacity_per_image == c->jpeg_cap) return OMNI_OK;
    (void)hipSetDevice(c->c1->device);
    // (set-up time: the frees below wait for the device)
    if (c->jpeg) { omni_jpeg_destroy(c->jpeg); c->jpeg = nullptr; }
    c->jpeg_quality = 0;
    if (capacity_per_image != c->jpeg_cap || !c->d_jpeg) {
        if (c->d_jpeg) (void)hipFree(c->d_jpeg);
        if (c->h_jpeg) (void)hipHostFree(c->h_jpeg);
        c->d_jpeg = c->h_jpeg = nullptr; c->jpeg_cap = 0;
        c->jpeg_meta = ((size_t)c->n_cap * capacity_per_image + 255) & ~(size_t)255;
        const size_t bytes = c->jpeg_meta + (size_t)2 * c->n_cap * 4;
        OMNI_HIP_TRY(hipMalloc((void**)&c->d_jpeg, bytes));
        OMNI_HIP_TRY(hipHostMalloc((void**)&c->h_jpeg, bytes, hipHostMallocDefault));
        memset(c->h_jpeg, 0, bytes);
        c->jpeg_cap = capacity_per_image;
    }
    c->jpeg = omni_jpeg_create(c->c2, c->W, c->H, c->n_cap, quality, capacity_per_image);
    if (!c->jpeg) return OMNI_ERR_INVALID;                                    // (omni_jpeg_create left the message)
    c->jpeg_quality = quality;
    return OMNI_OK;
}

int omni_cam_jpeg(omni_cam* c, omni_cam_jpeg_result* out) {
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_jpeg with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->jpeg_unit, OMNI_ERR_INVALID, "omni_cam_jpeg: the last unit ran with the stage off (omni_cam_set_jpeg)");
    out->n_images = c->jpeg_n; out->capacity = c->jpeg_cap;
    out->bytes = c->h_jpeg;
    out->sizes = reinterpret_cast<const int*>(c->h_jpeg + c->jpeg_meta);
    out->status = out->sizes + c->n_cap;
    return OMNI_OK;
}

// non-blocking: *ready = 1 when omni_cam_wait would return at once (or nothing is pending)
int omni_cam_ready(omni_cam* c, int* ready) {
    OMNI_REQUIRE(c && ready, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *ready = 1;
    if (!c->pending) return OMNI_OK;
    (void)hipSetDevice(c->c1->device);
    for (hipEvent_t e : {c->e1, c->e2}) {
        const hipError_t r = hipEventQuery(e);
        if (r == hipErrorNotReady) { *ready = 0; return OMNI_OK; }
        if (r != hipSuccess) { omni::set_error("hipEventQuery failed: %s", hipGetErrorString(r)); return OMNI_ERR_HIP; }
    }
    return OMNI_OK;
}

int omni_cam_wait(omni_cam* c, omni_cam_result* out) {
    omni::TraceRange trace_range("omni_cam_wait");
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(c->pending, OMNI_ERR_INVALID, "omni_cam_wait without a pending omni_cam_enqueue_dev");
    (void)hipSetDevice(c->c1->device);
    OMNI_HIP_TRY(hipEventSynchronize(c->e1));
    OMNI_HIP_TRY(hipEventSynchronize(c->e2));
    c->pending = false;
    const char* h = c->host;
    out->n_dirs = c->n; out->max_num = c->M; out->desc_dim = c->D; out->global_dim = c->out_dim; out->n_images = c->cams * c->n;
    out->kps_xy = reinterpret_cast<const float*>(h + c->off_kps);
    out->n_kps = reinterpret_cast<const int*>(h + c->off_n);
    out->desc = reinterpret_cast<const float*>(h + c->off_desc);
    out->scores = reinterpret_cast<const float*>(h + c->off_sc);
    out->global_desc = reinterpret_cast<const float*>(h + c->off_g);
    out->match_up = reinterpret_cast<const int*>(h + c->off_q);
    out->match_down = reinterpret_cast<const int*>(h + c->off_t);
    out->match_dist = reinterpret_cast<const float*>(h + c->off_d);
    out->n_matches = reinterpret_cast<const int*>(h + c->off_nm);
    return OMNI_OK;
}

}  // extern "C"
