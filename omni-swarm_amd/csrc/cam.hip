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
// However a unit's frames arrive -- ten omni_cam_enqueue_* entries -- they get in front of the networks through ONE body, cam_input_run, which works from the plan of
// csrc/cam_input.h: where the bytes go and in which order the steps run is decided there, not here.
#include "common.h"
#include "camera_plan.h"
#include "cam_input.h"
#include "wire_plan.h"
#include <string.h>

namespace ci = omni::ci;

// The handle's stages, each with the memory it owns and its release (omni_cam_destroy, also behind a creation that failed half way)
struct CamCore {                              // the unit itself: match outputs, the pinned result block, the events, the staging buffers
    omni::DevMem mem;
    int *d_qidx = nullptr, *d_tidx = nullptr, *d_nm = nullptr;
    float* d_dist = nullptr;
    const float *kps_dev = nullptr, *desc_dev = nullptr, *sc_dev = nullptr, *g_dev = nullptr;      // the networks' own outputs
    const int* n_dev = nullptr;
    char* host = nullptr;
    size_t off_kps = 0, off_n = 0, off_desc = 0, off_sc = 0, off_g = 0, off_q = 0, off_t = 0, off_d = 0, off_nm = 0;
    hipEvent_t e1 = nullptr, e2 = nullptr, e_up = nullptr;
    // gray: the unit's input block when the handle makes it, cams * n images, rows packed to the networks' width; raw: the frames in front of a flatten / resize,
    // the up (left) cameras' and then the down (right) cameras', uploaded or decoded there (cam_input.h)
    omni::DevBuf gray, raw;
    size_t input_bytes = 0;                   // what the last unit read from `gray` (0: it read a caller's buffer): omni_cam_get_input
    void release() {
        mem.release_all(); gray.release(); raw.release();
        if (host) (void)hipHostFree(host);
        for (hipEvent_t e : {e1, e2, e_up}) if (e) (void)hipEventDestroy(e);
    }
};
// stereo landmarks inside the unit (omni_cam_set_stereo_model; landmarks.hip) and depth landmarks inside a MONO unit (omni_cam_set_depth_model; depth_landmarks.hip)
// share this block: the NEXT unit's poses (pinned staging in the result block, uploaded at enqueue) and the stage's four device outputs -- laid out as the key
// points, [up images | down images] of the active size (mono: one image per direction, count_3d per image)
struct CamLandmarks {
    bool on = false, unit = false;            // a stereo model is set; the unit enqueued last ran either stage (omni_cam_landmarks)
    omni_stereo_model model;
    omni_camera_model camera = omni::cam::ideal();      // the lens of the stage's lifts (omni_cam_set_camera_model): kept over omni_cam_set_stereo_model
    int n_poses = 0, n = 0;                   // key frames omni_cam_set_poses set since the last unit (0: none); directions of the unit that ran the stage last
    omni::DevMem mem;
    double* d_poses = nullptr;
    char* d_lm = nullptr;                     // ONE block laid out as host + off_norm .. off_end: norm2d | landmarks_3d | flags | count_3d (one copy down)
    size_t off_poses = 0, off_norm = 0, off_l3d = 0, off_flag = 0, off_cnt = 0, off_end = 0;
    void release() { mem.release_all(); }
};
// the NEXT mono unit's depth frames -- host (pinned): [n_cap] frames of depth_width x depth_height u16, rows packed, then (at have_at) have [n_cap] u8; dev: the
// same layout in HBM.  omni_cam_set_depth_dev borrows the frames instead (ext) and sets have only
struct CamDepth {
    bool on = false;
    omni_depth_model model;
    omni_camera_model camera = omni::cam::ideal();
    int n = 0, ext_stride = 0;                // n: images omni_cam_set_depth_host / _dev set since the last unit (0: none)
    const uint16_t* ext = nullptr;            // != nullptr: the next unit reads these frames (HBM, borrowed until omni_cam_wait) with ext_stride
    omni::HostBuf host;
    omni::DevBuf dev;
    size_t have_at = 0;
    void release() { host.release(); dev.release(); }
};
// send_img inside the unit (omni_cam_set_jpeg; jpeg.hip): the unit's main images [0, n) as JPEG files, on the MobileNetVLAD stream.  dev / host: the images' bytes
// [n_cap][cap], then (at meta) sizes [n_cap] and statuses [n_cap] -- a block of its own, pinned on the host side
struct CamJpegEnc {
    omni_jpeg* h = nullptr;
    int quality = 0, n = 0;                   // quality 0: the stage is off; n: main images of the unit enqueued last
    bool unit = false;                        // that unit ran the stage (omni_cam_jpeg)
    int64_t cap = 0;
    size_t meta = 0;
    omni::DevBuf dev;
    omni::HostBuf host;
    void release() { if (h) omni_jpeg_destroy(h); h = nullptr; dev.release(); host.release(); }
};
// is_compressed_images (omni_cam_enqueue_jpeg_host; jpeg_dec.hip): the unit's frames arrive as JPEG files and are decoded on the SuperPoint stream in front of the
// pre-processing.  The decoder is made at first use for the frames' size; statuses [cams * n_cap] go down into a pinned block of their own
struct CamJpegDec {
    omni_jpegdec* h = nullptr;
    int w = 0, ht = 0, max = 0, n = 0;        // max: pictures the decoder was made for; n: frames of the unit enqueued last if it came as files, else 0
    omni::DevMem mem;
    int *d_status = nullptr, *h_status = nullptr;
    void release() { if (h) omni_jpegdec_destroy(h); h = nullptr; mem.release_all(); if (h_status) (void)hipHostFree(h_status); }
};

// the LoopNet wire inside the unit (omni_cam_set_wire; wire_pack.hip): the unit's MAIN images [0, n) as packets, on the SuperPoint stream behind the landmark stage.
// dev / host (pinned): the images' buffers [n_cap][cap], then (at table_at) their tables [n_cap][te], then (at meta_at) the NEXT unit's records [n_cap], which the
// host side stages (omni_cam_set_wire_meta) and the enqueue uploads
struct CamWire {
    bool on = false, unit = false;            // the stage is on; the unit enqueued last ran it (omni_cam_wire)
    int send_all = 0, n = 0, n_meta = 0;      // n: main images of the unit enqueued last; n_meta: records set since the last unit (0: none)
    int64_t cap = 0;
    int te = 0;
    size_t table_at = 0, meta_at = 0;
    omni::DevBuf dev;
    omni::HostBuf host;
    hipEvent_t e_g = nullptr;                 // MobileNetVLAD's rows, for the SuperPoint stream to wait on
    // the whole descriptor of the same images (omni_cam_set_wire_image; wire_pack_image_kernel) behind the packets above and, with the file, behind the JPEG stage of
    // the other stream.  img_dev / img_host (pinned): the images' buffers [n_cap][img_cap], then (at img_sizes_at) their (offset, size) pairs [n_cap][2]
    bool img_on = false, img_unit = false;    // the stage is on; the unit enqueued last ran it (omni_cam_wire_image)
    int img_features = 0, img_file = 0;       // with_features, with_image
    int64_t img_cap = 0, img_jcap = 0;        // img_jcap: the JPEG stage's capacity the buffers were sized for (0 without the file)
    size_t img_sizes_at = 0;
    omni::DevBuf img_dev;
    omni::HostBuf img_host;
    hipEvent_t e_j = nullptr;                 // the JPEG stage's files, for the SuperPoint stream to wait on
    void release() {
        dev.release(); host.release(); img_dev.release(); img_host.release();
        for (hipEvent_t* e : {&e_g, &e_j}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    }
};

struct omni_cam {
    omni_sp* sp = nullptr; omni_vlad* vlad = nullptr;
    omni_ctx *c1 = nullptr, *c2 = nullptr;    // the SuperPoint stream's context, the MobileNetVLAD stream's
    int n = 0, n_cap = 0, cams = 2, M = 0, D = 0, out_dim = 0, bf_mode = 0, W = 0, H = 0;   // cams: 2 = up + down camera per direction, 1 = one camera (no stereo match)
      // n: directions of the NEXT enqueue (omni_cam_set_active), n_cap: what the handle and its networks were created for
      // W x H: the size the SuperPoint handle (and MobileNetVLAD) was created for
    bool pending = false;
    CamCore core; CamLandmarks lm; CamDepth depth; CamJpegEnc enc; CamJpegDec dec; CamWire wire;      // the stages: omni_cam_destroy releases each
    std::mutex mu;
};

// the landmark block's four arrays, at `base` = CamLandmarks::d_lm (HBM) or the result block + off_norm (pinned)
struct CamLmView { float *norm2d, *l3d; uint8_t* flag; int* count; };
static CamLmView cam_lm_view(const CamLandmarks& l, char* base) {
    return {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + (l.off_l3d - l.off_norm)), reinterpret_cast<uint8_t*>(base + (l.off_flag - l.off_norm)),
            reinterpret_cast<int*>(base + (l.off_cnt - l.off_norm))};
}

extern "C" {

static omni_cam* cam_create(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_dirs, int cams, int max_num, int global_dim, int bf_mode) {
    if (!sp_ctx || !sp || !vlad_ctx || !vlad) { omni::set_error("null handle"); return nullptr; }
    if (n_dirs < 1 || n_dirs > 64 || max_num < 1 || max_num > 1024 || global_dim < 1) { omni::set_error("bad n_dirs/max_num/global_dim"); return nullptr; }
    if (sp_ctx->device != vlad_ctx->device) { omni::set_error("SuperPoint and MobileNetVLAD contexts are on different devices"); return nullptr; }
    (void)hipSetDevice(sp_ctx->device);
    omni_cam* c = new omni_cam();
    c->sp = sp; c->vlad = vlad; c->c1 = sp_ctx; c->c2 = vlad_ctx; c->n = c->n_cap = n_dirs; c->cams = cams; c->M = max_num; c->D = omni_sp_desc_dim(sp);
    c->out_dim = global_dim; c->bf_mode = bf_mode;
    (void)omni_sp_image_size(sp, &c->W, &c->H);
    CamCore& k = c->core; CamLandmarks& l = c->lm;
    const size_t n = n_dirs, M = max_num, D = c->D, ni = (size_t)cams * n;
    size_t o = 0;                                                             // the pinned result block: every array at a multiple of 256 bytes
    auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    k.off_kps = take(ni * M * 2 * 4); k.off_n = take(ni * 4); k.off_desc = take(ni * M * D * 4); k.off_sc = take(ni * M * 4);
    k.off_g = take(n * (size_t)global_dim * 4);
    k.off_q = take(n * M * 4); k.off_t = take(n * M * 4); k.off_d = take(n * M * 4); k.off_nm = take(n * 4);
    // the landmark stage's part of the block (a few kilobytes per image; mono: the depth landmarks')
    l.off_poses = take(n * 7 * 8);
    l.off_norm = take(ni * M * 2 * 4); l.off_l3d = take(ni * M * 3 * 4); l.off_flag = take(ni * M); l.off_cnt = take(n * 4);
    l.off_end = o;
    bool ok = hipHostMalloc((void**)&k.host, o, hipHostMallocDefault) == hipSuccess &&
              k.mem.alloc(&k.d_qidx, n * M * 4) == OMNI_OK && k.mem.alloc(&k.d_tidx, n * M * 4) == OMNI_OK &&
              k.mem.alloc(&k.d_dist, n * M * 4) == OMNI_OK && k.mem.alloc(&k.d_nm, n * 4) == OMNI_OK &&
              l.mem.alloc(&l.d_poses, n * 7 * 8) == OMNI_OK && l.mem.alloc(&l.d_lm, l.off_end - l.off_norm) == OMNI_OK &&
              omni_sp_dev_outputs(sp, &k.kps_dev, &k.n_dev, &k.desc_dev, &k.sc_dev) == OMNI_OK && omni_vlad_dev_output(vlad, &k.g_dev) == OMNI_OK;
    for (hipEvent_t* e : {&k.e1, &k.e2, &k.e_up}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) { omni::set_error("omni_cam_create: allocation failed"); omni_cam_destroy(c); return nullptr; }
    memset(k.host, 0, o);
    return c;
}

omni_cam* omni_cam_create(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_dirs, int max_num, int global_dim, int bf_mode) {
    return cam_create(sp_ctx, sp, vlad_ctx, vlad, n_dirs, 2, max_num, global_dim, bf_mode);
}

// CameraConfig::PINHOLE_DEPTH (loop_cam.cpp:190-194, generate_gray_depth_image_descriptor :231-339): ONE camera per image, both networks on every
// image, no up/down match; the landmarks come from the depth image: inside the unit with a depth model (omni_cam_set_depth_model, depth_landmarks.hip), else on
// the host (loop_geometry.hpp fill_depth_landmarks)
omni_cam* omni_cam_create_mono(omni_ctx* sp_ctx, omni_sp* sp, omni_ctx* vlad_ctx, omni_vlad* vlad, int n_images, int max_num, int global_dim) {
    return cam_create(sp_ctx, sp, vlad_ctx, vlad, n_images, 1, max_num, global_dim, 0);
}

void omni_cam_destroy(omni_cam* c) {
    if (!c) return;
    (void)hipSetDevice(c->c1->device);
    (void)hipStreamSynchronize(c->c1->stream); (void)hipStreamSynchronize(c->c2->stream);
    c->wire.release(); c->dec.release(); c->enc.release(); c->depth.release(); c->lm.release(); c->core.release();
    delete c;
}

static int cam_enqueue_locked(omni_cam* c, const uint8_t* gray_dev, int stride, int fisheye_mask);

// with a stereo model set, a unit needs the poses of ITS key frames; with a depth model, the depth frames of its images too
static int cam_landmark_inputs_check(omni_cam* c) {
    const int n_poses = c->lm.n_poses, n_depth = c->depth.n;
    if (c->depth.on) {                                                        // a mono unit with a depth model: the poses AND the depth frames of its images, one key frame per image
        OMNI_REQUIRE(n_poses > 0, OMNI_ERR_INVALID, "a depth model is set but the unit's poses are not (omni_cam_set_poses before every enqueue)");
        OMNI_REQUIRE(n_poses == c->n, OMNI_ERR_INVALID, "poses of %d key frames for a unit of %d images (omni_cam_set_poses, omni_cam_set_active)", n_poses, c->n);
        OMNI_REQUIRE(n_depth > 0, OMNI_ERR_INVALID, "a depth model is set but the unit's depth frames are not (omni_cam_set_depth_host / _dev before every enqueue)");
        OMNI_REQUIRE(n_depth == c->n, OMNI_ERR_INVALID, "depth frames of %d images for a unit of %d images (omni_cam_set_depth_host / _dev, omni_cam_set_active)", n_depth, c->n);
        return OMNI_OK;
    }
    if (!c->lm.on) return OMNI_OK;
    OMNI_REQUIRE(n_poses > 0, OMNI_ERR_INVALID, "a stereo model is set but the unit's poses are not (omni_cam_set_poses before every enqueue)");
    OMNI_REQUIRE(n_poses * c->lm.model.dirs_per_keyframe == c->n, OMNI_ERR_INVALID, "poses of %d key frames x %d directions for a unit of %d (omni_cam_set_poses, omni_cam_set_active)",
                 n_poses, c->lm.model.dirs_per_keyframe, c->n);
    return OMNI_OK;
}

// what a unit needs besides its frames: the above, and with the wire stage on the records of its main images and a landmark stage to pack the landmarks of.
// Checked by every enqueue entry before anything is enqueued (c->mu held)
static int cam_poses_depth_check(omni_cam* c) {
    int rc;
    if ((rc = cam_landmark_inputs_check(c))) return rc;
    if (!c->wire.on) return OMNI_OK;
    OMNI_REQUIRE(c->lm.on || c->depth.on, OMNI_ERR_INVALID, "the wire stage is on but the handle has no landmark model (omni_cam_set_stereo_model / omni_cam_set_depth_model)");
    OMNI_REQUIRE(c->wire.n_meta > 0, OMNI_ERR_INVALID, "the wire stage is on but the unit's records are not set (omni_cam_set_wire_meta before every enqueue)");
    OMNI_REQUIRE(c->wire.n_meta == c->n, OMNI_ERR_INVALID, "records of %d images for a unit of %d main images (omni_cam_set_wire_meta, omni_cam_set_active)", c->wire.n_meta, c->n);
    if (c->wire.img_on && c->wire.img_file)
        OMNI_REQUIRE(c->enc.quality && c->enc.cap == c->wire.img_jcap, OMNI_ERR_INVALID,
                     "the whole descriptor carries the image but the JPEG stage is off or has another capacity (omni_cam_set_jpeg, then omni_cam_set_wire_image again)");
    return OMNI_OK;
}

// ---- a unit's input: every arrival form through one body ---------------------------------------------------------------------------------------------------
// what a plan's steps read: per camera its parts -- segments of host memory (FORM_HOST), files (FORM_FILES; sizes: theirs) or ONE pointer into HBM (FORM_DEV) --
// and the object of its pre-processing.  The maps and tables are read on the unit's streams, never on the objects' own: keep them alive until omni_cam_wait
struct CamSources {
    const uint8_t* const* parts[2]; const int64_t* sizes[2];
    const omni_flatten* flat[2]; const omni_resize* resize;
};

// the handle's geometry and one source size for both cameras; host frames as one part per camera unless the entry says otherwise
static ci::CamInput cam_input_of(const omni_cam* c, int form, int pre, int frames, int stride, int fisheye_mask, int src_w, int src_h) {
    ci::CamInput in;
    in.form = form; in.pre = pre; in.cams = c->cams; in.n = c->n; in.W = c->W; in.H = c->H; in.n_cap = c->n_cap;
    in.src_w[0] = in.src_w[1] = src_w; in.src_h[0] = in.src_h[1] = src_h; in.frames = frames; in.stride = stride; in.fisheye_mask = fisheye_mask;
    return in;
}

// the handle's decoder for the plan's frames (made again for another size or more pictures).  c->mu held, no unit in flight
static int cam_jdec_ensure(omni_cam* c, const ci::CamInputPlan& p) {
    CamJpegDec& d = c->dec;
    const size_t status_bytes = (size_t)c->cams * c->n_cap * sizeof(int);
    int rc;
    if (!d.d_status && (rc = d.mem.alloc(&d.d_status, status_bytes))) return rc;
    if (!d.h_status) OMNI_HIP_TRY(hipHostMalloc((void**)&d.h_status, status_bytes, hipHostMallocDefault));
    if (d.h && d.w == p.dec_w && d.ht == p.dec_h && d.max >= p.dec_max) return OMNI_OK;
    if (d.h) omni_jpegdec_destroy(d.h);
    d.h = omni_jpegdec_create(c->c1, p.dec_w, p.dec_h, p.dec_max, p.dec_cap);
    if (!d.h) return OMNI_ERR_INVALID;                                        // (omni_jpegdec_create left the message)
    d.w = p.dec_w; d.ht = p.dec_h; d.max = p.dec_max;
    return OMNI_OK;
}

// c->mu held, the entry's own checks passed.  First camera first and MobileNetVLAD behind it (FENCE), then the second camera: MobileNetVLAD only reads the first
// cameras' images -- the first half of the input block -- and starts as soon as they are there, while the second half is still on the bus or in its kernels;
// SuperPoint's stream carries every step and so waits for all of it.  The reference uploads one image per engine call and blocks (tensorrt_generic.cpp:58-75);
// here every part is one asynchronous copy (pinned source: the copy engine runs it next to the other pipelines' kernels; packed rows go up as plain 1-D copies:
// 56 GB/s against 50 GB/s for the 2-D form of the same bytes, tools/probes/h2d_probe.hip).  A refusal of any step leaves nothing of the later ones enqueued
static int cam_input_run(omni_cam* c, const char* who, const ci::CamInput& in, const CamSources& src) {
    const ci::CamInputPlan p = ci::plan(in);
    // (no entry gets here with such frames: its own checks refuse them first, with its own message)
    OMNI_REQUIRE(p.n_steps, OMNI_ERR_INVALID, "%s: not a unit's frames (%d cameras x %d frames, %d + %d parts)", who, in.cams, in.frames, in.n_parts[0], in.n_parts[1]);
    (void)hipSetDevice(c->c1->device);
    c->dec.n = 0;                                                             // (whatever fails below, an earlier unit's statuses are not handed out for this one)
    int rc;
    // (both buffers grow behind whatever the device still reads from the old one: DevBuf::ensure's hipFree waits for it)
    if ((rc = c->core.gray.ensure(p.gray_bytes)) || (rc = c->core.raw.ensure(p.raw_bytes)) || (p.dec_images && (rc = cam_jdec_ensure(c, p)))) return rc;
    hipStream_t s1 = c->c1->stream;
    uint8_t *gray = c->core.gray.as<uint8_t>(), *raw = c->core.raw.as<uint8_t>(), *stage = p.stage == ci::AT_RAW ? raw : gray;
    for (int i = 0; i < p.n_steps; ++i) {
        const int cam = p.steps[i].cam;
        switch (p.steps[i].kind) {
        case ci::UPLOAD:
            for (int k = 0; k < p.n_parts[cam]; ++k) {
                const ci::Part& q = p.part[cam][k];
                OMNI_HIP_TRY(q.rows ? hipMemcpy2DAsync(stage + q.dst, in.src_w[cam], src.parts[cam][k], in.stride, in.src_w[cam], q.rows, hipMemcpyHostToDevice, s1)
                                    : hipMemcpyAsync(stage + q.dst, src.parts[cam][k], q.bytes, hipMemcpyHostToDevice, s1));
            }
            break;
        case ci::DECODE_ALL: {                                                // all frames of the unit in one decode (an UNSUPPORTED file or a picture of another size is refused here)
            const uint8_t* files[ci::MAX_FRAMES];
            int64_t sizes[ci::MAX_FRAMES];
            for (int k = 0; k < p.dec_images; ++k) { files[k] = src.parts[k / in.frames][k % in.frames]; sizes[k] = src.sizes[k / in.frames][k % in.frames]; }
            if ((rc = omni::jpegdec_enqueue_on(c->dec.h, s1, files, sizes, p.dec_images, stage, p.dec_stride, c->dec.d_status))) return rc;
            break;
        }
        case ci::STATUS_DOWN:
            OMNI_HIP_TRY(hipMemcpyAsync(c->dec.h_status, c->dec.d_status, (size_t)p.dec_images * sizeof(int), hipMemcpyDeviceToHost, s1));
            break;
        case ci::PRE: {
            const uint8_t* from = p.pre_src == ci::AT_CALLER ? src.parts[cam][0] : raw + (cam ? p.raw_cam1 : 0);
            uint8_t* to = gray + (cam ? p.gray_cam1 : 0);
            if ((rc = in.pre == ci::PRE_FLATTEN ? omni::flatten_unit_launch(src.flat[cam], s1, from, p.pre_stride, in.frames, in.first_view, in.dirs, in.W, in.H, in.fisheye_mask, to)
                                                : omni::resize_unit_launch(src.resize, s1, from, p.pre_stride, in.frames, to)))
                return rc;
            break;
        }
        case ci::FENCE:
            OMNI_HIP_TRY(hipEventRecord(c->core.e_up, s1));
            OMNI_HIP_TRY(hipStreamWaitEvent(c->c2->stream, c->core.e_up, 0));
            break;
        case ci::UNIT:
            if ((rc = cam_enqueue_locked(c, p.unit_src == ci::AT_CALLER ? src.parts[0][0] : gray, p.unit_stride, p.unit_mask))) return rc;
            c->dec.n = p.dec_images;
            break;
        }
    }
    return OMNI_OK;
}

int omni_cam_enqueue_dev(omni_cam* c, const uint8_t* gray_dev, int stride, int fisheye_mask) {
    omni::TraceRange trace_range("omni_cam_enqueue_dev");
    OMNI_REQUIRE(c && gray_dev, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_poses_depth_check(c))) return rc;
    const CamSources src = {{&gray_dev}};
    return cam_input_run(c, "omni_cam_enqueue_dev", cam_input_of(c, ci::FORM_DEV, ci::PRE_NONE, c->n, stride, fisheye_mask, c->W, c->H), src);
}

int omni_cam_enqueue_host(omni_cam* c, const uint8_t* gray_host, int stride, int width, int height, int fisheye_mask) {
    omni::TraceRange trace_range("omni_cam_enqueue_host (upload + unit)");
    OMNI_REQUIRE(c && gray_host, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(width > 0 && height > 0 && stride >= width, OMNI_ERR_INVALID, "bad image geometry %dx%d stride %d", width, height, stride);
    // the networks read cams * n images of THEIR size from the staging buffer: any other size would run them past its end
    OMNI_REQUIRE(width == c->W && height == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_host: images are %dx%d but the networks were created for %dx%d", width, height, c->W, c->H);
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_poses_depth_check(c))) return rc;
    const uint8_t* down_host = gray_host + (size_t)c->n * height * stride;  // one part per camera: the first n * height rows, the remaining rows
    const CamSources src = {{&gray_host, &down_host}};
    return cam_input_run(c, "omni_cam_enqueue_host", cam_input_of(c, ci::FORM_HOST, ci::PRE_NONE, c->n, stride, fisheye_mask, width, height), src);
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
    if ((rc = cam_poses_depth_check(c))) return rc;
    ci::CamInput in = cam_input_of(c, ci::FORM_HOST, ci::PRE_NONE, c->n, width, fisheye_mask, width, height);
    in.n_parts[0] = n_up; in.n_parts[1] = n_down; in.part_frames[0] = up_images; in.part_frames[1] = down_images;
    const CamSources src = {{up, down}};
    return cam_input_run(c, "omni_cam_enqueue_host_parts", in, src);
}

// A key frame's two RAW fisheye frames instead of its flattened views: the remap (flatten.hip) runs inside the unit, on the SuperPoint stream, and writes the
// unit's own input block.  n_keyframes up frames and as many down frames (u8, src_stride, frame i at + i * src_stride * source height); `up` / `down` hold the
// two cameras' maps, of which views [first_view, n_views) are the unit's directions: n_keyframes * (n_views - first_view) = the unit's active size, each view of
// the networks' size.  c->mu held; `a` / `b`: each camera's frames as ONE pointer (the pixel forms, which take each camera's own frame size) or its files
static int cam_fisheye_run(omni_cam* c, const char* who, int form, const omni_flatten* up, const omni_flatten* down, const uint8_t* const* a, const uint8_t* const* b,
                           const int64_t* a_sizes, const int64_t* b_sizes, int src_stride, int n_keyframes, int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: a mono handle has no up / down camera pair");
    OMNI_REQUIRE(n_keyframes >= 1 && first_view >= 0 && first_view < up->n_views && up->n_views == down->n_views, OMNI_ERR_INVALID,
                 "omni_cam_enqueue_fisheye: %d key frames, first view %d of %d (up) / %d (down)", n_keyframes, first_view, up->n_views, down->n_views);
    const int dirs = up->n_views - first_view;
    OMNI_REQUIRE((int64_t)n_keyframes * dirs == c->n, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: %d key frames x %d directions for a unit of %d (omni_cam_set_active)",
                 n_keyframes, dirs, c->n);
    for (const omni_flatten* f : {up, down}) {
        OMNI_REQUIRE(f->ctx->device == c->c1->device, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: maps on device %d, the unit on device %d", f->ctx->device, c->c1->device);
        OMNI_REQUIRE(src_stride >= f->src_w, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: stride %d for frames %d wide", src_stride, f->src_w);
        for (int v = first_view; v < f->n_views; ++v)
            OMNI_REQUIRE(f->vw[v] == c->W && f->vh[v] == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye: view %d is %dx%d but the networks were created for %dx%d", v,
                         f->vw[v], f->vh[v], c->W, c->H);
    }
    int rc, row0 = 0, row1 = 0;
    if ((rc = cam_poses_depth_check(c))) return rc;
    omni_fisheye_mask_rows(c->H, fisheye_mask, &row0, &row1);                 // files: flatten_unit_launch's own refusal, in front of the decode
    OMNI_REQUIRE(form != ci::FORM_FILES || (c->W % 4 == 0 && row1 == c->H && up->src_w >= 2), OMNI_ERR_INVALID, "%s: %dx%d views, frames %d wide", who, c->W, c->H, up->src_w);
    ci::CamInput in = cam_input_of(c, form, ci::PRE_FLATTEN, n_keyframes, src_stride, fisheye_mask, up->src_w, up->src_h);
    in.src_w[1] = down->src_w; in.src_h[1] = down->src_h; in.first_view = first_view; in.dirs = dirs;
    const CamSources src = {{a, b}, {a_sizes, b_sizes}, {up, down}};
    return cam_input_run(c, who, in, src);
}

int omni_cam_enqueue_fisheye_dev(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* up_dev, const uint8_t* down_dev, int src_stride, int n_keyframes,
                                 int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c && up && down && up_dev && down_dev, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_fisheye_dev (flatten + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_fisheye_run(c, "omni_cam_enqueue_fisheye_dev", ci::FORM_DEV, up, down, &up_dev, &down_dev, nullptr, nullptr, src_stride, n_keyframes, first_view, fisheye_mask);
}

int omni_cam_enqueue_fisheye_host(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* up_host, const uint8_t* down_host, int src_stride, int n_keyframes,
                                  int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c && up && down && up_host && down_host, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_fisheye_host (upload + flatten + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    return cam_fisheye_run(c, "omni_cam_enqueue_fisheye_host", ci::FORM_HOST, up, down, &up_host, &down_host, nullptr, nullptr, src_stride, n_keyframes, first_view, fisheye_mask);
}

// The same with each camera's n_keyframes RAW frames given as JPEG files (the compressed fisheye topics the reference's upstream, VINS-Fisheye, decodes in front of
// its own flattening): ONE decode of [up frames | down frames] (jpeg_dec.hip) on the SuperPoint stream into the raw staging, rows packed, where
// omni_cam_enqueue_fisheye_host uploads them; the two remaps and the unit follow as there, MobileNetVLAD behind the up camera's views.  A CORRUPT file is an
// all-zero frame and so all-zero views.
int omni_cam_enqueue_fisheye_jpeg_host(omni_cam* c, omni_flatten* up, omni_flatten* down, const uint8_t* const* up_files, const int64_t* up_sizes,
                                       const uint8_t* const* down_files, const int64_t* down_sizes, int n_keyframes, int first_view, int fisheye_mask) {
    OMNI_REQUIRE(c && up && down && up_files && up_sizes && down_files && down_sizes, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_fisheye_jpeg_host (decode + flatten + unit)");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye_jpeg_host with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(up->src_w == down->src_w && up->src_h == down->src_h, OMNI_ERR_INVALID, "omni_cam_enqueue_fisheye_jpeg_host: up frames of %dx%d, down frames of %dx%d (one decoder: one size)",
                 up->src_w, up->src_h, down->src_w, down->src_h);
    return cam_fisheye_run(c, "omni_cam_enqueue_fisheye_jpeg_host", ci::FORM_FILES, up, down, up_files, down_files, up_sizes, down_sizes, up->src_w, n_keyframes, first_view, fisheye_mask);
}

// A key frame's two RAW stereo-pinhole frames (CameraConfig::STEREO_PINHOLE: generate_stereo_image_descriptor for ONE direction, loop_cam.cpp:189-196) of the
// camera's size instead of network-size images: the resize both reference engines run on the host in front of their networks (resize.hip) runs inside the unit,
// on the SuperPoint stream, and writes the unit's own input block.  With one direction the unit's active size counts key frames: n_keyframes left frames (the
// "up" role) and as many right frames, each camera's in one buffer or in parts (loop_cam.cpp:536 blanks rows for STEREO_FISHEYE only: no mask)
static int cam_raw_run(omni_cam* c, int form, omni_resize* r, const uint8_t* const* left, const int* left_images, int n_left, const uint8_t* const* right,
                       const int* right_images, int n_right, int src_stride, int n_keyframes) {
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: a mono handle has no left / right camera pair");
    OMNI_REQUIRE(r->dst_w == c->W && r->dst_h == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: the resize object makes %dx%d images but the networks were created for %dx%d",
                 r->dst_w, r->dst_h, c->W, c->H);
    OMNI_REQUIRE(r->ctx->device == c->c1->device, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: resize tables on device %d, the unit on device %d", r->ctx->device, c->c1->device);
    OMNI_REQUIRE(n_keyframes == c->n, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: %d key frames for a unit of %d (omni_cam_set_active)", n_keyframes, c->n);
    OMNI_REQUIRE(src_stride >= r->src_w, OMNI_ERR_INVALID, "omni_cam_enqueue_raw: stride %d for frames %d wide", src_stride, r->src_w);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_enqueue_raw with a unit in flight (omni_cam_wait first)");
    int rc;
    if ((rc = cam_poses_depth_check(c))) return rc;
    ci::CamInput in = cam_input_of(c, form, ci::PRE_RESIZE, n_keyframes, src_stride, 0, r->src_w, r->src_h);
    in.n_parts[0] = n_left; in.n_parts[1] = n_right; in.part_frames[0] = left_images; in.part_frames[1] = right_images;
    const CamSources src = {{left, right}, {}, {}, r};
    return cam_input_run(c, "omni_cam_enqueue_raw", in, src);
}

int omni_cam_enqueue_raw_dev(omni_cam* c, omni_resize* r, const uint8_t* left_dev, const uint8_t* right_dev, int src_stride, int n_keyframes) {
    OMNI_REQUIRE(c && r && left_dev && right_dev, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_raw_dev (resize + unit)");
    return cam_raw_run(c, ci::FORM_DEV, r, &left_dev, nullptr, 1, &right_dev, nullptr, 1, src_stride, n_keyframes);
}

int omni_cam_enqueue_raw_host(omni_cam* c, omni_resize* r, const uint8_t* left_host, const uint8_t* right_host, int src_stride, int n_keyframes) {
    OMNI_REQUIRE(c && r && left_host && right_host, OMNI_ERR_INVALID, "null argument");
    omni::TraceRange trace_range("omni_cam_enqueue_raw_host (upload + resize + unit)");
    return cam_raw_run(c, ci::FORM_HOST, r, &left_host, nullptr, 1, &right_host, nullptr, 1, src_stride, n_keyframes);
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
    return cam_raw_run(c, ci::FORM_HOST, r, left, left_images, n_left, right, right_images, n_right, src_stride, nl);
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
    if (r) {
        OMNI_REQUIRE(r->dst_w == c->W && r->dst_h == c->H, OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host: the resize object makes %dx%d images but the networks were created for %dx%d",
                     r->dst_w, r->dst_h, c->W, c->H);
        OMNI_REQUIRE(r->ctx->device == c->c1->device, OMNI_ERR_INVALID, "omni_cam_enqueue_jpeg_host: resize tables on device %d, the unit on device %d", r->ctx->device, c->c1->device);
    }
    int rc;
    if ((rc = cam_poses_depth_check(c))) return rc;
    const int sw = r ? r->src_w : c->W, sh = r ? r->src_h : c->H;            // (no compressed path for STEREO_FISHEYE here: no mask)
    const CamSources src = {{left_files, right_files}, {left_sizes, right_sizes}, {}, r};
    return cam_input_run(c, "omni_cam_enqueue_jpeg_host", cam_input_of(c, ci::FORM_FILES, r ? ci::PRE_RESIZE : ci::PRE_NONE, n_keyframes, sw, 0, sw, sh), src);
}

// the OMNI_JPEGDEC_* status of every frame of the last unit, [left frames | right frames]; after omni_cam_wait
int omni_cam_jpegdec_status(omni_cam* c, int* status, int n_frames) {
    OMNI_REQUIRE(c && status, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_jpegdec_status with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->dec.n > 0, OMNI_ERR_INVALID, "omni_cam_jpegdec_status: the last unit did not come as JPEG files");
    OMNI_REQUIRE(n_frames == c->dec.n, OMNI_ERR_INVALID, "omni_cam_jpegdec_status: %d frames asked for, the last unit had %d", n_frames, c->dec.n);
    memcpy(status, c->dec.h_status, (size_t)n_frames * sizeof(int));
    return OMNI_OK;
}

// the handle's own input block as the last unit's networks read it (the fisheye mask is applied inside the networks, not here: a unit of flattened views shows
// them as uploaded, a unit of raw frames as flatten_unit_kernel wrote them)
int omni_cam_get_input(omni_cam* c, uint8_t* out_host, int64_t bytes) {
    OMNI_REQUIRE(c && out_host && bytes > 0, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_get_input with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->core.input_bytes > 0, OMNI_ERR_INVALID, "omni_cam_get_input: the last unit read the caller's buffer, not the handle's");
    OMNI_REQUIRE((size_t)bytes <= c->core.input_bytes, OMNI_ERR_INVALID, "omni_cam_get_input: %lld bytes of an input block of %zu", (long long)bytes, c->core.input_bytes);
    (void)hipSetDevice(c->c1->device);
    OMNI_HIP_TRY(hipMemcpyAsync(out_host, c->core.gray.p, (size_t)bytes, hipMemcpyDeviceToHost, c->c1->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(c->c1->stream));
    return OMNI_OK;
}

static int cam_enqueue_locked(omni_cam* c, const uint8_t* gray_dev, int stride, int fisheye_mask) {
    const int n = c->n, M = c->M, D = c->D, ni = c->cams * c->n;
    CamCore& k = c->core; CamLandmarks& l = c->lm;
    int rc;
    k.input_bytes = gray_dev == k.gray.p ? (size_t)ni * c->W * c->H : 0;
    // images 0..n-1 = "up" (main) camera of each direction, n..2n-1 = "down" camera (loop_cam.cpp:350-351)
    if ((rc = omni_sp_enqueue_dev(c->sp, gray_dev, stride, ni, fisheye_mask))) return rc;
    if ((rc = omni_vlad_enqueue_dev(c->vlad, gray_dev, stride, n, fisheye_mask))) return rc;       // main camera only (:553-556)
    // match_HFNet_local_features: up = query, down = train (:147-150); pair p = direction p
    if (c->cams == 2 &&
        (rc = omni_bf_match_batched_dev(c->c1, n, M, D, c->bf_mode, k.desc_dev, (int64_t)M * D, k.n_dev,
                                        k.desc_dev + (size_t)n * M * D, (int64_t)M * D, k.n_dev + n, k.d_qidx, k.d_tidx, k.d_dist, k.d_nm)))
        return rc;
    hipStream_t s1 = c->c1->stream, s2 = c->c2->stream;
    char* h = k.host;
    // the networks' four arrays go down, and behind them the match's four (one camera: n_matches stays 0, as the block was zeroed at creation)
    const struct { size_t off; const void* dev; size_t bytes; } down[8] = {
        {k.off_kps, k.kps_dev, (size_t)ni * M * 2 * 4}, {k.off_n, k.n_dev, (size_t)ni * 4}, {k.off_desc, k.desc_dev, (size_t)ni * M * D * 4}, {k.off_sc, k.sc_dev, (size_t)ni * M * 4},
        {k.off_q, k.d_qidx, (size_t)n * M * 4}, {k.off_t, k.d_tidx, (size_t)n * M * 4}, {k.off_d, k.d_dist, (size_t)n * M * 4}, {k.off_nm, k.d_nm, (size_t)n * 4}};
    for (int i = 0; i < (c->cams == 2 ? 8 : 4); ++i) OMNI_HIP_TRY(hipMemcpyAsync(h + down[i].off, down[i].dev, down[i].bytes, hipMemcpyDeviceToHost, s1));
    l.unit = false;
    const CamLmView v = cam_lm_view(l, l.d_lm);
    // either landmark stage reads the poses of the unit's key frames (cam_poses_depth_check: as many as the stage needs)
    if (l.on || c->depth.on) OMNI_HIP_TRY(hipMemcpyAsync(l.d_poses, h + l.off_poses, (size_t)l.n_poses * 7 * 8, hipMemcpyHostToDevice, s1));
    if (l.on) {
        // generate_stereo_image_descriptor's lifting and triangulation (loop_cam.cpp:397-444), right behind the up <-> down match it reads; its four arrays go
        // down in front of the unit's event.  (The down images' key points lie right behind the up images' in the network's output, as the outputs here.)
        const size_t half = (size_t)n * M;
        if ((rc = omni::landmarks_launch(s1, l.model, l.camera, l.d_poses, n, M, k.kps_dev, k.kps_dev + half * 2, k.n_dev, k.n_dev + n, k.d_qidx, k.d_tidx, k.d_nm, v.norm2d,
                                         v.norm2d + half * 2, v.l3d, v.l3d + half * 3, v.flag, v.flag + half, v.count)))
            return rc;
    }
    if (c->depth.on) {
        // generate_gray_depth_image_descriptor's landmarks (loop_cam.cpp:260-304) behind the key points they read: the unit's poses, have flags and (unless they
        // are in HBM already) depth frames go up on this stream, the kernel follows, its four arrays go down in front of the unit's event
        CamDepth& d = c->depth;
        const size_t frame = (size_t)d.model.depth_width * d.model.depth_height * sizeof(uint16_t);
        uint8_t *d_depth = d.dev.as<uint8_t>(), *h_depth = d.host.as<uint8_t>();
        OMNI_HIP_TRY(hipMemcpyAsync(d_depth + d.have_at, h_depth + d.have_at, (size_t)n, hipMemcpyHostToDevice, s1));
        if (!d.ext) OMNI_HIP_TRY(hipMemcpyAsync(d_depth, h_depth, (size_t)n * frame, hipMemcpyHostToDevice, s1));
        const uint16_t* depth = d.ext ? d.ext : reinterpret_cast<const uint16_t*>(d_depth);
        if ((rc = omni::depth_landmarks_launch(s1, d.model, d.camera, l.d_poses, n, M, k.kps_dev, k.n_dev, depth, d.ext ? d.ext_stride : d.model.depth_width,
                                               d_depth + d.have_at, v.norm2d, v.l3d, v.flag, v.count)))
            return rc;
        d.n = 0; d.ext = nullptr;                                             // (consumed: the next unit needs its own)
    }
    if (l.on || c->depth.on) {
        // (the whole block in one copy, a few hundred kilobytes at most; a smaller unit leaves the tail of each array as it was)
        OMNI_HIP_TRY(hipMemcpyAsync(h + l.off_norm, l.d_lm, l.off_end - l.off_norm, hipMemcpyDeviceToHost, s1));
        l.unit = true; l.n = n; l.n_poses = 0;                                // (the poses are consumed: the next unit needs its own)
    }
    c->wire.unit = false;
    if (c->wire.on) {
        // LoopNet::broadcast_fisheye_desc's packets of the unit's main images (loop_net.cpp:19-101; csrc/wire_plan.h) behind the landmark stage whose arrays they
        // carry -- the first n images of every array, on a stereo handle the up cameras' -- and behind MobileNetVLAD's rows, which come from the other stream.  The
        // records go up, the buffers and tables of the n images go down in front of the unit's event
        CamWire& w = c->wire;
        uint8_t *d_w = w.dev.as<uint8_t>(), *h_w = w.host.as<uint8_t>();
        OMNI_HIP_TRY(hipEventRecord(w.e_g, s2));
        OMNI_HIP_TRY(hipStreamWaitEvent(s1, w.e_g, 0));
        OMNI_HIP_TRY(hipMemcpyAsync(d_w + w.meta_at, h_w + w.meta_at, (size_t)n * sizeof(omni_wire_image_meta), hipMemcpyHostToDevice, s1));
        if ((rc = omni::wire_pack_launch(s1, n, M, w.send_all, k.kps_dev, k.n_dev, k.desc_dev, v.norm2d, v.l3d, v.flag, k.g_dev,
                                         reinterpret_cast<const omni_wire_image_meta*>(d_w + w.meta_at), d_w, reinterpret_cast<int*>(d_w + w.table_at))))
            return rc;
        OMNI_HIP_TRY(hipMemcpyAsync(h_w, d_w, (size_t)n * w.cap, hipMemcpyDeviceToHost, s1));
        OMNI_HIP_TRY(hipMemcpyAsync(h_w + w.table_at, d_w + w.table_at, (size_t)n * w.te * sizeof(int), hipMemcpyDeviceToHost, s1));
        w.unit = true; w.n = n; w.n_meta = 0;                                 // (the records are consumed: the next unit needs its own)
    }
    // (with the whole descriptor on, the SuperPoint stream has one more kernel to run, behind the JPEG stage enqueued below: its event is recorded there)
    const bool wire_image = c->wire.on && c->wire.img_on;
    c->wire.img_unit = false;
    if (!wire_image) OMNI_HIP_TRY(hipEventRecord(k.e1, s1));
    OMNI_HIP_TRY(hipMemcpyAsync(h + k.off_g, k.g_dev, (size_t)n * c->out_dim * 4, hipMemcpyDeviceToHost, s2));
    c->enc.unit = false;
    if (c->enc.quality) {
        // encode_image on the main image of every direction (loop_cam.cpp:306-308, 463-469): behind MobileNetVLAD's read of the same n images on ITS stream, next
        // to the SuperPoint stack.  The reference blanks the mask's rows in the very pixels it encodes (:536-539 through a cv::Mat that shares its data); the
        // unit's input block keeps them, so the kernel reads those rows as zeros
        CamJpegEnc& e = c->enc;
        int row0 = c->H, row1 = c->H;
        if (fisheye_mask) omni_fisheye_mask_rows(c->H, fisheye_mask, &row0, &row1);
        uint8_t *d_jpeg = e.dev.as<uint8_t>(), *h_jpeg = e.host.as<uint8_t>();
        int* d_meta = reinterpret_cast<int*>(d_jpeg + e.meta);
        if ((rc = omni::jpeg_check_enqueue(e.h, stride, n, row0))) return rc;
        if ((rc = omni::jpeg_launch(e.h, s2, gray_dev, stride, n, row0, d_jpeg, d_meta, d_meta + c->n_cap))) return rc;
        if (wire_image && c->wire.img_file) OMNI_HIP_TRY(hipEventRecord(c->wire.e_j, s2));
        OMNI_HIP_TRY(hipMemcpyAsync(h_jpeg, d_jpeg, (size_t)n * e.cap, hipMemcpyDeviceToHost, s2));
        OMNI_HIP_TRY(hipMemcpyAsync(h_jpeg + e.meta, d_meta, (size_t)2 * c->n_cap * 4, hipMemcpyDeviceToHost, s2));
        e.unit = true; e.n = n;
    }
    if (wire_image) {
        // the third packet of the same images, the whole ImageDescriptor_t (loop_net.cpp:103-116; csrc/wire_plan.h whole_*), on the SuperPoint stream behind
        // wire_pack_kernel: the same arrays and records, and with the file the JPEG stage's output where it lies in HBM, behind that stage's event.  Buffers and
        // sizes of the n images go down in front of the unit's event
        CamWire& w = c->wire;
        const CamJpegEnc& e = c->enc;
        uint8_t *d_w = w.dev.as<uint8_t>(), *d_i = w.img_dev.as<uint8_t>(), *h_i = w.img_host.as<uint8_t>();
        const uint8_t* d_jpeg = w.img_file ? e.dev.as<uint8_t>() : nullptr;
        const int* d_meta = w.img_file ? reinterpret_cast<const int*>(d_jpeg + e.meta) : nullptr;
        if (w.img_file) OMNI_HIP_TRY(hipStreamWaitEvent(s1, w.e_j, 0));
        if ((rc = omni::wire_pack_image_launch(s1, n, M, w.img_features, w.img_file, k.kps_dev, k.n_dev, k.desc_dev, v.norm2d, v.l3d, v.flag, k.g_dev,
                                               reinterpret_cast<const omni_wire_image_meta*>(d_w + w.meta_at), d_jpeg, d_meta, w.img_file ? d_meta + c->n_cap : nullptr,
                                               w.img_jcap, w.img_file ? c->W : 0, w.img_file ? c->H : 0,      // (encode_image sets the size with the file, loop_cam.cpp:67-70)
                                               d_i, reinterpret_cast<int*>(d_i + w.img_sizes_at))))
            return rc;
        OMNI_HIP_TRY(hipMemcpyAsync(h_i, d_i, (size_t)n * w.img_cap, hipMemcpyDeviceToHost, s1));
        OMNI_HIP_TRY(hipMemcpyAsync(h_i + w.img_sizes_at, d_i + w.img_sizes_at, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, s1));
        OMNI_HIP_TRY(hipEventRecord(k.e1, s1));
        w.img_unit = true;
    }
    OMNI_HIP_TRY(hipEventRecord(k.e2, s2));
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
    if (!model) { c->lm.on = false; c->lm.n_poses = 0; return OMNI_OK; }
    OMNI_REQUIRE(c->cams == 2, OMNI_ERR_INVALID, "omni_cam_set_stereo_model: a mono handle has no up / down camera pair to triangulate from");
    int rc;
    if ((rc = omni::landmarks_check_model(model))) return rc;
    OMNI_REQUIRE(c->n_cap % model->dirs_per_keyframe == 0, OMNI_ERR_INVALID, "omni_cam_set_stereo_model: %d directions per key frame do not divide the handle's %d",
                 model->dirs_per_keyframe, c->n_cap);
    c->lm.model = *model; c->lm.on = true; c->lm.n_poses = 0;
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
    c->lm.camera = cm;
    return OMNI_OK;
}

int omni_cam_set_poses(omni_cam* c, const double* poses7, int n_keyframes) {
    OMNI_REQUIRE(c && poses7, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_poses with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->lm.on || c->depth.on, OMNI_ERR_INVALID, "omni_cam_set_poses without a stereo model (omni_cam_set_stereo_model)");
    const int dirs = c->depth.on ? 1 : c->lm.model.dirs_per_keyframe;        // (a mono unit with a depth model: one key frame per image)
    OMNI_REQUIRE(n_keyframes >= 1 && (int64_t)n_keyframes * dirs <= c->n_cap, OMNI_ERR_INVALID,
                 "omni_cam_set_poses: %d key frames x %d directions, the handle holds %d directions", n_keyframes, dirs, c->n_cap);
    memcpy(c->core.host + c->lm.off_poses, poses7, (size_t)n_keyframes * 7 * sizeof(double));
    c->lm.n_poses = n_keyframes;
    return OMNI_OK;
}

int omni_cam_landmarks(omni_cam* c, omni_cam_landmarks_result* out) {
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_landmarks with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->lm.unit, OMNI_ERR_INVALID, "omni_cam_landmarks: the last unit ran without a stereo model (omni_cam_set_stereo_model)");
    const CamLmView v = cam_lm_view(c->lm, c->core.host + c->lm.off_norm);
    out->n_images = c->cams * c->lm.n; out->n_dirs = c->lm.n; out->max_num = c->M;      // (a mono unit: the depth landmarks, count_3d per image)
    out->norm2d = v.norm2d; out->landmarks_3d = v.l3d; out->landmarks_flag = v.flag; out->count_3d = v.count;
    return OMNI_OK;
}

// ---- depth landmarks inside a mono unit ----------------------------------------------------------------------------------------------------------------
int omni_cam_set_depth_model(omni_cam* c, const omni_depth_model* model, const omni_camera_model* camera) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_depth_model with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->cams == 1, OMNI_ERR_INVALID, "omni_cam_set_depth_model: a stereo handle triangulates its landmarks (omni_cam_set_stereo_model), it reads no depth image");
    CamDepth& d = c->depth;
    if (!model) { d.on = false; c->lm.n_poses = 0; d.n = 0; d.ext = nullptr; return OMNI_OK; }
    int rc;
    if ((rc = omni::depth_check_model(model))) return rc;
    const omni_camera_model cm = camera ? *camera : omni::cam::ideal();
    if ((rc = omni::landmarks_check_camera(&cm))) return rc;
    (void)hipSetDevice(c->c1->device);
    const size_t have_at = ((size_t)c->n_cap * model->depth_width * model->depth_height * sizeof(uint16_t) + 255) & ~(size_t)255, bytes = have_at + (size_t)c->n_cap;
    if (have_at != d.have_at) {                      // (set-up time: no unit is in flight, a buffer that grows waits for nothing of this handle)
        d.on = false; d.have_at = 0;
        if ((rc = d.dev.ensure(bytes)) || (rc = d.host.ensure(bytes))) return rc;
        memset(d.host.p, 0, bytes);
        d.have_at = have_at;
    }
    d.model = *model; d.camera = cm; d.on = true;
    c->lm.n_poses = 0; d.n = 0; d.ext = nullptr;
    return OMNI_OK;
}

static int cam_depth_check(omni_cam* c, const char* who, int stride_elems, int n_images) {
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "%s with a unit in flight (omni_cam_wait first)", who);
    OMNI_REQUIRE(c->depth.on, OMNI_ERR_INVALID, "%s without a depth model (omni_cam_set_depth_model)", who);
    OMNI_REQUIRE(n_images >= 1 && n_images <= c->n_cap, OMNI_ERR_INVALID, "%s: %d images, the handle holds 1..%d", who, n_images, c->n_cap);
    OMNI_REQUIRE(stride_elems >= c->depth.model.depth_width, OMNI_ERR_INVALID, "%s: a stride of %d elements for depth images %d wide", who, stride_elems, c->depth.model.depth_width);
    return OMNI_OK;
}

int omni_cam_set_depth_host(omni_cam* c, const uint16_t* const* frames, int stride_elems, int n_images) {
    OMNI_REQUIRE(c && frames, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_depth_check(c, "omni_cam_set_depth_host", stride_elems, n_images))) return rc;
    CamDepth& d = c->depth;
    const int w = d.model.depth_width, hgt = d.model.depth_height;
    uint16_t* dst = d.host.as<uint16_t>();
    uint8_t* have = d.host.as<uint8_t>() + d.have_at;
    for (int i = 0; i < n_images; ++i) {
        have[i] = frames[i] != nullptr;
        if (!frames[i]) continue;                                             // (the kernel does not read the frame of an image without one)
        uint16_t* q = dst + (size_t)i * w * hgt;
        if (stride_elems == w) memcpy(q, frames[i], (size_t)w * hgt * sizeof(uint16_t));
        else for (int y = 0; y < hgt; ++y) memcpy(q + (size_t)y * w, frames[i] + (size_t)y * stride_elems, (size_t)w * sizeof(uint16_t));
    }
    d.n = n_images; d.ext = nullptr;
    return OMNI_OK;
}

int omni_cam_set_depth_dev(omni_cam* c, const uint16_t* depth_dev, int stride_elems, const uint8_t* have_host, int n_images) {
    OMNI_REQUIRE(c && depth_dev, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = cam_depth_check(c, "omni_cam_set_depth_dev", stride_elems, n_images))) return rc;
    uint8_t* have = c->depth.host.as<uint8_t>() + c->depth.have_at;
    for (int i = 0; i < n_images; ++i) have[i] = have_host ? have_host[i] != 0 : 1;
    c->depth.n = n_images; c->depth.ext = depth_dev; c->depth.ext_stride = stride_elems;
    return OMNI_OK;
}

// ---- send_img inside the unit --------------------------------------------------------------------------------------------------------------------------
int omni_cam_set_jpeg(omni_cam* c, int quality, int64_t capacity_per_image) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_jpeg with a unit in flight (omni_cam_wait first)");
    CamJpegEnc& e = c->enc;
    if (quality == 0) { e.quality = 0; return OMNI_OK; }
    OMNI_REQUIRE(quality >= 1 && quality <= 100, OMNI_ERR_INVALID, "omni_cam_set_jpeg: quality %d outside 1..100 (0: off)", quality);
    OMNI_REQUIRE(capacity_per_image >= OMNI_JPEG_HEADER_BYTES + 2 && capacity_per_image <= 0x7fffffff, OMNI_ERR_INVALID,
                 "omni_cam_set_jpeg: a capacity of %lld bytes, the header and EOI alone take %d", (long long)capacity_per_image, OMNI_JPEG_HEADER_BYTES + 2);
    if (e.h && quality == e.quality && capacity_per_image == e.cap) return OMNI_OK;
    (void)hipSetDevice(c->c1->device);
    // (set-up time: the destroy and a buffer that grows wait for the device)
    if (e.h) { omni_jpeg_destroy(e.h); e.h = nullptr; }
    e.quality = 0;
    if (capacity_per_image != e.cap) {
        int rc;
        e.cap = 0;
        e.meta = ((size_t)c->n_cap * capacity_per_image + 255) & ~(size_t)255;
        const size_t bytes = e.meta + (size_t)2 * c->n_cap * 4;
        if ((rc = e.dev.ensure(bytes)) || (rc = e.host.ensure(bytes))) return rc;
        memset(e.host.p, 0, bytes);
        e.cap = capacity_per_image;
    }
    e.h = omni_jpeg_create(c->c2, c->W, c->H, c->n_cap, quality, capacity_per_image);
    if (!e.h) return OMNI_ERR_INVALID;                                        // (omni_jpeg_create left the message)
    e.quality = quality;
    return OMNI_OK;
}

int omni_cam_jpeg(omni_cam* c, omni_cam_jpeg_result* out) {
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_jpeg with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->enc.unit, OMNI_ERR_INVALID, "omni_cam_jpeg: the last unit ran with the stage off (omni_cam_set_jpeg)");
    out->n_images = c->enc.n; out->capacity = c->enc.cap; out->bytes = c->enc.host.as<uint8_t>();
    out->sizes = reinterpret_cast<const int*>(out->bytes + c->enc.meta); out->status = out->sizes + c->n_cap;
    return OMNI_OK;
}

// ---- the LoopNet wire inside the unit --------------------------------------------------------------------------------------------------------------------
int omni_cam_set_wire(omni_cam* c, int on, int send_all_features) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_wire with a unit in flight (omni_cam_wait first)");
    CamWire& w = c->wire;
    if (!on) { w.on = false; w.img_on = false; w.n_meta = 0; return OMNI_OK; }
    OMNI_REQUIRE(c->lm.on || c->depth.on, OMNI_ERR_INVALID,
                 "omni_cam_set_wire: the handle has no landmark model (omni_cam_set_stereo_model / omni_cam_set_depth_model): the stage packs landmarks the device made");
    OMNI_REQUIRE(c->D == WP_DESC_DIM && c->out_dim == WP_GLOBAL_DIM, OMNI_ERR_INVALID, "omni_cam_set_wire: descriptors of %d and global descriptors of %d floats, the wire carries %d and %d",
                 c->D, c->out_dim, WP_DESC_DIM, WP_GLOBAL_DIM);
    (void)hipSetDevice(c->c1->device);
    if (!w.cap) {                                    // (set-up time: no unit is in flight)
        int rc;
        const int64_t cap = omni::wp::capacity(c->M);
        const int te = omni::wp::table_ints(c->M);
        const size_t table_at = ((size_t)c->n_cap * cap + 255) & ~(size_t)255, meta_at = (table_at + (size_t)c->n_cap * te * sizeof(int) + 255) & ~(size_t)255;
        const size_t bytes = meta_at + (size_t)c->n_cap * sizeof(omni_wire_image_meta);
        if ((rc = w.dev.ensure(bytes)) || (rc = w.host.ensure(bytes))) return rc;
        if (!w.e_g) OMNI_HIP_TRY(hipEventCreateWithFlags(&w.e_g, hipEventDisableTiming));
        memset(w.host.p, 0, bytes);
        w.cap = cap; w.te = te; w.table_at = table_at; w.meta_at = meta_at;
    }
    w.on = true; w.send_all = send_all_features != 0; w.n_meta = 0;
    return OMNI_OK;
}

int omni_cam_set_wire_meta(omni_cam* c, const omni_wire_image_meta* records, int n_images) {
    OMNI_REQUIRE(c && records, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_wire_meta with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->wire.on, OMNI_ERR_INVALID, "omni_cam_set_wire_meta with the wire stage off (omni_cam_set_wire)");
    OMNI_REQUIRE(n_images >= 1 && n_images <= c->n_cap, OMNI_ERR_INVALID, "omni_cam_set_wire_meta: %d images, the handle holds 1..%d main images", n_images, c->n_cap);
    memcpy(c->wire.host.as<uint8_t>() + c->wire.meta_at, records, (size_t)n_images * sizeof(omni_wire_image_meta));
    c->wire.n_meta = n_images;
    return OMNI_OK;
}

int omni_cam_wire(omni_cam* c, omni_cam_wire_result* out) {
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_wire with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->wire.unit, OMNI_ERR_INVALID, "omni_cam_wire: the last unit ran with the stage off (omni_cam_set_wire)");
    out->n_images = c->wire.n; out->max_num = c->M; out->table_ints = c->wire.te; out->capacity = c->wire.cap;
    out->packets = c->wire.host.as<uint8_t>(); out->table = reinterpret_cast<const int*>(out->packets + c->wire.table_at);
    return OMNI_OK;
}

// the whole descriptor behind the packets above: with_features and with_image both 0 switch it off again
int omni_cam_set_wire_image(omni_cam* c, int with_features, int with_image) {
    OMNI_REQUIRE(c, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_set_wire_image with a unit in flight (omni_cam_wait first)");
    CamWire& w = c->wire;
    if (!with_features && !with_image) { w.img_on = false; return OMNI_OK; }
    OMNI_REQUIRE(w.on, OMNI_ERR_INVALID, "omni_cam_set_wire_image with the wire stage off (omni_cam_set_wire): the whole descriptor follows an image's packets");
    OMNI_REQUIRE(!with_image || c->enc.quality, OMNI_ERR_INVALID, "omni_cam_set_wire_image: with_image, but the unit encodes no JPEG files (omni_cam_set_jpeg)");
    const int64_t jcap = with_image ? c->enc.cap : 0;
    OMNI_REQUIRE(jcap % 4 == 0 && jcap <= WP_MAX_JPEG_CAPACITY, OMNI_ERR_INVALID,
                 "omni_cam_set_wire_image: the JPEG stage's capacity of %lld bytes per image is above 2^30 or no multiple of 4: a file's row would not be 4-byte aligned",
                 (long long)jcap);
    (void)hipSetDevice(c->c1->device);
    const int64_t cap = omni::wp::whole_capacity(c->M, jcap);
    if (cap != w.img_cap) {                          // (set-up time: no unit is in flight)
        int rc;
        w.img_on = false; w.img_cap = 0;
        const size_t sizes_at = ((size_t)c->n_cap * cap + 255) & ~(size_t)255, bytes = sizes_at + (size_t)c->n_cap * 2 * sizeof(int);
        if ((rc = w.img_dev.ensure(bytes)) || (rc = w.img_host.ensure(bytes))) return rc;
        memset(w.img_host.p, 0, bytes);
        w.img_cap = cap; w.img_sizes_at = sizes_at;
    }
    if (!w.e_j) OMNI_HIP_TRY(hipEventCreateWithFlags(&w.e_j, hipEventDisableTiming));
    w.img_jcap = jcap; w.img_features = with_features != 0; w.img_file = with_image != 0; w.img_on = true;
    return OMNI_OK;
}

int omni_cam_wire_image(omni_cam* c, omni_cam_wire_image_result* out) {
    OMNI_REQUIRE(c && out, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    OMNI_REQUIRE(!c->pending, OMNI_ERR_INVALID, "omni_cam_wire_image with a unit in flight (omni_cam_wait first)");
    OMNI_REQUIRE(c->wire.img_unit, OMNI_ERR_INVALID, "omni_cam_wire_image: the last unit ran with the stage off (omni_cam_set_wire_image)");
    out->n_images = c->wire.n; out->capacity = c->wire.img_cap; out->with_features = c->wire.img_features; out->with_image = c->wire.img_file;
    out->packets = c->wire.img_host.as<uint8_t>(); out->sizes = reinterpret_cast<const int*>(out->packets + c->wire.img_sizes_at);
    return OMNI_OK;
}

// non-blocking: *ready = 1 when omni_cam_wait would return at once (or nothing is pending)
int omni_cam_ready(omni_cam* c, int* ready) {
    OMNI_REQUIRE(c && ready, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *ready = 1;
    if (!c->pending) return OMNI_OK;
    (void)hipSetDevice(c->c1->device);
    for (hipEvent_t e : {c->core.e1, c->core.e2}) {
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
    OMNI_HIP_TRY(hipEventSynchronize(c->core.e1));
    OMNI_HIP_TRY(hipEventSynchronize(c->core.e2));
    c->pending = false;
    const CamCore& k = c->core; const char* h = k.host;
    out->n_dirs = c->n; out->max_num = c->M; out->desc_dim = c->D; out->global_dim = c->out_dim; out->n_images = c->cams * c->n;
    out->kps_xy = reinterpret_cast<const float*>(h + k.off_kps);
    out->n_kps = reinterpret_cast<const int*>(h + k.off_n);
    out->desc = reinterpret_cast<const float*>(h + k.off_desc);
    out->scores = reinterpret_cast<const float*>(h + k.off_sc);
    out->global_desc = reinterpret_cast<const float*>(h + k.off_g);
    out->match_up = reinterpret_cast<const int*>(h + k.off_q);
    out->match_down = reinterpret_cast<const int*>(h + k.off_t);
    out->match_dist = reinterpret_cast<const float*>(h + k.off_d);
    out->n_matches = reinterpret_cast<const int*>(h + k.off_nm);
    return OMNI_OK;
}

}  // extern "C"
