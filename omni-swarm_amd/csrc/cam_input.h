// cam_input.h -- where the input bytes of a key-frame unit (cam.hip) go, stated once: how big the handle's two staging buffers must be, where every host part and
// every decoded frame lands in them, where each camera's pre-processing reads and writes, and in which order the steps run.  Plain C++ for g++ AND hipcc, nothing of
// HIP or of the handle: each omni_cam_enqueue_* entry fills a CamInput behind its own argument checks, cam_input_run (cam.hip) works from plan()'s answer alone, and
// tests/cpp/cam_input_pin.cpp prints the same answer for tests/test_cam_input_plan_cpu.py to compare with its own restatement.
// A camera's frames arrive as a device pointer (FORM_DEV), as segments of host memory (FORM_HOST: a single buffer is one part) or as JPEG files (FORM_FILES); they
// are handed to the networks as they are (PRE_NONE), remapped into views (PRE_FLATTEN) or resized (PRE_RESIZE).  d_gray is the unit's input block, cams * n images
// of W x H with packed rows, the second camera's n images behind the first camera's; d_raw holds the frames in front of a pre-processing.  The rules:
//   pixel paths   the raw bytes of f frames are (f * src_h - 1) * stride + src_w (the last row may end at its width); the second camera lies at the first camera's
//                 raw bytes rounded up to 256; a host part of k frames goes to frames_before * stride * src_h and copies the raw bytes of k frames.  Frames in HBM
//                 are read where they are: d_raw is not touched (raw_bytes = 0)
//   PRE_NONE      host parts go straight into d_gray, packed: part bytes k * W * H at (camera's half) + frames_before * W * H -- one 1-D copy when stride == width,
//                 a 2-D copy of k * H rows otherwise.  omni_cam_enqueue_host is the case of one part per camera: the first n * H rows, FENCE, the remaining rows
//                 (a mono handle has no second copy).  FORM_DEV reads the caller's buffer with the caller's stride and touches neither staging buffer
//   file paths    ONE decode of [first camera's frames | second camera's], packed: the output stride is src_w and the second camera lies at frames * src_w * src_h.
//                 The decoder holds files of max(w * h / 2, 1024) bytes and 2 * (n_cap / dirs) pictures for fisheye files, cams * n_cap otherwise.  With a
//                 pre-processing the decode writes d_raw, without one it writes d_gray directly and d_raw is not touched
//   mask          the unit's networks get fisheye_mask, but 0 on the resize paths and for plain files (loop_cam.cpp:536 blanks rows for STEREO_FISHEYE only)
//   step order    [DECODE_ALL, STATUS_DOWN,] then per camera [UPLOAD,] [PRE,] with ONE FENCE (record e_up on the SuperPoint stream, the MobileNetVLAD stream
//                 waits for it) behind the first camera's last step and in front of anything of the second camera, then UNIT
// Two differences between the arrival forms are kept on purpose; making either uniform changes behaviour and is not this header's business:
//   pending       the resize and file entries refuse a handle with a unit in flight; the dev, host, host_parts and fisheye pixel entries do not.  Each entry that
//                 refuses does so among its own checks, where its message has always stood in their order: the plan has no say in it
//   no FENCE      omni_cam_enqueue_dev (FORM_DEV, PRE_NONE) has no step but UNIT: nothing of it runs in front of the networks, and its MobileNetVLAD stream does
//                 not wait for its SuperPoint stream
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace omni::ci {

enum { FORM_DEV, FORM_HOST, FORM_FILES };
enum { PRE_NONE, PRE_FLATTEN, PRE_RESIZE };
enum { AT_CALLER, AT_GRAY, AT_RAW };                        // a camera's own device pointer, the handle's d_gray, its d_raw
enum { UPLOAD, DECODE_ALL, STATUS_DOWN, PRE, FENCE, UNIT };
constexpr int MAX_PARTS = 64, MAX_FRAMES = 128, MAX_STEPS = 8;      // (a handle holds 64 directions at the most: omni_cam_create)

struct CamInput {
    int form = FORM_DEV, pre = PRE_NONE;
    int cams = 2, n = 0, W = 0, H = 0, n_cap = 0;           // the handle: cameras, the unit's active size, the networks' size, what it was created for
    int src_w[2] = {0, 0}, src_h[2] = {0, 0}, stride = 0, frames = 0;      // each camera's frames (W x H with PRE_NONE), per camera; stride: of pixels, whatever the form (files: none)
    int first_view = 0, dirs = 1, fisheye_mask = 0;
    int n_parts[2] = {1, 1};                                // FORM_HOST: parts per camera, and the frames of each (nullptr: one part of all frames)
    const int* part_frames[2] = {nullptr, nullptr};
};
struct Part { size_t dst, bytes, rows; };                   // dst: in the stage buffer; rows != 0: a 2-D copy of so many rows of src_w bytes, source pitch stride
struct Step { int kind, cam; };
struct CamInputPlan {
    int n_steps = 0;                                        // 0: not a unit, nothing else of the plan may be used
    Step steps[MAX_STEPS];
    size_t gray_bytes = 0, raw_bytes = 0, gray_cam1 = 0, raw_cam1 = 0;      // bytes 0: the unit does not touch the buffer; cam1: the second camera's images in d_gray, its frames in d_raw
    int stage = AT_GRAY;                                    // where uploads and the decode write: d_raw in front of a pre-processing, else d_gray
    int n_parts[2] = {0, 0};
    Part part[2][MAX_PARTS];                                // (only [0, n_parts) of each camera is ever written or read)
    int dec_images = 0, dec_stride = 0, dec_w = 0, dec_h = 0, dec_max = 0;      // dec_images = 0: no decode; w, h, max, cap: what the decoder is made for
    int64_t dec_cap = 0;
    int pre_src = AT_RAW, pre_stride = 0;                   // a pre-processing reads the camera's own pointer or d_raw (+ raw_cam1) and writes d_gray (+ gray_cam1)
    int unit_src = AT_GRAY, unit_stride = 0, unit_mask = 0; // the networks read the caller's buffer or d_gray
};

inline size_t raw_span(const CamInput& in, int cam, size_t f) { return (f * in.src_h[cam] - 1) * in.stride + in.src_w[cam]; }

// n_steps = 0 for what is not a unit: no frames, more parts or frames than a handle holds, parts that do not add up to the camera's frames.  (The entries' own
// checks refuse all of these first; the test here is what keeps the plan's fixed tables from being overrun whoever calls)
inline CamInputPlan plan(const CamInput& in) {
    CamInputPlan p;
    if (in.cams < 1 || in.cams > 2 || in.frames < 1 || in.cams * in.frames > MAX_FRAMES || in.dirs < 1) return p;
    const bool files = in.form == FORM_FILES, host = in.form == FORM_HOST, pre = in.pre != PRE_NONE;
    const size_t half = (size_t)in.n * in.W * in.H, frame = (size_t)in.src_w[0] * in.src_h[0];
    p.gray_bytes = files || host || pre ? in.cams * half : 0;
    p.gray_cam1 = half;
    p.stage = pre ? AT_RAW : AT_GRAY;
    p.pre_src = in.form == FORM_DEV ? AT_CALLER : AT_RAW;
    p.pre_stride = files ? in.src_w[0] : in.stride;
    p.unit_src = p.gray_bytes ? AT_GRAY : AT_CALLER;
    p.unit_stride = p.gray_bytes ? in.W : in.stride;
    p.unit_mask = in.pre == PRE_RESIZE || (files && !pre) ? 0 : in.fisheye_mask;
    if (files) {
        p.dec_images = in.cams * in.frames; p.dec_stride = p.dec_w = in.src_w[0]; p.dec_h = in.src_h[0];
        p.dec_cap = (int64_t)frame / 2 > 1024 ? (int64_t)frame / 2 : 1024;      // (a larger file is decoded on the calling thread: same pixels)
        p.dec_max = in.pre == PRE_FLATTEN ? 2 * (in.n_cap / in.dirs) : in.cams * in.n_cap;
        if (pre) { p.raw_bytes = p.dec_images * frame; p.raw_cam1 = in.frames * frame; }
    } else if (pre && host) {
        p.raw_cam1 = (raw_span(in, 0, in.frames) + 255) & ~(size_t)255;
        p.raw_bytes = in.cams == 2 ? p.raw_cam1 + raw_span(in, 1, in.frames) : raw_span(in, 0, in.frames);
    }
    for (int cam = 0; host && cam < in.cams; ++cam) {
        if (in.n_parts[cam] < 1 || in.n_parts[cam] > MAX_PARTS) return p;
        size_t before = 0;
        for (int i = 0; i < in.n_parts[cam]; ++i, ++p.n_parts[cam]) {
            const int k = in.part_frames[cam] ? in.part_frames[cam][i] : in.frames;
            if (k < 1) return p;
            if (pre) p.part[cam][i] = {(cam ? p.raw_cam1 : 0) + before * in.stride * in.src_h[cam], raw_span(in, cam, k), 0};
            else p.part[cam][i] = {cam * half + before * frame, k * frame, in.stride != in.src_w[0] ? (size_t)k * in.src_h[0] : 0};
            before += k;
        }
        if (before != (size_t)in.frames) return p;
    }
    auto add = [&p](int kind, int cam) { p.steps[p.n_steps++] = {kind, cam}; };
    if (files) { add(DECODE_ALL, 0); add(STATUS_DOWN, 0); }
    for (int cam = 0; cam < in.cams && p.gray_bytes; ++cam) {
        if (host) add(UPLOAD, cam);
        if (pre) add(PRE, cam);
        if (cam == 0) add(FENCE, 0);
    }
    add(UNIT, 0);
    return p;
}

}  // namespace omni::ci
