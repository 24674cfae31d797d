// Internal helpers shared by the HIP translation units of libomni_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/omni_hip.h"

namespace omni {

void set_error(const char* fmt, ...);

#define OMNI_HIP_TRY(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            ::omni::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return OMNI_ERR_HIP;                                                             \
        }                                                                                    \
    } while (0)

#define OMNI_REQUIRE(cond, code, ...)                                                        \
    do {                                                                                     \
        if (!(cond)) { ::omni::set_error(__VA_ARGS__); return (code); }                      \
    } while (0)

#define OMNI_LAUNCH_CHECK()                                                                  \
    do {                                                                                     \
        hipError_t _e = hipGetLastError();                                                   \
        if (_e != hipSuccess) {                                                              \
            ::omni::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return OMNI_ERR_HIP;                                                             \
        }                                                                                    \
    } while (0)

// roctx ranges around the stages of the hot path (ctx.hip; OMNI_ROCTX=1: librocprofiler-sdk-roctx / libroctx64 resolved by dlopen, like RCCL): what the
// reference's per-stage timers print (superpoint_tensorrt.cpp:130-162, loop_cam.cpp:205-207) becomes a `rocprofv3 --marker-trace` timeline.  No-ops when off.
void trace_push(const char* name);
void trace_pop();
struct TraceRange { explicit TraceRange(const char* name) { trace_push(name); } ~TraceRange() { trace_pop(); } TraceRange(const TraceRange&) = delete; };

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: remember what was set per (kernel instantiation, device)
// instead of per process, so that a process driving several GPUs through several omni_ctx stays correct.  One static State per call site.
struct DynSmemState { size_t set[16] = {0}; };
static inline hipError_t ensure_dyn_smem(DynSmemState& st, const void* kfn, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 16 && st.set[dev] >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev >= 0 && dev < 16) st.set[dev] = bytes;
    return e;
}
static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grow-only device scratch buffer.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return OMNI_OK;
        // hipFree waits for the WHOLE device to go idle: a buffer whose need creeps up with the database (the key lists of a scan: 8 bytes per row per
        // query) must not be reallocated at every micro-batch -- that made the host wait for the key-frame unit in flight each time it enqueued a search
        // (2.7 ms of a 3.8 ms cycle, round 4).  Grow by half at least: a handful of reallocations over a database's life.
        size_t want = bytes + bytes / 2;
        if (want < need) want = need;
        want = (want + 4095) & ~(size_t)4095;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            want = need;                                    // no room for the slack: the exact size
            OMNI_HIP_TRY(hipMalloc(&p, want));
        }
        bytes = want;
        return OMNI_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Every device allocation of a handle (omni_sp, omni_vlad): what alloc() handed out is what the handle's destroy frees -- also after a creation that
// failed half way -- with no list to keep next to the struct's pointers
struct DevMem {
    std::vector<void*> ptrs;
    template <typename T>
    int alloc(T** p, size_t bytes, hipStream_t st = nullptr, bool zero = false) {
        void* q = nullptr;
        OMNI_HIP_TRY(hipMalloc(&q, bytes));
        ptrs.push_back(q);
        *p = static_cast<T*>(q);
        if (zero) OMNI_HIP_TRY(hipMemsetAsync(q, 0, bytes, st));
        return OMNI_OK;
    }
    void release(void* one, bool all) {
        for (void*& q : ptrs)
            if (q && (all || q == one)) { (void)hipFree(q); q = nullptr; }
    }
    void release_one(void* p) { release(p, false); }        // a lazy buffer that has to grow (null: nothing)
    void release_all() { release(nullptr, true); ptrs.clear(); }
};

// Pinned host staging buffer.
struct HostBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return OMNI_OK;
        size_t want = bytes + bytes / 2;                    // (as DevBuf: hipHostFree synchronises too)
        if (want < need) want = need;
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0;
        OMNI_HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        bytes = want;
        return OMNI_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace omni

extern "C" hipEvent_t omni_sp_convs_event(omni_sp* s);      // internal (superpoint.hip -> cam.hip): recorded behind a pass's convolution stack

#define OMNI_ZERO_PAGE_BYTES 65536

struct omni_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_order = nullptr;     // omni_ctx_order_after: marks this stream's position for another stream to wait on
    hipDeviceProp_t prop;
    std::mutex mu;
    // 64 KB of zeros in HBM, never written after creation: the LDS-DMA source of convolution halo pixels outside the image.  A lane reads the
    // 16 bytes at (its would-be image offset mod 64 KB), so the requests spread over the L2 channels: with ONE shared line the rate depended
    // on where the allocator happened to put it (7 % of the whole pipeline between two placements)
    void* zero_page = nullptr;
    omni::DevBuf scratch;     // generic per-call scratch (bf match, host-entry staging)
    omni::DevBuf scratch2;
    omni::HostBuf hstage;
    omni::DevBuf ransac_T;    // homography.hip: the stop rule's table T[count][good] for count <= ransac_T_n (csrc/ransac_plan.h), filled once
    int ransac_T_n = 0;
    std::vector<std::vector<int>> pnp_T;      // pnp.hip: the PnP RANSAC's stop-rule rows T[good] by count (csrc/pnp_plan.h), each filled on first use; on the host
    int ensure_zero_page() {
        if (zero_page) return OMNI_OK;
        OMNI_HIP_TRY(hipMalloc(&zero_page, OMNI_ZERO_PAGE_BYTES));
        OMNI_HIP_TRY(hipMemsetAsync(zero_page, 0, OMNI_ZERO_PAGE_BYTES, stream));
        return OMNI_OK;
    }
};

// omni_flatten (flatten.hip): a fisheye camera's undistortion maps in HBM, immutable after creation.  cam.hip reads the view table to check a raw key
// frame against its unit and hands the maps to flatten_unit_launch
struct omni_flatten {
    omni_ctx* ctx = nullptr;
    int src_w = 0, src_h = 0, n_views = 0;
    std::vector<int> vw, vh;
    std::vector<int64_t> out_off;          // byte offset of view v inside one image's output block
    int64_t out_bytes = 0;                 // per source image
    float* maps = nullptr;                 // all views back to back, [h][w][2]; every view starts on a 16-byte boundary
    int* meta = nullptr;                   // per view: w, h, map offset (in float2), out offset
    std::mutex mu;
};

namespace omni {
// flatten.hip: remaps n_images raw fisheye frames of ONE camera (u8, src_stride) into views [first_view, first_view + dirs) of f, all width x height, written
// as [image][view][row][x] with packed rows at out_dev -- a key-frame unit's input block for that camera.  fisheye_mask != 0: the rows
// omni_fisheye_mask_rows names are written as zeros.  Asynchronous on `stream`; the caller has checked the view sizes.
int flatten_unit_launch(const omni_flatten* f, hipStream_t stream, const uint8_t* src_dev, int src_stride, int n_images, int first_view, int dirs, int width,
                        int height, int fisheye_mask, uint8_t* out_dev);
}  // namespace omni

// omni_resize (resize.hip): the four tables of one source size -> destination size (resize_plan.h) in HBM, immutable after creation.  cam.hip reads the sizes
// to check a unit of raw stereo frames and hands the object to resize_unit_launch
struct omni_resize {
    omni_ctx* ctx = nullptr;
    int mode = 0, src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
    uint8_t* tables = nullptr;             // one allocation: xofs int32 [W] | ialpha int16 [W][2] | yofs int32 [H] | ibeta int16 [H][2], each part on 16 bytes
    const int32_t *xofs = nullptr, *yofs = nullptr;
    const int16_t *ialpha = nullptr, *ibeta = nullptr;
    std::mutex mu;
};

namespace omni {
// resize.hip: n_images frames (u8, src_stride, frame i at + i * src_stride * source height) -> n_images images of the object's destination size, rows packed,
// back to back at out_dev (4-byte aligned).  Asynchronous on `stream`, which need not be the object's own.
int resize_unit_launch(const omni_resize* r, hipStream_t stream, const uint8_t* src_dev, int src_stride, int n_images, uint8_t* out_dev);
}  // namespace omni

namespace omni {
// landmarks.hip: the stereo landmarks of n_pairs image pairs (landmark_plan.h) -- pair p = up image p of the *_up arrays and down image p of the *_down arrays,
// key frame p / m.dirs_per_keyframe of poses7_dev.  Asynchronous on `stream`; the caller has checked the model (landmarks_check_model) and the sizes.
int landmarks_launch(hipStream_t stream, const omni_stereo_model& m, const omni_camera_model& cm, const double* poses7_dev, int n_pairs, int max_num, const float* kps_up, const float* kps_down,
                     const int* n_up, const int* n_down, const int* match_up, const int* match_down, const int* n_matches, float* norm_up, float* norm_down,
                     float* l3d_up, float* l3d_down, uint8_t* flag_up, uint8_t* flag_down, int* count);
int landmarks_check_model(const omni_stereo_model* m);
int landmarks_check_camera(const omni_camera_model* cm);      // csrc/camera_plan.h's cam::check as an error code
// depth_landmarks.hip: the depth landmarks of n_images images of ONE camera each (csrc/depth_plan.h); image i reads pose i of poses7_dev, depth image i of `depth`
// (stride in elements) and have[i] (nullptr: all).  Asynchronous on `stream`; the caller has checked the model (depth_check_model), the lens and the sizes.
int depth_landmarks_launch(hipStream_t stream, const omni_depth_model& m, const omni_camera_model& cm, const double* poses7_dev, int n_images, int max_num, const float* kps_xy,
                           const int* n_kps, const uint16_t* depth, int stride, const uint8_t* have, float* norm2d, float* l3d, uint8_t* flag, int* count);
int depth_check_model(const omni_depth_model* m);
// wire_pack.hip: LoopNet's packets of n_images images out of a unit's arrays (csrc/wire_plan.h); the caller has checked what omni_wire_pack_enqueue_dev refuses
int wire_pack_launch(hipStream_t stream, int n_images, int max_num, int send_all_features, const float* kps_xy, const int* n_kps, const float* desc, const float* norm2d,
                     const float* l3d, const uint8_t* flag, const float* global, const omni_wire_image_meta* meta, uint8_t* out, int* table);
// ... and their whole descriptors (wire_plan.h whole_*), with the JPEG files jpeg [n_images][jpeg_capacity] (null without with_image); the caller has checked what
// omni_wire_pack_image_enqueue_dev refuses
int wire_pack_image_launch(hipStream_t stream, int n_images, int max_num, int with_features, int with_image, const float* kps_xy, const int* n_kps, const float* desc,
                           const float* norm2d, const float* l3d, const uint8_t* flag, const float* global, const omni_wire_image_meta* meta, const uint8_t* jpeg,
                           const int* jpeg_sizes, const int* jpeg_status, int64_t jpeg_capacity, int width, int height, uint8_t* out, int* sizes_out);
}  // namespace omni

struct omni_jpeg;
namespace omni {
// jpeg.hip: n_images images as JPEG files (jpeg_plan.h) -- out_dev [n_images][the handle's capacity], sizes_dev / status_dev [n_images].  Asynchronous on `stream`,
// which need not be the handle's own; jpeg_check_enqueue first.
int jpeg_check_enqueue(const omni_jpeg* j, int stride, int n_images, int zero_from_row);
int jpeg_launch(omni_jpeg* j, hipStream_t stream, const uint8_t* gray_dev, int stride, int n_images, int zero_from_row, uint8_t* out_dev, int* sizes_dev,
                int* status_dev);
}  // namespace omni

struct omni_jpegdec;
namespace omni {
// jpeg_dec.hip: n_images JPEG files -> gray pictures at out_dev (picture i at + i * out_stride * the handle's height), status_dev [n_images] -- parse, pack, ONE
// upload and the kernels on `stream`, which need not be the handle's own.  Refuses before anything is enqueued (an UNSUPPORTED file, another size)
int jpegdec_enqueue_on(omni_jpegdec* d, hipStream_t stream, const uint8_t* const* files, const int64_t* sizes, int n_images, uint8_t* out_dev, int out_stride,
                       int* status_dev);
}  // namespace omni

namespace omni {
// pca_fit.hip: the rows of one SuperPoint pass (csrc/pca_plan.h) added to the fit's accumulator on `stream`, which must be the fit's own context's (a fit is
// attached only to a handle of its own context: omni_sp_set_pcafit)
int pcafit_enqueue_on(omni_pcafit* f, hipStream_t stream, const float* raw_desc, const float* norm_partial, const int* n_kps, int batch, int max_num);
const omni_ctx* pcafit_ctx(const omni_pcafit* f);
int pcafit_set_owner(omni_pcafit* f, omni_sp* sp_or_null);      // the handle that holds the fit (nullptr: none); refused while another handle holds it
void sp_drop_pcafit(omni_sp* sp, omni_pcafit* f);               // superpoint.hip: sp stops feeding f, if it does (omni_pcafit_destroy of an attached fit)
}  // namespace omni

// ---- 64-bit sortable keys -------------------------------------------------------------------------------------
// key = (orderable(score) << 32) | (0xFFFFFFFF - id): descending key order == (score desc, id asc).
__host__ __device__ static inline uint32_t omni_f32_orderable(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float omni_orderable_f32(uint32_t o) {
    uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(u);
#else
    memcpy(&f, &u, 4);
#endif
    return f;
}
__host__ __device__ static inline uint64_t omni_make_key(float score, uint32_t id) {
    return ((uint64_t)omni_f32_orderable(score) << 32) | (uint64_t)(0xFFFFFFFFu - id);
}
#define OMNI_KEY_EMPTY 0ull   // sorts last; decodes to id 0xFFFFFFFF -> reported as -1
