// omni_wire_pack_*: a key frame's images as LoopNet's packets (swarm_loop/src/loop_net.cpp:19-101 broadcast_fisheye_desc / broadcast_img_desc) on the GPU, out of the
// arrays a key-frame unit leaves in HBM.  The layout is wire_plan.h's -- this file only spreads it over lanes:
//   one workgroup per image, 256 lanes (4 waves); an image without key points writes its all-zero table and leaves;
//   compact  which landmarks are sent, in index order: a ballot per wave and pass (<= 4 passes of 256 slots: max_num <= 1024), a lane's rank = popcount of the ballot
//            below it, the 16 (pass, wave) counts through LDS, every lane sums the ones in front of its own; the order goes into LDS.  feature_num = the flagged
//            ones, counted the same way.  No atomics;
//   header   the 161 misaligned bytes in front of the float area (with 3 bytes of padding: 164) one byte per lane into LDS, then 41 dword stores; the 4096 floats a
//            coalesced sweep of byte-swapped dwords;
//   packets  one wave per landmark packet in turn: 81 dwords = one store of 64 lanes and one of 17;
//   table    lanes over its entries.
// No workgroup reads what another wrote, none waits for another; every loop's trip count is bounded by max_num, a launch argument.
#include "common.h"
#include "wire_plan.h"

namespace omni {

#define WP_THREADS 256
#define WP_WAVES (WP_THREADS / 64)
#define WP_PASSES (WP_MAX_NUM / WP_THREADS)

__global__ __launch_bounds__(WP_THREADS) void wire_pack_kernel(int n_images, int max_num, int send_all_features, const float* __restrict__ kps_xy,
                                                               const int* __restrict__ n_kps, const float* __restrict__ desc, const float* __restrict__ norm2d,
                                                               const float* __restrict__ l3d, const uint8_t* __restrict__ flag, const float* __restrict__ global,
                                                               const omni_wire_image_meta* __restrict__ meta, uint8_t* __restrict__ out, int* __restrict__ table) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_images) return;
    __shared__ int chunk_sent[WP_PASSES * WP_WAVES], chunk_flagged[WP_PASSES * WP_WAVES];
    __shared__ uint16_t order[WP_MAX_NUM];
    __shared__ uint32_t head[WP_HEAD_DWORDS];
    const int n = wp::clamp_count(n_kps[g], max_num), te = wp::table_ints(max_num);
    int* tb = table + (size_t)g * te;
    if (!wp::image_sent(n)) {                                 // (uniform over the workgroup)
        for (int e = lane; e < te; e += WP_THREADS) tb[e] = wp::table_entry(e, -1);
        return;
    }
    const size_t at = (size_t)g * max_num;
    const float *kp = kps_xy + at * 2, *ds = desc + at * WP_DESC_DIM, *nm = norm2d + at * 2, *l3 = l3d + at * 3, *gl = global + (size_t)g * WP_GLOBAL_DIM;
    const uint8_t* fl = flag + at;
    const int wave = lane >> 6, wl = lane & 63;
    const unsigned long long below = (1ull << wl) - 1;
    int rank[WP_PASSES];
    bool sent[WP_PASSES];
#pragma unroll
    for (int p = 0; p < WP_PASSES; ++p) {                     // (every lane of a wave reaches both ballots)
        const int i = p * WP_THREADS + lane;
        const uint8_t f = i < n ? fl[i] : (uint8_t)0;
        sent[p] = wp::landmark_sent(i, n, f, send_all_features);
        const unsigned long long ms = __ballot(sent[p]), mc = __ballot(wp::landmark_counted(i, n, f));
        rank[p] = __popcll(ms & below);
        if (wl == 0) { chunk_sent[p * WP_WAVES + wave] = __popcll(ms); chunk_flagged[p * WP_WAVES + wave] = __popcll(mc); }
    }
    __syncthreads();
    int n_sent = 0, feature_num = 0, base[WP_PASSES];
#pragma unroll
    for (int c = 0; c < WP_PASSES * WP_WAVES; ++c) {
        if ((c % WP_WAVES) == wave) base[c / WP_WAVES] = n_sent;
        n_sent += chunk_sent[c];
        feature_num += chunk_flagged[c];
    }
#pragma unroll
    for (int p = 0; p < WP_PASSES; ++p)
        if (sent[p]) order[base[p] + rank[p]] = (uint16_t)(p * WP_THREADS + lane);
    if (lane < WP_HEAD_PADDED) reinterpret_cast<uint8_t*>(head)[lane] = wp::head_byte(lane, meta[g], feature_num);
    __syncthreads();
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out + (size_t)g * wp::capacity(max_num));
    if (lane < WP_HEAD_DWORDS) o32[lane] = head[lane];
    for (int j = lane; j < WP_GLOBAL_DIM; j += WP_THREADS) o32[WP_HEAD_DWORDS + j] = __builtin_bswap32(wp::f32_bits(gl + j));
    for (int k = wave; k < n_sent; k += WP_WAVES) {           // n_sent <= n <= max_num
        const int i = order[k];
        uint32_t* dst = o32 + WP_LANDMARKS_AT / 4 + WP_LANDMARK_DWORDS * k;
        dst[wl] = wp::landmark_dword(wl, i, meta[g].drone_id, kp, ds, nm, l3, fl);
        if (wl < WP_LANDMARK_DWORDS - 64) dst[64 + wl] = wp::landmark_dword(64 + wl, i, meta[g].drone_id, kp, ds, nm, l3, fl);
    }
    for (int e = lane; e < te; e += WP_THREADS) tb[e] = wp::table_entry(e, n_sent);
}
static_assert(WP_HEAD_PADDED <= WP_THREADS && WP_LANDMARK_DWORDS > 64 && WP_LANDMARK_DWORDS <= 128, "lane coverage");

const char* wire_pack_refusal(int n_images, int max_num, int desc_dim, int global_dim);      // wire_pack_host.cpp

int wire_pack_launch(hipStream_t stream, int n_images, int max_num, int send_all_features, const float* kps_xy, const int* n_kps, const float* desc, const float* norm2d,
                     const float* l3d, const uint8_t* flag, const float* global, const omni_wire_image_meta* meta, uint8_t* out, int* table) {
    hipLaunchKernelGGL(wire_pack_kernel, dim3(n_images), dim3(WP_THREADS), 0, stream, n_images, max_num, send_all_features, kps_xy, n_kps, desc, norm2d, l3d, flag,
                       global, meta, out, table);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

// The third packet of an image, the whole descriptor (SWARM_LOOP_IMG_DES; wire_plan.h whole_*): one workgroup per image, 256 lanes, no atomics, nothing read that
// another workgroup wrote.
//   head    its misaligned bytes (with 3 bytes of padding) one byte per lane into LDS, then dword stores;
//   floats  image_desc, the descriptors when they travel, the three landmark arrays: ALL landmark_num landmarks, one coalesced sweep of byte-swapped dwords;
//   tail    landmark_num flag bytes, then the JPEG file the unit's encode stage left in HBM.  The file starts at an arbitrary byte of its destination and on a dword
//           of its source, so a lane puts each output dword together from two neighbouring source dwords (wp::whole_tail_dword); the last dword is completed with
//           zeros.  Plain vector stores.
// Trip counts: landmark_num is clamped to max_num and image_size to jpeg_capacity before any loop, both launch arguments.
__global__ __launch_bounds__(WP_THREADS) void wire_pack_image_kernel(int n_images, int max_num, int with_features, int with_image, int jpeg_capacity, int width, int height,
                                                                     const float* __restrict__ kps_xy, const int* __restrict__ n_kps, const float* __restrict__ desc,
                                                                     const float* __restrict__ norm2d, const float* __restrict__ l3d, const uint8_t* __restrict__ flag,
                                                                     const float* __restrict__ global, const omni_wire_image_meta* __restrict__ meta,
                                                                     const uint8_t* __restrict__ jpeg, const int* __restrict__ jpeg_sizes,
                                                                     const int* __restrict__ jpeg_status, uint8_t* __restrict__ out, int* __restrict__ sizes_out) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_images) return;
    __shared__ uint32_t head[WP_IMAGE_HEAD_DWORDS];
    const int n = wp::clamp_count(n_kps[g], max_num);
    if (!wp::image_sent(n)) {                                 // (uniform over the workgroup)
        if (lane < 2) sizes_out[2 * g + lane] = 0;
        return;
    }
    const int isz = with_image ? wp::whole_image_size(1, jpeg_status[g], jpeg_sizes[g], jpeg_capacity) : 0;      // 0 <= isz <= jpeg_capacity
    const int ff = wp::whole_feature_floats(n, with_features), fd = wp::whole_float_dwords(n, with_features);
    const size_t at = (size_t)g * max_num;
    const float *kp = kps_xy + at * 2, *ds = desc + at * WP_DESC_DIM, *nm = norm2d + at * 2, *l3 = l3d + at * 3, *gl = global + (size_t)g * WP_GLOBAL_DIM;
    const uint8_t *fl = flag + at, *jr = with_image ? jpeg + (size_t)g * jpeg_capacity : nullptr;
    if (lane < WP_IMAGE_HEAD_PADDED) reinterpret_cast<uint8_t*>(head)[lane] = wp::whole_head_byte(lane, meta[g], n, width, height, ff, isz);
    __syncthreads();
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out + (size_t)g * wp::whole_capacity(max_num, jpeg_capacity));
    if (lane < WP_IMAGE_HEAD_DWORDS) o32[lane] = head[lane];
    uint32_t* fa = o32 + WP_IMAGE_HEAD_DWORDS;
    for (int j = lane; j < fd; j += WP_THREADS) fa[j] = wp::whole_float_dword(j, n, ff, gl, ds, nm, kp, l3);       // fd <= 4096 + 71 * max_num
    uint32_t* ta = fa + fd;
    const int td = (n + isz + 3) >> 2;                                                                              // <= (max_num + jpeg_capacity + 3) / 4
    for (int d = lane; d < td; d += WP_THREADS) ta[d] = wp::whole_tail_dword(d, n, isz, fl, jr);
    if (lane < 2) sizes_out[2 * g + lane] = lane == 0 ? WP_IMAGE_OFFSET : wp::whole_packet_bytes(n, with_features, isz);
}
static_assert(WP_IMAGE_HEAD_PADDED <= WP_THREADS, "lane coverage of the whole descriptor's head");

const char* wire_pack_image_refusal(int with_image, const void* jpeg, const void* jpeg_sizes, const void* jpeg_status, int64_t jpeg_capacity);      // wire_pack_host.cpp

int wire_pack_image_launch(hipStream_t stream, int n_images, int max_num, int with_features, int with_image, const float* kps_xy, const int* n_kps, const float* desc,
                           const float* norm2d, const float* l3d, const uint8_t* flag, const float* global, const omni_wire_image_meta* meta, const uint8_t* jpeg,
                           const int* jpeg_sizes, const int* jpeg_status, int64_t jpeg_capacity, int width, int height, uint8_t* out, int* sizes_out) {
    hipLaunchKernelGGL(wire_pack_image_kernel, dim3(n_images), dim3(WP_THREADS), 0, stream, n_images, max_num, with_features, with_image, (int)jpeg_capacity, width, height,
                       kps_xy, n_kps, desc, norm2d, l3d, flag, global, meta, jpeg, jpeg_sizes, jpeg_status, out, sizes_out);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

}  // namespace omni

extern "C" int omni_wire_pack_image_enqueue_dev(omni_ctx* ctx, int n_images, int max_num, int desc_dim, int global_dim, int with_features, int with_image,
                                                const float* kps_xy_dev, const int* n_kps_dev, const float* desc_dev, const float* norm2d_dev, const float* l3d_dev,
                                                const uint8_t* flag_dev, const float* global_dev, const omni_wire_image_meta* meta_dev, const uint8_t* jpeg_dev,
                                                const int* jpeg_sizes_dev, const int* jpeg_status_dev, int64_t jpeg_capacity, int image_width, int image_height,
                                                uint8_t* packets_out_dev, int* sizes_out_dev) {
    OMNI_REQUIRE(ctx && kps_xy_dev && n_kps_dev && desc_dev && norm2d_dev && l3d_dev && flag_dev && global_dev && meta_dev && packets_out_dev && sizes_out_dev,
                 OMNI_ERR_INVALID, "omni_wire_pack_image_enqueue_dev: null argument");
    const char* why = omni::wire_pack_refusal(n_images, max_num, desc_dim, global_dim);
    if (!why) why = omni::wire_pack_image_refusal(with_image, jpeg_dev, jpeg_sizes_dev, jpeg_status_dev, jpeg_capacity);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "omni_wire_pack_image_enqueue_dev: %s (n_images %d, max_num %d, desc_dim %d, global_dim %d, with_image %d, jpeg_capacity %lld)", why,
                 n_images, max_num, desc_dim, global_dim, with_image, (long long)jpeg_capacity);
    OMNI_REQUIRE((uintptr_t)packets_out_dev % 4 == 0 && (uintptr_t)jpeg_dev % 4 == 0, OMNI_ERR_INVALID,
                 "omni_wire_pack_image_enqueue_dev: packets_out or jpeg is not 4-byte aligned");
    omni::TraceRange trace_range("LoopNet wire pack (whole descriptor)");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    return omni::wire_pack_image_launch(ctx->stream, n_images, max_num, with_features != 0, with_image != 0, kps_xy_dev, n_kps_dev, desc_dev, norm2d_dev, l3d_dev, flag_dev,
                                        global_dev, meta_dev, jpeg_dev, jpeg_sizes_dev, jpeg_status_dev, jpeg_capacity, image_width, image_height, packets_out_dev,
                                        sizes_out_dev);
}

extern "C" int omni_wire_pack_enqueue_dev(omni_ctx* ctx, int n_images, int max_num, int desc_dim, int global_dim, int send_all_features, const float* kps_xy_dev,
                                          const int* n_kps_dev, const float* desc_dev, const float* norm2d_dev, const float* l3d_dev, const uint8_t* flag_dev,
                                          const float* global_dev, const omni_wire_image_meta* meta_dev, uint8_t* packets_out_dev, int* table_out_dev) {
    OMNI_REQUIRE(ctx && kps_xy_dev && n_kps_dev && desc_dev && norm2d_dev && l3d_dev && flag_dev && global_dev && meta_dev && packets_out_dev && table_out_dev,
                 OMNI_ERR_INVALID, "omni_wire_pack_enqueue_dev: null argument");
    const char* why = omni::wire_pack_refusal(n_images, max_num, desc_dim, global_dim);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "omni_wire_pack_enqueue_dev: %s (n_images %d, max_num %d, desc_dim %d, global_dim %d)", why, n_images, max_num, desc_dim,
                 global_dim);
    OMNI_REQUIRE((uintptr_t)packets_out_dev % 4 == 0, OMNI_ERR_INVALID, "omni_wire_pack_enqueue_dev: packets_out is not 4-byte aligned");
    omni::TraceRange trace_range("LoopNet wire pack");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    return omni::wire_pack_launch(ctx->stream, n_images, max_num, send_all_features != 0, kps_xy_dev, n_kps_dev, desc_dev, norm2d_dev, l3d_dev, flag_dev, global_dev,
                                  meta_dev, packets_out_dev, table_out_dev);
}
