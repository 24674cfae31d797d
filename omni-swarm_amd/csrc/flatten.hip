// omni_flatten_*: fisheye -> virtual pinhole views ("flattening") on the GPU: the cv::cuda::remap(INTER_LINEAR) calls of
// FisheyeUndist::undist_all_cuda (swarm_localization/test/fisheye_undist.hpp:57-90; VINS-Fisheye runs the same class in front of swarm_loop,
// SURVEY.md 8f rank 4).  The undistortion maps (generateAllUndistMap, :118-186: one float (x, y) source coordinate per output pixel and
// view) are made on the host (host/fisheye_flatten.hpp) and live in HBM; one launch remaps a batch of fisheye images into all views,
// written back to back so that the result can be handed to omni_cam_enqueue_dev / omni_sp_enqueue_dev without leaving the GPU.
// Interpolation = cv::cuda's LinearFilter with BORDER_CONSTANT(0): floor, four taps weighted (x2-x)(y2-y) ... in float, saturate_cast<uchar>
// (round half to even); the products and sums are rounded one by one (no FMA contraction) so that the numpy oracle reproduces the bytes.
// OpenCV is un-vendored: PARITY UNPINNED.  1 output byte + ~4 gathered source bytes + 8 map bytes per pixel; bound by the gather instructions (docs/kernels.md).
// flatten_unit_kernel is the same remap for a key-frame unit (omni_cam_enqueue_fisheye_*, cam.hip): only the views and rows the unit's networks read.
#include "common.h"

namespace omni {

// One output pixel: the four taps around map coordinate m of image s, weighted in float, rounded half to even, saturated.
// every product and sum below must be rounded on its own: this file is compiled with -ffp-contract=off (Makefile; HIP's __fmul_rn / __fadd_rn
// are plain operators that hipcc would otherwise fuse into FMAs -- measured: 1 pixel in a million off by one)
// PAIR: the two taps of a row are neighbouring bytes and come in as ONE (unaligned) 16-bit load -- the same values, half the gather instructions, which is what
// bounds this kernel (docs/kernels.md).  No branch: the load address is clamped into the image (src_w >= 2) and a tap outside it is selected to zero
template <bool PAIR>
__device__ __forceinline__ uint32_t remap_pixel(const uint8_t* __restrict__ s, int src_stride, int src_w, int src_h, float2 m) {
    const int x1 = (int)floorf(m.x), y1 = (int)floorf(m.y), x2 = x1 + 1, y2 = y1 + 1;
    float t11, t12, t21, t22;
    if constexpr (PAIR) {
        const int xc = min(max(x1, 0), src_w - 2);
        auto row = [&](int y, float& a, float& b) {
            const int yc = min(max(y, 0), src_h - 1);
            uint16_t v;
            __builtin_memcpy(&v, s + (int64_t)yc * src_stride + xc, 2);
            const uint32_t lo = y == yc ? v & 255u : 0u, hi = y == yc ? v >> 8 : 0u;      // bytes xc, xc + 1 of row y, or zeros for a row outside
            a = (float)(x1 == xc ? lo : (x1 == xc + 1 ? hi : 0u));
            b = (float)(x2 == xc + 1 ? hi : (x2 == xc ? lo : 0u));
        };
        row(y1, t11, t12); row(y2, t21, t22);
    } else {
        auto at = [&](int y, int x) -> float { return (x >= 0 && x < src_w && y >= 0 && y < src_h) ? (float)s[(int64_t)y * src_stride + x] : 0.f; };
        t11 = at(y1, x1); t12 = at(y1, x2); t21 = at(y2, x1); t22 = at(y2, x2);
    }
    const float ax2 = __fsub_rn((float)x2, m.x), ax1 = __fsub_rn(m.x, (float)x1), ay2 = __fsub_rn((float)y2, m.y), ay1 = __fsub_rn(m.y, (float)y1);
    float acc = __fmul_rn(t11, __fmul_rn(ax2, ay2));
    acc = __fadd_rn(acc, __fmul_rn(t12, __fmul_rn(ax1, ay2)));
    acc = __fadd_rn(acc, __fmul_rn(t21, __fmul_rn(ax2, ay1)));
    acc = __fadd_rn(acc, __fmul_rn(t22, __fmul_rn(ax1, ay1)));
    const float r = rintf(acc);
    return (uint32_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

__global__ void __launch_bounds__(256)
flatten_remap_kernel(const uint8_t* __restrict__ src, int src_stride, int src_w, int src_h, int64_t src_image_bytes, const float2* __restrict__ maps,
                     const int* __restrict__ meta, int n_views, uint8_t* __restrict__ out, int64_t out_image_bytes) {
    const int v = blockIdx.y, b = blockIdx.z;
    const int w = meta[4 * v], h = meta[4 * v + 1];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const float2 m = maps[meta[4 * v + 2] + i];
    out[(int64_t)b * out_image_bytes + meta[4 * v + 3] + i] = (uint8_t)remap_pixel<false>(src + (int64_t)b * src_image_bytes, src_stride, src_w, src_h, m);
}

// The same remap straight into a key-frame unit's input block (cam.hip): image b's views [first_view, first_view + gridDim.y), all of view_px pixels, land at
// out + (b * gridDim.y + d) * view_px.  A lane makes four consecutive pixels: 32 map bytes in (two 16-byte loads, 2 KiB contiguous per wave) and one dword
// out.  Pixels [0, remap_px) of a view are remapped by its first tiles_remap blocks, [remap_px, view_px) -- the rows the fisheye mask blanks before both
// networks -- are zeros from the blocks behind them, which read neither maps nor source; a block is one or the other.  The only per-view datum, the map
// offset, is one scalar load per block.  remap_px, view_px: multiples of 4; every view's map starts on 16 bytes (omni_flatten_create).
#define OMNI_FLATTEN_UNIT_TILE 1024     // pixels per block
__global__ void __launch_bounds__(256)
flatten_unit_kernel(const uint8_t* __restrict__ src, int src_stride, int src_w, int src_h, int64_t src_image_bytes, const float2* __restrict__ maps,
                    const int* __restrict__ meta, int first_view, int view_px, int remap_px, int tiles_remap, uint8_t* __restrict__ out) {
    const int d = blockIdx.y, b = blockIdx.z, tile = blockIdx.x;
    uint32_t* o = reinterpret_cast<uint32_t*>(out + ((int64_t)b * gridDim.y + d) * view_px);
    if (tile >= tiles_remap) {
        const int p = remap_px + (tile - tiles_remap) * OMNI_FLATTEN_UNIT_TILE + 4 * threadIdx.x;
        if (p < view_px) o[p >> 2] = 0u;
        return;
    }
    const int p = tile * OMNI_FLATTEN_UNIT_TILE + 4 * threadIdx.x;
    if (p >= remap_px) return;
    const float4* mp = reinterpret_cast<const float4*>(maps + meta[4 * (first_view + d) + 2] + p);
    const float4 m01 = mp[0], m23 = mp[1];
    const uint8_t* s = src + (int64_t)b * src_image_bytes;
    auto px = [&](float x, float y) { return remap_pixel<true>(s, src_stride, src_w, src_h, make_float2(x, y)); };
    o[p >> 2] = px(m01.x, m01.y) | px(m01.z, m01.w) << 8 | px(m23.x, m23.y) << 16 | px(m23.z, m23.w) << 24;
}

int flatten_unit_launch(const omni_flatten* f, hipStream_t stream, const uint8_t* src_dev, int src_stride, int n_images, int first_view, int dirs, int width,
                        int height, int fisheye_mask, uint8_t* out_dev) {
    int row0 = 0, row1 = 0;
    omni_fisheye_mask_rows(height, fisheye_mask, &row0, &row1);
    // (the networks take multiples of 8 only: the masked rows then run to the end of the view and every row holds whole quads)
    OMNI_REQUIRE(width % 4 == 0 && row1 == height && ((uintptr_t)out_dev & 3) == 0 && f->src_w >= 2, OMNI_ERR_INVALID, "flatten_unit_launch: %dx%d views at %p, frames %d wide",
                 width, height, (void*)out_dev, f->src_w);
    omni::TraceRange trace_range("flatten");
    const int view_px = width * height, remap_px = width * row0, tiles_remap = cdiv(remap_px, OMNI_FLATTEN_UNIT_TILE);
    hipLaunchKernelGGL(flatten_unit_kernel, dim3(tiles_remap + cdiv(view_px - remap_px, OMNI_FLATTEN_UNIT_TILE), dirs, n_images), dim3(256), 0, stream, src_dev, src_stride,
                       f->src_w, f->src_h, (int64_t)src_stride * f->src_h, reinterpret_cast<const float2*>(f->maps), f->meta, first_view, view_px, remap_px, tiles_remap,
                       out_dev);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

}  // namespace omni

extern "C" {

omni_flatten* omni_flatten_create(omni_ctx* ctx, int src_width, int src_height, int n_views, const int* view_w, const int* view_h, const float* const* map_xy) {
    if (!ctx || !view_w || !view_h || !map_xy || n_views < 1 || n_views > 16 || src_width < 1 || src_height < 1) { omni::set_error("bad argument"); return nullptr; }
    (void)hipSetDevice(ctx->device);
    omni_flatten* f = new omni_flatten();
    f->ctx = ctx; f->src_w = src_width; f->src_h = src_height; f->n_views = n_views;
    std::vector<int> meta(4 * n_views);
    int64_t map_px = 0;
    for (int v = 0; v < n_views; ++v) {
        if (view_w[v] < 1 || view_h[v] < 1 || !map_xy[v]) { omni::set_error("bad view %d", v); delete f; return nullptr; }
        f->vw.push_back(view_w[v]); f->vh.push_back(view_h[v]); f->out_off.push_back(f->out_bytes);
        meta[4 * v] = view_w[v]; meta[4 * v + 1] = view_h[v]; meta[4 * v + 2] = (int)map_px; meta[4 * v + 3] = (int)f->out_bytes;
        map_px += ((int64_t)view_w[v] * view_h[v] + 1) & ~(int64_t)1;      // every view's map on a 16-byte boundary (flatten_unit_kernel loads float4)
        f->out_bytes += (int64_t)view_w[v] * view_h[v];
    }
    bool ok = hipMalloc((void**)&f->maps, (size_t)map_px * 8) == hipSuccess && hipMalloc((void**)&f->meta, meta.size() * 4) == hipSuccess;
    for (int v = 0; ok && v < n_views; ++v)
        ok = hipMemcpyAsync(f->maps + 2 * (int64_t)meta[4 * v + 2], map_xy[v], (size_t)view_w[v] * view_h[v] * 8, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(f->meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) { omni::set_error("omni_flatten_create: device allocation / upload failed"); omni_flatten_destroy(f); return nullptr; }
    return f;
}

void omni_flatten_destroy(omni_flatten* f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    if (f->maps) (void)hipFree(f->maps);
    if (f->meta) (void)hipFree(f->meta);
    delete f;
}

int64_t omni_flatten_out_bytes(const omni_flatten* f) { return f ? f->out_bytes : -1; }

int omni_flatten_enqueue_dev(omni_flatten* f, const uint8_t* src_dev, int src_stride, int batch, uint8_t* out_dev) {
    OMNI_REQUIRE(f && src_dev && out_dev && batch >= 1 && src_stride >= f->src_w, OMNI_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(f->mu);
    (void)hipSetDevice(f->ctx->device);
    int max_px = 0;
    for (int v = 0; v < f->n_views; ++v) max_px = std::max(max_px, f->vw[v] * f->vh[v]);
    hipLaunchKernelGGL(omni::flatten_remap_kernel, dim3(omni::cdiv(max_px, 256), f->n_views, batch), dim3(256), 0, f->ctx->stream, src_dev, src_stride,
                       f->src_w, f->src_h, (int64_t)src_stride * f->src_h, reinterpret_cast<const float2*>(f->maps), f->meta, f->n_views, out_dev, f->out_bytes);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

}  // extern "C"
