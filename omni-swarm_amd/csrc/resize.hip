// omni_resize_*: camera-size frames -> network-size images on the GPU: the cv::resize(input, _input, cv::Size(width, height)) both of the reference's engines run
// on the host in front of their networks (superpoint_tensorrt.cpp:123-125, mobilenetvlad_tensorrt.cpp:6-8; INTER_LINEAR on CV_8UC1).  The arithmetic is the fixed
// spec of resize_plan.h -- OpenCV 3.4's own integer path restated; OpenCV is un-vendored: PARITY UNPINNED -- and the four tables it reads are made there, on the
// host, once per object, and live in HBM.  All integer: no rounding-mode or contraction concern.
// One kernel, no intermediate image: a lane makes four consecutive destination pixels of one row (horizontal pass of its two source rows in registers, then the
// vertical pass) and stores one dword.  Per lane: 16 + 16 table bytes for its columns (two 16-byte loads, contiguous over the wave), 4 + 4 for its row, and
// 8 gathers: a row's two taps are neighbouring bytes and come in as ONE (unaligned) 16-bit load, as in flatten.hip's remap_pixel<true>; the gather instructions
// bound the kernel (docs/kernels.md).  The copy and area-2x modes of the plan are the same kernel with the gathers replaced by one 4- / two 8-byte loads.
// Destination widths are multiples of 4 (the networks take multiples of 8): every lane owns a whole dword, there is no tail.
#include "common.h"
#include "resize_plan.h"

namespace omni {

template <int MODE>
__global__ void __launch_bounds__(256)
resize_kernel(const uint8_t* __restrict__ src, int src_stride, int src_w, int src_h, int64_t src_image_bytes, const int32_t* __restrict__ xofs,
              const int16_t* __restrict__ ialpha, const int32_t* __restrict__ yofs, const int16_t* __restrict__ ibeta, int quads_per_row, int dst_h,
              uint8_t* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads_per_row * dst_h) return;
    const int y = q / quads_per_row, x = (q - y * quads_per_row) * 4;
    const uint8_t* s = src + (int64_t)blockIdx.y * src_image_bytes;
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (int64_t)blockIdx.y * quads_per_row * 4 * dst_h) + q;
    if constexpr (MODE == RESIZE_COPY) {
        uint32_t v;
        __builtin_memcpy(&v, s + (int64_t)y * src_stride + x, 4);
        *o = v;
    } else if constexpr (MODE == RESIZE_AREA2) {
        uint2 r0, r1;                                                     // source bytes [2x, 2x + 8) of rows 2y and 2y + 1
        __builtin_memcpy(&r0, s + (int64_t)(2 * y) * src_stride + 2 * x, 8);
        __builtin_memcpy(&r1, s + (int64_t)(2 * y + 1) * src_stride + 2 * x, 8);
        auto pair = [](uint32_t a, uint32_t b, int sh) { return ((a >> sh) & 255u) + ((a >> (sh + 8)) & 255u) + ((b >> sh) & 255u) + ((b >> (sh + 8)) & 255u) + 2u; };
        *o = pair(r0.x, r1.x, 0) >> 2 | (pair(r0.x, r1.x, 16) >> 2) << 8 | (pair(r0.y, r1.y, 0) >> 2) << 16 | (pair(r0.y, r1.y, 16) >> 2) << 24;
    } else {
        const int sy = yofs[y];
        const uint8_t* row0 = s + (int64_t)min(max(sy, 0), src_h - 1) * src_stride;
        const uint8_t* row1 = s + (int64_t)min(max(sy + 1, 0), src_h - 1) * src_stride;
        const int beta = *reinterpret_cast<const int*>(ibeta + 2 * y);     // (coefficients are 0..2048: the halves unpack without sign care)
        const int b0 = beta & 0xffff, b1 = beta >> 16;
        const int4 xo = *reinterpret_cast<const int4*>(xofs + x);
        const int4 al = *reinterpret_cast<const int4*>(ialpha + 2 * x);
        auto px = [&](int sx, int alpha) -> uint32_t {
            const int a0 = alpha & 0xffff, a1 = alpha >> 16;
            const int xc = min(sx, src_w - 2);                             // the 16-bit load stays inside the row (src_w >= 2); sx == src_w - 1: its tap is the high byte
            uint16_t v0, v1;
            __builtin_memcpy(&v0, row0 + xc, 2);
            __builtin_memcpy(&v1, row1 + xc, 2);
            const int h0 = v0 >> 8, h1 = v1 >> 8;                          // byte min(sx + 1, src_w - 1), the second tap
            const int t0 = sx == xc ? (v0 & 255) : h0, t1 = sx == xc ? (v1 & 255) : h1;
            const int R0 = t0 * a0 + h0 * a1, R1 = t1 * a0 + h1 * a1;
            return (uint32_t)((((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2);
        };
        *o = px(xo.x, al.x) | px(xo.y, al.y) << 8 | px(xo.z, al.z) << 16 | px(xo.w, al.w) << 24;
    }
}

int resize_unit_launch(const omni_resize* r, hipStream_t stream, const uint8_t* src_dev, int src_stride, int n_images, uint8_t* out_dev) {
    OMNI_REQUIRE(r && src_dev && out_dev && n_images >= 1 && n_images <= 65535 && src_stride >= r->src_w && ((uintptr_t)out_dev & 3) == 0, OMNI_ERR_INVALID,
                 "resize: %d frames, stride %d for frames %d wide, output at %p", n_images, src_stride, r ? r->src_w : 0, (void*)out_dev);
    omni::TraceRange trace_range("resize");
    const int qpr = r->dst_w / 4;
    const dim3 grid(cdiv(qpr * r->dst_h, 256), n_images), block(256);
    const int64_t image_bytes = (int64_t)src_stride * r->src_h;
#define OMNI_RESIZE_LAUNCH(MODE)                                                                                                                                  \
    hipLaunchKernelGGL(resize_kernel<MODE>, grid, block, 0, stream, src_dev, src_stride, r->src_w, r->src_h, image_bytes, r->xofs, r->ialpha, r->yofs, r->ibeta, qpr, \
                       r->dst_h, out_dev)
    if (r->mode == RESIZE_COPY) OMNI_RESIZE_LAUNCH(RESIZE_COPY);
    else if (r->mode == RESIZE_AREA2) OMNI_RESIZE_LAUNCH(RESIZE_AREA2);
    else OMNI_RESIZE_LAUNCH(RESIZE_LINEAR);
#undef OMNI_RESIZE_LAUNCH
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

}  // namespace omni

extern "C" {

omni_resize* omni_resize_create(omni_ctx* ctx, int src_width, int src_height, int dst_width, int dst_height) {
    if (!ctx) { omni::set_error("null context"); return nullptr; }
    // (two taps per row come in as one 16-bit load: a source row holds at least two bytes; a lane stores one dword: destination widths in fours)
    if (src_width < 2 || src_height < 1 || dst_width < 4 || dst_height < 1 || dst_width % 4 != 0 || src_width > 32768 || src_height > 32768 || dst_width > 32768 ||
        dst_height > 32768) {
        omni::set_error("omni_resize_create: %dx%d -> %dx%d (source at least 2 wide, destination width a multiple of 4, every side <= 32768)", src_width, src_height,
                        dst_width, dst_height);
        return nullptr;
    }
    (void)hipSetDevice(ctx->device);
    const omni::ResizePlan p = omni::resize_plan(src_width, src_height, dst_width, dst_height);
    omni_resize* r = new omni_resize();
    r->ctx = ctx; r->mode = p.mode; r->src_w = src_width; r->src_h = src_height; r->dst_w = dst_width; r->dst_h = dst_height;
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_xofs = 0, o_ialpha = al(o_xofs + p.xofs.size() * 4), o_yofs = al(o_ialpha + p.ialpha.size() * 2), o_ibeta = al(o_yofs + p.yofs.size() * 4),
                 bytes = al(o_ibeta + p.ibeta.size() * 2);
    std::vector<uint8_t> host(bytes, 0);
    memcpy(host.data() + o_xofs, p.xofs.data(), p.xofs.size() * 4);
    memcpy(host.data() + o_ialpha, p.ialpha.data(), p.ialpha.size() * 2);
    memcpy(host.data() + o_yofs, p.yofs.data(), p.yofs.size() * 4);
    memcpy(host.data() + o_ibeta, p.ibeta.data(), p.ibeta.size() * 2);
    const bool ok = hipMalloc((void**)&r->tables, bytes) == hipSuccess &&
                    hipMemcpyAsync(r->tables, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) { omni::set_error("omni_resize_create: device allocation / upload failed"); omni_resize_destroy(r); return nullptr; }
    r->xofs = reinterpret_cast<const int32_t*>(r->tables + o_xofs); r->ialpha = reinterpret_cast<const int16_t*>(r->tables + o_ialpha);
    r->yofs = reinterpret_cast<const int32_t*>(r->tables + o_yofs); r->ibeta = reinterpret_cast<const int16_t*>(r->tables + o_ibeta);
    return r;
}

void omni_resize_destroy(omni_resize* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    if (r->tables) (void)hipFree(r->tables);
    delete r;
}

int omni_resize_mode(const omni_resize* r) { return r ? r->mode : -1; }

int omni_resize_enqueue_dev(omni_resize* r, const uint8_t* src_dev, int src_stride, int batch, uint8_t* out_dev) {
    OMNI_REQUIRE(r && src_dev && out_dev, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(r->mu);
    (void)hipSetDevice(r->ctx->device);
    return omni::resize_unit_launch(r, r->ctx->stream, src_dev, src_stride, batch, out_dev);
}

}  // extern "C"
