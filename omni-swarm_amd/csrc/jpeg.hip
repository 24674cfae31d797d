// omni_jpeg_*: the main images of a key-frame unit as baseline JPEG files (send_img: encode_image, swarm_loop/src/loop_cam.cpp:56-71) on the GPU.  The arithmetic
// and the file layout are jpeg_plan.h's -- this file only spreads them over lanes and puts the variable-length pieces together:
//   length   one 8 x 8 block per lane: load (stride, edge replication, zero_from_row), DCT, quantise, and COUNT the bits of the block's code.  The DC predictor is the
//            previous block's quantised DC, recomputed from that block's pixel sum (the islow DC is exactly the sum of the 64 centred samples);
//   scan     one workgroup per image: the exclusive scan of the bit lengths = every block's bit offset, and the image's total;
//   emit     the length pass again, this time writing: each lane shifts its block's code to its bit offset and ORs it, 32 bits at a time, into the image's zeroed word
//            buffer (MSB first).  Neighbouring blocks share boundary words: ordinary vector atomics (atomicOr).  Recomputing the block costs a few hundred
//            integer operations; keeping its code between the passes would cost a 208-byte slot per block (63 x 26 + 20 bits) written and read through HBM;
//   stuff    one workgroup per image: header, then the scan bytes with a 0x00 behind every 0xFF (count, scan, scatter, 4 bytes per lane and step), the last byte padded
//            with 1-bits, EOI, size and status.  Every store is checked against the capacity.
// Everything runs on the caller's stream; nothing synchronises with the host.  All scratch is owned by the handle.
#include "common.h"
#include "jpeg_plan.h"

struct omni_jpeg {
    omni_ctx* ctx = nullptr;
    int w = 0, h = 0, max_images = 0, quality = 0, bw = 0, nblocks = 0;
    int64_t capacity = 0;
    size_t cap_words = 0;                  // per image: the words that can hold scan bytes of a file that fits (a longer scan is TRUNCATED whatever it holds)
    omni::DevMem mem;
    omni::jp::Tables* d_tables = nullptr;
    uint8_t* d_header = nullptr;           // JP_HEADER_BYTES
    uint32_t* d_off = nullptr;             // [max_images][nblocks]: bit lengths, then (in place) bit offsets
    uint32_t* d_total = nullptr;           // [max_images] bits of the scan
    uint32_t* d_words = nullptr;           // [max_images][cap_words]
    std::mutex mu;
};

namespace omni {

#define JP_THREADS 256
#define JP_SCAN_THREADS 1024

__device__ __forceinline__ void jp_load_tables(jp::Tables* dst, const jp::Tables* __restrict__ src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(jp::Tables) / 4); i += blockDim.x) d[i] = s[i];
    __syncthreads();
}

// a block's code ORed into the image's word buffer at its bit offset; words at or beyond `limit` are dropped (they belong to a file that does not fit)
struct WordSink {
    uint32_t* words;
    uint32_t wi, limit;
    uint64_t acc = 0;
    int nacc;
    __device__ WordSink(uint32_t* w, uint32_t bit_off, uint32_t lim) : words(w), wi(bit_off >> 5), limit(lim), nacc((int)(bit_off & 31)) {}
    __device__ void word(uint32_t v) {
        if (v != 0 && wi < limit) atomicOr(words + wi, v);
        ++wi;
    }
    __device__ void put(uint32_t bits, int n) {               // n <= 27, nacc <= 31 on entry: at most 58 bits held
        acc = acc << n | bits;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            word((uint32_t)(acc >> nacc));
            acc &= (1ull << nacc) - 1ull;
        }
    }
    __device__ void flush() {
        if (nacc > 0) word((uint32_t)(acc << (32 - nacc)));
    }
};

template <bool kEmit>
__global__ __launch_bounds__(JP_THREADS) void jpeg_block_kernel(const uint8_t* __restrict__ gray, int stride, int w, int h, int zero_from_row, int bw, int nblocks,
                                                                const jp::Tables* __restrict__ tables, uint32_t* __restrict__ off, uint32_t* __restrict__ words,
                                                                uint32_t cap_words) {
    __shared__ jp::Tables T;
    jp_load_tables(&T, tables);
    const int b = blockIdx.x * JP_THREADS + threadIdx.x, img = blockIdx.y;
    if (b >= nblocks) return;
    const uint8_t* g = gray + (size_t)img * stride * h;
    uint32_t* o = off + (size_t)img * nblocks + b;
    if (kEmit) {
        WordSink sink(words + (size_t)img * cap_words, *o, cap_words);
        jp::encode_block(g, stride, w, h, zero_from_row, bw, b, T.qv, T.dc, T.ac, sink);
        sink.flush();
    } else {
        jp::BitCount sink;
        jp::encode_block(g, stride, w, h, zero_from_row, bw, b, T.qv, T.dc, T.ac, sink);
        *o = sink.bits;
    }
}

// exclusive scan of one value per lane over a workgroup of JP_SCAN_THREADS; *total = the sum.  lds: JP_SCAN_THREADS / 64 + 1 words, free again on return
__device__ __forceinline__ uint32_t jp_wg_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = JP_SCAN_THREADS / 64;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < nw; ++i) { const uint32_t t = lds[i]; lds[i] = run; run += t; }
        lds[nw] = run;
    }
    __syncthreads();
    const uint32_t r = lds[wave] + incl - v;
    *total = lds[nw];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(JP_SCAN_THREADS) void jpeg_scan_kernel(uint32_t* __restrict__ off, int nblocks, uint32_t* __restrict__ total) {
    __shared__ uint32_t lds[JP_SCAN_THREADS / 64 + 1];
    uint32_t* o = off + (size_t)blockIdx.x * nblocks;
    uint32_t carry = 0;
    for (int base = 0; base < nblocks; base += JP_SCAN_THREADS) {     // (uniform trip count: every lane reaches the barriers)
        const int i = base + threadIdx.x;
        uint32_t sum;
        const uint32_t excl = jp_wg_scan(i < nblocks ? o[i] : 0u, lds, &sum);
        if (i < nblocks) o[i] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

__global__ __launch_bounds__(JP_SCAN_THREADS) void jpeg_stuff_kernel(const uint32_t* __restrict__ words, uint32_t cap_words, const uint32_t* __restrict__ total,
                                                                     const uint8_t* __restrict__ header, uint8_t* __restrict__ out, int64_t capacity,
                                                                     int* __restrict__ sizes, int* __restrict__ status) {
    __shared__ uint32_t lds[JP_SCAN_THREADS / 64 + 1];
    const int img = blockIdx.x;
    const uint32_t* wd = words + (size_t)img * cap_words;
    uint8_t* o = out + (size_t)img * capacity;
    for (int i = threadIdx.x; i < JP_HEADER_BYTES; i += JP_SCAN_THREADS) o[i] = header[i];      // (capacity >= header + 2: checked at creation)
    const uint32_t bits = total[img];
    const int64_t nbytes = ((int64_t)bits + 7) >> 3, room = capacity - JP_HEADER_BYTES - 2;     // room: what is left for the scan
    if (nbytes > room) {                                                                        // (uniform: the whole workgroup leaves)
        if (threadIdx.x == 0) { sizes[img] = 0; status[img] = OMNI_JPEG_TRUNCATED; }
        return;
    }
    const uint32_t pad = (bits & 7) ? (1u << (8 - (bits & 7))) - 1u : 0u;                       // 1-bits behind the last code bit
    const int64_t nwords = (nbytes + 3) >> 2;                                                   // <= cap_words
    int64_t carry = 0;                                                                          // stuffed bytes in front of this step
    for (int64_t base = 0; base < nwords; base += JP_SCAN_THREADS) {
        const int64_t wi = base + threadIdx.x;
        const uint32_t v = wi < nwords ? wd[wi] : 0u;
        uint8_t by[4];
        uint32_t cnt = 0;
        for (int k = 0; k < 4; ++k) {
            const int64_t j = wi * 4 + k;
            by[k] = (uint8_t)(v >> (24 - 8 * k));
            if (j == nbytes - 1) by[k] |= (uint8_t)pad;
            if (j < nbytes) cnt += by[k] == 0xff ? 2u : 1u;
        }
        uint32_t sum;
        int64_t p = JP_HEADER_BYTES + carry + jp_wg_scan(cnt, lds, &sum);
        for (int k = 0; k < 4; ++k) {
            if (wi * 4 + k >= nbytes) break;
            if (p < capacity) o[p] = by[k];
            ++p;
            if (by[k] == 0xff) {
                if (p < capacity) o[p] = 0;
                ++p;
            }
        }
        carry += sum;
    }
    if (threadIdx.x == 0) {
        const int64_t size = JP_HEADER_BYTES + carry + 2;
        if (size > capacity) {
            sizes[img] = 0; status[img] = OMNI_JPEG_TRUNCATED;
        } else {
            o[size - 2] = 0xff; o[size - 1] = 0xd9;
            sizes[img] = (int)size; status[img] = OMNI_JPEG_OK;
        }
    }
}

// jpeg.hip's stage on `stream` (cam.hip runs it on the unit's MobileNetVLAD stream); the caller holds j->mu and has checked the arguments
int jpeg_launch(omni_jpeg* j, hipStream_t stream, const uint8_t* gray_dev, int stride, int n_images, int zero_from_row, uint8_t* out_dev, int* sizes_dev,
                int* status_dev) {
    OMNI_HIP_TRY(hipMemsetAsync(j->d_words, 0, (size_t)n_images * j->cap_words * 4, stream));
    const dim3 grid(cdiv(j->nblocks, JP_THREADS), n_images);
    hipLaunchKernelGGL(jpeg_block_kernel<false>, grid, dim3(JP_THREADS), 0, stream, gray_dev, stride, j->w, j->h, zero_from_row, j->bw, j->nblocks, j->d_tables, j->d_off,
                       j->d_words, (uint32_t)j->cap_words);
    OMNI_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n_images), dim3(JP_SCAN_THREADS), 0, stream, j->d_off, j->nblocks, j->d_total);
    OMNI_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_block_kernel<true>, grid, dim3(JP_THREADS), 0, stream, gray_dev, stride, j->w, j->h, zero_from_row, j->bw, j->nblocks, j->d_tables, j->d_off,
                       j->d_words, (uint32_t)j->cap_words);
    OMNI_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(n_images), dim3(JP_SCAN_THREADS), 0, stream, j->d_words, (uint32_t)j->cap_words, j->d_total, j->d_header, out_dev,
                       j->capacity, sizes_dev, status_dev);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

int jpeg_check_enqueue(const omni_jpeg* j, int stride, int n_images, int zero_from_row) {
    OMNI_REQUIRE(n_images >= 1 && n_images <= j->max_images, OMNI_ERR_INVALID, "omni_jpeg: %d images, the handle holds 1..%d", n_images, j->max_images);
    OMNI_REQUIRE(stride >= j->w, OMNI_ERR_INVALID, "omni_jpeg: stride %d for images %d wide", stride, j->w);
    OMNI_REQUIRE(zero_from_row >= 0 && zero_from_row <= j->h, OMNI_ERR_INVALID, "omni_jpeg: zero_from_row %d outside [0, %d]", zero_from_row, j->h);
    return OMNI_OK;
}

}  // namespace omni

extern "C" omni_jpeg* omni_jpeg_create(omni_ctx* ctx, int width, int height, int max_images, int quality, int64_t capacity_per_image) {
    using namespace omni;
    if (!ctx) { set_error("null context"); return nullptr; }
    if (width < 1 || height < 1 || width > 65535 || height > 65535) { set_error("omni_jpeg_create: %dx%d outside 1..65535", width, height); return nullptr; }
    const int64_t nblocks = (int64_t)cdiv(width, 8) * cdiv(height, 8);
    if (nblocks > (1 << 21)) { set_error("omni_jpeg_create: %dx%d is more than 2^21 blocks (32-bit bit offsets)", width, height); return nullptr; }
    if (max_images < 1 || max_images > 65535) { set_error("omni_jpeg_create: max_images=%d outside [1, 65535]", max_images); return nullptr; }
    if (capacity_per_image < JP_HEADER_BYTES + 2 || capacity_per_image > 0x7fffffff) {
        set_error("omni_jpeg_create: a capacity of %lld bytes, the header and EOI alone take %d", (long long)capacity_per_image, JP_HEADER_BYTES + 2);
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    omni_jpeg* j = new omni_jpeg();
    j->ctx = ctx; j->w = width; j->h = height; j->max_images = max_images; j->quality = jp::clamp_quality(quality); j->capacity = capacity_per_image;
    j->bw = cdiv(width, 8); j->nblocks = (int)nblocks;
    j->cap_words = (size_t)((capacity_per_image - JP_HEADER_BYTES - 2 + 3) / 4 + 1);
    jp::Tables T;
    jp::build_tables(j->quality, &T);
    uint8_t header[JP_HEADER_BYTES];
    auto make = [&]() -> int {
        OMNI_REQUIRE(jp::jpeg_header(width, height, j->quality, header) == JP_HEADER_BYTES, OMNI_ERR_INVALID, "omni_jpeg_create: header size");
        int rc;
        if ((rc = j->mem.alloc(&j->d_tables, sizeof(T))) || (rc = j->mem.alloc(&j->d_header, JP_HEADER_BYTES)) ||
            (rc = j->mem.alloc(&j->d_off, (size_t)max_images * j->nblocks * 4)) || (rc = j->mem.alloc(&j->d_total, (size_t)max_images * 4)) ||
            (rc = j->mem.alloc(&j->d_words, (size_t)max_images * j->cap_words * 4)))
            return rc;
        OMNI_HIP_TRY(hipMemcpy(j->d_tables, &T, sizeof(T), hipMemcpyHostToDevice));
        OMNI_HIP_TRY(hipMemcpy(j->d_header, header, JP_HEADER_BYTES, hipMemcpyHostToDevice));
        return OMNI_OK;
    };
    if (make() != OMNI_OK) { j->mem.release_all(); delete j; return nullptr; }
    return j;
}

extern "C" void omni_jpeg_destroy(omni_jpeg* j) {
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    (void)hipDeviceSynchronize();          // (the unit's MobileNetVLAD stream may still run the stage, cam.hip)
    j->mem.release_all();
    delete j;
}

extern "C" int omni_jpeg_enqueue_dev(omni_jpeg* j, const uint8_t* gray_dev, int stride, int n_images, int zero_from_row, uint8_t* out_dev, int* sizes_dev,
                                     int* status_dev) {
    OMNI_REQUIRE(j && gray_dev && out_dev && sizes_dev && status_dev, OMNI_ERR_INVALID, "null argument");
    int rc;
    if ((rc = omni::jpeg_check_enqueue(j, stride, n_images, zero_from_row))) return rc;
    omni::TraceRange trace_range("jpeg (main images)");
    std::lock_guard<std::mutex> lk(j->mu);
    std::lock_guard<std::mutex> lk2(j->ctx->mu);
    (void)hipSetDevice(j->ctx->device);
    return omni::jpeg_launch(j, j->ctx->stream, gray_dev, stride, n_images, zero_from_row, out_dev, sizes_dev, status_dev);
}
