// The consistency rows of pairwise consistency maximisation on the GPU (csrc/pcm_plan.h has the arithmetic, the verdict and the clique rule -- this file only spreads
// the pairs over lanes).  A handle owns one graph in HBM: the edges as structure-of-arrays F [29][capacity] f64 + D [2][capacity] i32, the bit matrix M
// [capacity][capacity / 64] u64, and one block that travels back: deg [capacity] i32 | new rows [64][capacity / 64] u64.  omni_pcm_add is four launches on the
// context's stream between one upload and one download:
//   pcm_append_kernel   the n uploaded records -> columns held .. held + n - 1 of F and D; deg of the new vertices = 0
//   pcm_pairs_kernel    grid (row words / 4, n), 256 lanes: wave w of new edge i owns word w of row i, lane l the pair (i, j = 64 w + l), j < i -- earlier edges of
//                       the same call included.  The wave's 64 verdicts become the word through a ballot, written by lane 0 with an ordinary 64-bit vector store;
//                       the same word goes to L [64][capacity / 64], the call's lower triangle; lane 0 also adds the word's popcount to deg[i] (an integer
//                       atomicAdd: the sum does not depend on the order)
//   pcm_mirror_kernel   one lane per vertex j < held + n: the bits (i, j) of the new rows i > j, read from L, become bits (j, held ..) of row j of M -- at most two
//                       words, owned by this lane alone, a plain read-modify-write -- and are added to deg[j]
//   pcm_gather_kernel   the new rows, contiguous in M, -> the block behind deg
// No workgroup waits for another or reads what another of the same launch wrote; every loop's trip count is n (<= 64), a launch argument; no LDS, no scratch.  Every
// index is below capacity by the checks of omni_pcm_add (held + n <= capacity) and the guards in the kernels.  Built with contraction off (Makefile; the header's
// pragma says the same).
#include "common.h"
#include "pcm_plan.h"

struct omni_pcm {
    omni_ctx* ctx = nullptr;
    int cap = 0, words = 0, size = 0;
    omni_pcm_params params{};
    omni::DevMem mem;
    double* F = nullptr;
    int* D = nullptr;
    uint64_t* M = nullptr;
    char* out = nullptr;                   // deg [cap] i32 | rows [64][words] u64
    uint64_t* L = nullptr;                 // [64][words]: the lower triangle of the rows of the call in flight, as pcm_pairs_kernel left it
    omni_pcm_edge* stage = nullptr;        // [64]
    omni::HostBuf hstage;
    std::mutex mu;
};

namespace omni {

__global__ __launch_bounds__(64) void pcm_append_kernel(const omni_pcm_edge* __restrict__ stage, double* __restrict__ F, int* __restrict__ D, int* __restrict__ deg, int cap,
                                                        int held, int n) {
    const int k = threadIdx.x;
    if (k >= n || held + k >= cap) return;
    pcm::store_soa(F, D, cap, held + k, stage[k]);
    deg[held + k] = 0;
}

__global__ __launch_bounds__(pcm::THREADS) void pcm_pairs_kernel(const double* __restrict__ F, const int* __restrict__ D, uint64_t* __restrict__ M, uint64_t* __restrict__ L,
                                                                 int* __restrict__ deg, int cap, int words, int held, int n, int words_used, const omni_pcm_params pr) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = held + (int)blockIdx.y, w = (int)blockIdx.x * (pcm::THREADS / 64) + wave;
    if ((int)blockIdx.y >= n || i >= cap || w >= words_used || w >= words) return;          // (uniform over the wave)
    const int j = w * 64 + lane;
    bool ok = false;
    if (j < i) {
        double smd = 0;
        const int orient = pcm::pair_smd(pcm::load_soa(F, D, cap, i), pcm::load_soa(F, D, cap, j), pr.pos_covariance_per_meter, pr.yaw_covariance_per_meter, &smd);
        ok = pcm::consistent(orient, smd, pr.pcm_thres);
    }
    const unsigned long long word = __ballot(ok);
    if (lane == 0) {
        M[(size_t)i * words + w] = word;
        L[(size_t)blockIdx.y * words + w] = word;
        if (word) atomicAdd(&deg[i], __popcll(word));
    }
}

__global__ __launch_bounds__(256) void pcm_mirror_kernel(uint64_t* __restrict__ M, const uint64_t* __restrict__ L, int* __restrict__ deg, int cap, int words, int held, int n) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= held + n || j >= cap) return;
    unsigned long long bits = 0;
    for (int k = 0; k < n; ++k) {
        const int i = held + k;
        if (i > j && i < cap) bits |= ((L[(size_t)k * words + (j >> 6)] >> (j & 63)) & 1ull) << k;
    }
    if (!bits) return;
    const int w0 = held >> 6, s = held & 63;
    M[(size_t)j * words + w0] |= bits << s;
    if (s && w0 + 1 < words && (bits >> (64 - s))) M[(size_t)j * words + w0 + 1] |= bits >> (64 - s);
    deg[j] += __popcll(bits);
}

__global__ __launch_bounds__(256) void pcm_gather_kernel(const uint64_t* __restrict__ M, uint64_t* __restrict__ rows_out, int cap, int words, int held, int n) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)n * words || held + n > cap) return;
    rows_out[k] = M[(size_t)held * words + k];
}

}  // namespace omni

extern "C" int omni_pcm_create(omni_ctx* ctx, int capacity, const omni_pcm_params* params, omni_pcm** out) {
    using namespace omni;
    OMNI_REQUIRE(ctx && params && out, OMNI_ERR_INVALID, "omni_pcm_create: null argument");
    const char* why = pcm::capacity_refusal(capacity);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "omni_pcm_create: %s (%d)", why, capacity);
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    omni_pcm* p = new omni_pcm;
    p->ctx = ctx; p->cap = capacity; p->words = capacity / 64; p->params = *params;
    const size_t cap = (size_t)capacity, words = cap / 64, out_bytes = cap * 4 + (size_t)OMNI_PCM_MAX_ADD * words * 8;
    int rc = p->mem.alloc(&p->F, (size_t)pcm::kFields * cap * 8, ctx->stream, true);
    if (!rc) rc = p->mem.alloc(&p->D, 2 * cap * 4, ctx->stream, true);
    if (!rc) rc = p->mem.alloc(&p->M, cap * words * 8, ctx->stream, true);
    if (!rc) rc = p->mem.alloc(&p->out, out_bytes, ctx->stream, true);
    if (!rc) rc = p->mem.alloc(&p->L, (size_t)OMNI_PCM_MAX_ADD * words * 8, ctx->stream, true);
    if (!rc) rc = p->mem.alloc(&p->stage, (size_t)OMNI_PCM_MAX_ADD * sizeof(omni_pcm_edge), ctx->stream, true);
    if (!rc) rc = p->hstage.ensure(out_bytes > (size_t)OMNI_PCM_MAX_ADD * sizeof(omni_pcm_edge) ? out_bytes : (size_t)OMNI_PCM_MAX_ADD * sizeof(omni_pcm_edge));
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("omni_pcm_create: hipStreamSynchronize failed"); rc = OMNI_ERR_HIP; }
    if (rc) { p->mem.release_all(); p->hstage.release(); delete p; return rc; }
    *out = p;
    return OMNI_OK;
}

extern "C" void omni_pcm_destroy(omni_pcm* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    p->mem.release_all();
    p->hstage.release();
    delete p;
}

extern "C" int omni_pcm_size(const omni_pcm* p) { return p ? p->size : 0; }
extern "C" int omni_pcm_capacity(const omni_pcm* p) { return p ? p->cap : 0; }

extern "C" int omni_pcm_add(omni_pcm* p, const omni_pcm_edge* edges, int n, int32_t* degrees_out, uint64_t* rows_out, float* kernel_us) {
    using namespace omni;
    OMNI_REQUIRE(p && edges && degrees_out && rows_out, OMNI_ERR_INVALID, "omni_pcm_add: null argument");
    OMNI_REQUIRE(n >= 1 && n <= OMNI_PCM_MAX_ADD, OMNI_ERR_INVALID, "omni_pcm_add: n %d outside 1..%d", n, OMNI_PCM_MAX_ADD);
    TraceRange trace_range("pcm rows");
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->size + n > p->cap) return OMNI_PCM_FULL;
    omni_ctx* ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    const int held = p->size, cap = p->cap, words = p->words, words_used = cdiv(held + n, 64);
    int* deg = (int*)p->out;
    uint64_t* rows_dev = (uint64_t*)(p->out + (size_t)cap * 4);
    char* h = p->hstage.as<char>();
    memcpy(h, edges, (size_t)n * sizeof(omni_pcm_edge));
    OMNI_HIP_TRY(hipMemcpyAsync(p->stage, h, (size_t)n * sizeof(omni_pcm_edge), hipMemcpyHostToDevice, ctx->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (kernel_us) { OMNI_HIP_TRY(hipEventCreate(&e0)); OMNI_HIP_TRY(hipEventCreate(&e1)); OMNI_HIP_TRY(hipEventRecord(e0, ctx->stream)); }
    hipLaunchKernelGGL(pcm_append_kernel, dim3(1), dim3(64), 0, ctx->stream, p->stage, p->F, p->D, deg, cap, held, n);
    hipLaunchKernelGGL(pcm_pairs_kernel, dim3((unsigned)cdiv(words_used, pcm::THREADS / 64), (unsigned)n), dim3(pcm::THREADS), 0, ctx->stream, p->F, p->D, p->M, p->L, deg, cap, words,
                       held, n, words_used, p->params);
    hipLaunchKernelGGL(pcm_mirror_kernel, dim3((unsigned)cdiv(held + n, 256)), dim3(256), 0, ctx->stream, p->M, p->L, deg, cap, words, held, n);
    hipLaunchKernelGGL(pcm_gather_kernel, dim3((unsigned)cdiv64((int64_t)n * words, 256)), dim3(256), 0, ctx->stream, p->M, rows_dev, cap, words, held, n);
    hipError_t err = hipGetLastError();
    if (kernel_us && err == hipSuccess) (void)hipEventRecord(e1, ctx->stream);
    const size_t down = (size_t)cap * 4 + (size_t)n * words * 8;
    if (err == hipSuccess) err = hipMemcpyAsync(h, p->out, down, hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (kernel_us) {
        float ms = 0;
        if (err == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *kernel_us = ms * 1000.f;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    // the records are in F and the rows in M whether or not the download arrived: a failed call leaves the handle unusable, like every HIP failure of this library
    OMNI_HIP_TRY(err);
    p->size = held + n;
    memcpy(degrees_out, h, (size_t)(held + n) * 4);
    memcpy(rows_out, h + (size_t)cap * 4, (size_t)n * words * 8);
    return OMNI_OK;
}

extern "C" int omni_pcm_adjacency(omni_pcm* p, int first, int n_rows, uint64_t* rows_out, int32_t* degrees_out) {
    using namespace omni;
    OMNI_REQUIRE(p, OMNI_ERR_INVALID, "omni_pcm_adjacency: null handle");
    OMNI_REQUIRE(first >= 0 && n_rows >= 0 && first + n_rows <= p->cap, OMNI_ERR_INVALID, "omni_pcm_adjacency: rows %d + %d of %d", first, n_rows, p->cap);
    std::lock_guard<std::mutex> lk(p->mu);
    (void)hipSetDevice(p->ctx->device);
    if (rows_out && n_rows) OMNI_HIP_TRY(hipMemcpyAsync(rows_out, p->M + (size_t)first * p->words, (size_t)n_rows * p->words * 8, hipMemcpyDeviceToHost, p->ctx->stream));
    if (degrees_out && p->size) OMNI_HIP_TRY(hipMemcpyAsync(degrees_out, p->out, (size_t)p->size * 4, hipMemcpyDeviceToHost, p->ctx->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return OMNI_OK;
}
