// omni_pcafit_*: the moments of a PCA fit (csrc/pca_plan.h: count, sum and the upper triangle of the 256 x 256 second-moment matrix, f64) accumulated in HBM from
// the operands a SuperPoint pass leaves there -- raw_desc [B][max_num][256], norm_partial [B][8][256], n_kps [B] -- so that the descriptors of a key-frame stream
// never cross PCIe (the reference dumps them to a text file, loop_cam.cpp:577-582, and fits in a notebook).  Three kernels per pass, in stream order:
//   pca_keep_kernel     one workgroup per row slot: 0 = no such row, 1 = kept, 2 = skipped (a non-finite element)
//   pca_list_kernel     ONE workgroup: the kept rows' indices in stream order (a scan over the flags), n / skipped
//   pca_moments_kernel  36 workgroups = the 32 x 32 tiles of the upper triangle, and a 37th for the chain of s (thread = channel); every lane of a tile owns a 2 x 2 block of S in registers, starts from the entry's current
//                       value and walks the kept rows in order, 64 rows at a time staged through LDS as f64: one v_fma_f64 per entry per row, the chain of
//                       pca_plan.h.  Bit-equal to the g++ build of the header (omni_pca_moments_host), whatever the batch and however the stream was cut.
// No floating-point atomics, no workgroup waits for another, every loop is bounded by the launch's batch * max_num, no scratch.
#include "common.h"
#include "pca_plan.h"

struct omni_pcafit {
    omni_ctx* ctx = nullptr;
    uint8_t* acc = nullptr;            // one allocation: State | s [256] f64 | S [256][256] f64 (i <= j used)
    omni::DevBuf keep, rows;           // per pass: the row flags (u8) and the kept rows' indices (int), batch * max_num each
    omni_sp* owner = nullptr;          // the SuperPoint handle it is attached to (omni_sp_set_pcafit; same context, so the same stream): at most one
    std::mutex mu;
};

namespace omni {
namespace {

struct PcaState { int64_t n, skipped; int n_rows, pad; };
constexpr size_t kStateBytes = 64;
constexpr size_t kAccBytes = kStateBytes + (size_t)pca::kDim * 8 + (size_t)pca::kDim * pca::kDim * 8;
constexpr int kTile = 32, kTilesPerSide = pca::kDim / kTile, kTilePairs = kTilesPerSide * (kTilesPerSide + 1) / 2, kChunk = 64;

PcaState* state_of(const omni_pcafit* f) { return reinterpret_cast<PcaState*>(f->acc); }
double* s_of(const omni_pcafit* f) { return reinterpret_cast<double*>(f->acc + kStateBytes); }
double* S_of(const omni_pcafit* f) { return s_of(f) + pca::kDim; }

__global__ void __launch_bounds__(256)
pca_keep_kernel(const float* __restrict__ raw_desc, const float* __restrict__ norm_partial, const int* __restrict__ n_kps, int max_num, uint8_t* __restrict__ keep) {
    const int b = blockIdx.y, i = blockIdx.x, c = threadIdx.x;
    const int n = pca::clamp_count(n_kps[b], max_num);
    if (i >= n) { if (c == 0) keep[(int64_t)b * max_num + i] = 0; return; }
    const float x = pca::row_value(raw_desc, max_num, b, i, c, pca::chan_norm(norm_partial, b, c));
    const int bad = __syncthreads_or(pca::finite_f32(x) ? 0 : 1);
    if (c == 0) keep[(int64_t)b * max_num + i] = bad ? 2 : 1;
}

__global__ void __launch_bounds__(256)
pca_list_kernel(int total, const uint8_t* __restrict__ keep,
                int* __restrict__ rows, PcaState* __restrict__ st) {
    __shared__ int kept_of[256], skipped_of[256], first_of[256];
    const int t = threadIdx.x;
    const int per = (total + 255) / 256;
    const int r0 = t * per < total ? t * per : total, r1 = r0 + per < total ? r0 + per : total;
    int kept = 0, skipped = 0;
    for (int r = r0; r < r1; ++r) { const int k = keep[r]; kept += k == 1; skipped += k == 2; }
    kept_of[t] = kept; skipped_of[t] = skipped;
    __syncthreads();
    if (t == 0) {
        int run = 0, sk = 0;
        for (int u = 0; u < 256; ++u) { first_of[u] = run; run += kept_of[u]; sk += skipped_of[u]; }
        st->n += run; st->skipped += sk; st->n_rows = run;
    }
    __syncthreads();
    int at = first_of[t];
    for (int r = r0; r < r1; ++r) if (keep[r] == 1) rows[at++] = r;
}

// the chain of s, thread = channel: 32 rows' loads are issued together (one memory latency per 32 steps of the chain); the additions stay in row order
__device__ void pca_sum_rows(const float* __restrict__ raw_desc, const float* __restrict__ norm_partial, int max_num, int n_rows, const int* __restrict__ rows,
                             double* __restrict__ s) {
    constexpr int G = 32;
    const int t = threadIdx.x;
    double acc = s[t];
    int last_b = -1;
    float norm = 1.f;
    for (int k0 = 0; k0 < n_rows; k0 += G) {
        int row[G];
        float v[G];
#pragma unroll
        for (int u = 0; u < G; ++u) row[u] = k0 + u < n_rows ? rows[k0 + u] : -1;
#pragma unroll
        for (int u = 0; u < G; ++u) v[u] = row[u] >= 0 ? raw_desc[(int64_t)row[u] * pca::kDim + t] : 0.f;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            if (row[u] < 0) continue;
            const int b = row[u] / max_num;
            if (b != last_b) { norm = pca::chan_norm(norm_partial, b, t); last_b = b; }
            acc += pca::widened(v[u], norm);
        }
    }
    s[t] = acc;
}

__global__ void __launch_bounds__(256)
pca_moments_kernel(const float* __restrict__ raw_desc, const float* __restrict__ norm_partial, int max_num, int total, const int* __restrict__ rows,
                   const PcaState* __restrict__ st, double* __restrict__ s, double* __restrict__ S) {
    __shared__ __attribute__((aligned(16))) double sx[kChunk][2 * kTile];      // one chunk of kept rows: the tile's 32 row channels, then its 32 column channels
    if (blockIdx.x == kTilePairs) {                                            // the workgroup behind the tiles: s
        const int n = st->n_rows;
        pca_sum_rows(raw_desc, norm_partial, max_num, n > total ? total : n, rows, s);
        return;
    }
    int ti = 0, tj = 0;
    { int left = blockIdx.x; for (ti = 0; ti < kTilesPerSide; ++ti) { const int len = kTilesPerSide - ti; if (left < len) { tj = ti + left; break; } left -= len; } }
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = ti * kTile + 2 * ty, j0 = tj * kTile + 2 * tx;
    int n_rows = st->n_rows;
    if (n_rows > total) n_rows = total;
    const bool own00 = i0 <= j0, own01 = i0 <= j0 + 1, own10 = i0 + 1 <= j0, own11 = i0 + 1 <= j0 + 1;      // the upper triangle only
    double a00 = own00 ? S[(int64_t)i0 * pca::kDim + j0] : 0.0, a01 = own01 ? S[(int64_t)i0 * pca::kDim + j0 + 1] : 0.0;
    double a10 = own10 ? S[(int64_t)(i0 + 1) * pca::kDim + j0] : 0.0, a11 = own11 ? S[(int64_t)(i0 + 1) * pca::kDim + j0 + 1] : 0.0;
    const int cs = tid & 63, rg = tid >> 6;
    const int chan = cs < kTile ? ti * kTile + cs : tj * kTile + cs - kTile;
    int last_b = -1;
    float norm = 1.f;
    for (int base = 0; base < n_rows; base += kChunk) {
        const int cnt = n_rows - base < kChunk ? n_rows - base : kChunk;
        {   // this thread's 16 rows of the chunk: the loads are issued together, then divided
            int row[kChunk / 4];
            float v[kChunk / 4];
#pragma unroll
            for (int u = 0; u < kChunk / 4; ++u) row[u] = rg + 4 * u < cnt ? rows[base + rg + 4 * u] : -1;
#pragma unroll
            for (int u = 0; u < kChunk / 4; ++u) v[u] = row[u] >= 0 ? raw_desc[(int64_t)row[u] * pca::kDim + chan] : 0.f;
#pragma unroll
            for (int u = 0; u < kChunk / 4; ++u) {
                if (row[u] < 0) continue;
                const int b = row[u] / max_num;
                if (b != last_b) { norm = pca::chan_norm(norm_partial, b, chan); last_b = b; }
                sx[rg + 4 * u][cs] = pca::widened(v[u], norm);
            }
        }
        __syncthreads();
        if (cnt == kChunk) {
#pragma unroll 16
            for (int r = 0; r < kChunk; ++r) {
                const double xi0 = sx[r][2 * ty], xi1 = sx[r][2 * ty + 1], xj0 = sx[r][kTile + 2 * tx], xj1 = sx[r][kTile + 2 * tx + 1];
                a00 = pca::step(xi0, xj0, a00); a01 = pca::step(xi0, xj1, a01); a10 = pca::step(xi1, xj0, a10); a11 = pca::step(xi1, xj1, a11);
            }
        } else {
            for (int r = 0; r < cnt; ++r) {
                const double xi0 = sx[r][2 * ty], xi1 = sx[r][2 * ty + 1], xj0 = sx[r][kTile + 2 * tx], xj1 = sx[r][kTile + 2 * tx + 1];
                a00 = pca::step(xi0, xj0, a00); a01 = pca::step(xi0, xj1, a01); a10 = pca::step(xi1, xj0, a10); a11 = pca::step(xi1, xj1, a11);
            }
        }
        __syncthreads();
    }
    if (own00) S[(int64_t)i0 * pca::kDim + j0] = a00;
    if (own01) S[(int64_t)i0 * pca::kDim + j0 + 1] = a01;
    if (own10) S[(int64_t)(i0 + 1) * pca::kDim + j0] = a10;
    if (own11) S[(int64_t)(i0 + 1) * pca::kDim + j0 + 1] = a11;
}

int fit_sync(omni_pcafit* f) {
    OMNI_HIP_TRY(hipSetDevice(f->ctx->device));
    OMNI_HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return OMNI_OK;
}

}  // namespace

const omni_ctx* pcafit_ctx(const omni_pcafit* f) { return f->ctx; }

// omni_sp_set_pcafit's half on the fit: sp takes it (refused while another handle has it), or gives it back (sp_or_null == nullptr)
int pcafit_set_owner(omni_pcafit* f, omni_sp* sp_or_null) {
    std::lock_guard<std::mutex> lk(f->mu);
    OMNI_REQUIRE(!sp_or_null || !f->owner || f->owner == sp_or_null, OMNI_ERR_INVALID, "the fit is attached to another SuperPoint handle: one fit serves one handle at a time");
    f->owner = sp_or_null;
    return OMNI_OK;
}

// one pass's rows on the fit's own stream, which is `stream`: the stream of the handle it is attached to (the same context), or its context's
int pcafit_enqueue_on(omni_pcafit* f, hipStream_t stream, const float* raw_desc, const float* norm_partial, const int* n_kps, int batch, int max_num) {
    OMNI_REQUIRE(stream == f->ctx->stream, OMNI_ERR_INVALID, "a fit accumulates on its own context's stream only");
    OMNI_REQUIRE(batch >= 1 && batch <= 65535, OMNI_ERR_INVALID, "batch=%d outside [1,65535]", batch);
    OMNI_REQUIRE(max_num >= 1 && max_num <= 1024, OMNI_ERR_INVALID, "max_num=%d outside [1,1024]", max_num);
    std::lock_guard<std::mutex> lk(f->mu);
    const int total = batch * max_num;
    int rc;
    if ((rc = f->keep.ensure((size_t)total))) return rc;
    if ((rc = f->rows.ensure((size_t)total * sizeof(int)))) return rc;
    hipLaunchKernelGGL(pca_keep_kernel, dim3(max_num, batch), dim3(256), 0, stream, raw_desc, norm_partial, n_kps, max_num, f->keep.as<uint8_t>());
    OMNI_LAUNCH_CHECK();
    hipLaunchKernelGGL(pca_list_kernel, dim3(1), dim3(256), 0, stream, total, f->keep.as<uint8_t>(), f->rows.as<int>(), state_of(f));
    OMNI_LAUNCH_CHECK();
    hipLaunchKernelGGL(pca_moments_kernel, dim3(kTilePairs + 1), dim3(256), 0, stream, raw_desc, norm_partial, max_num, total, f->rows.as<int>(), state_of(f), s_of(f), S_of(f));
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

}  // namespace omni

extern "C" {

omni_pcafit* omni_pcafit_create(omni_ctx* ctx) {
    if (!ctx) { omni::set_error("null ctx"); return nullptr; }
    (void)hipSetDevice(ctx->device);
    omni_pcafit* f = new omni_pcafit();
    f->ctx = ctx;
    if (hipMalloc(&f->acc, omni::kAccBytes) != hipSuccess || hipMemsetAsync(f->acc, 0, omni::kAccBytes, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        omni::set_error("omni_pcafit_create: no device memory for the accumulator (%zu bytes)", omni::kAccBytes);
        (void)hipGetLastError();
        if (f->acc) (void)hipFree(f->acc);
        delete f;
        return nullptr;
    }
    return f;
}

void omni_pcafit_destroy(omni_pcafit* f) {
    if (!f) return;
    omni_sp* owner;
    { std::lock_guard<std::mutex> lk(f->mu); owner = f->owner; }
    if (owner) omni::sp_drop_pcafit(owner, f);            // the handle it is attached to lets go of it first: no pass reads a freed accumulator
    (void)omni::fit_sync(f);
    f->keep.release(); f->rows.release();
    if (f->acc) (void)hipFree(f->acc);
    delete f;
}

int omni_pcafit_reset(omni_pcafit* f) {
    OMNI_REQUIRE(f, OMNI_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(f->mu);
    int rc;
    if ((rc = omni::fit_sync(f))) return rc;
    OMNI_HIP_TRY(hipMemsetAsync(f->acc, 0, omni::kAccBytes, f->ctx->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(f->ctx->stream));
    return OMNI_OK;
}

int omni_pcafit_enqueue_rows_dev(omni_pcafit* f, const float* raw_desc_dev, const float* norm_partial_dev, const int* n_kps_dev, int batch, int max_num) {
    OMNI_REQUIRE(f && raw_desc_dev && norm_partial_dev && n_kps_dev, OMNI_ERR_INVALID, "null argument");
    OMNI_HIP_TRY(hipSetDevice(f->ctx->device));
    return omni::pcafit_enqueue_on(f, f->ctx->stream, raw_desc_dev, norm_partial_dev, n_kps_dev, batch, max_num);
}

int omni_pcafit_stats(omni_pcafit* f, int64_t* n, int64_t* skipped) {
    OMNI_REQUIRE(f, OMNI_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(f->mu);
    int rc;
    if ((rc = omni::fit_sync(f))) return rc;
    omni::PcaState st;
    OMNI_HIP_TRY(hipMemcpy(&st, f->acc, sizeof st, hipMemcpyDeviceToHost));
    if (n) *n = st.n;
    if (skipped) *skipped = st.skipped;
    return OMNI_OK;
}

int omni_pcafit_moments(omni_pcafit* f, double* s256, double* S_full) {
    OMNI_REQUIRE(f && s256 && S_full, OMNI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(f->mu);
    int rc;
    if ((rc = omni::fit_sync(f))) return rc;
    OMNI_HIP_TRY(hipMemcpy(s256, omni::s_of(f), (size_t)omni::pca::kDim * 8, hipMemcpyDeviceToHost));
    OMNI_HIP_TRY(hipMemcpy(S_full, omni::S_of(f), (size_t)omni::pca::kDim * omni::pca::kDim * 8, hipMemcpyDeviceToHost));
    omni::pca::mirror(S_full);
    return OMNI_OK;
}

int omni_pcafit_merge_host(int64_t* n, double* s256, double* S_full, int64_t n_right, const double* s256_right, const double* S_full_right) {
    OMNI_REQUIRE(n && s256 && S_full && s256_right && S_full_right, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(*n >= 0 && n_right >= 0, OMNI_ERR_INVALID, "negative count (n %lld, right %lld)", (long long)*n, (long long)n_right);
    omni::pca::Moments l, r;
    l.n = *n; l.s = s256; l.S = S_full;
    r.n = n_right; r.s = const_cast<double*>(s256_right); r.S = const_cast<double*>(S_full_right);
    omni::pca::merge(l, r);
    omni::pca::mirror(S_full);
    *n = l.n;
    return OMNI_OK;
}

int omni_pcafit_solve(omni_pcafit* f, int pca_dim, double* components, float* components_f32, double* mean, float* mean_f32, double* explained_variance,
                      double* total_variance) {
    OMNI_REQUIRE(f, OMNI_ERR_INVALID, "null handle");
    int64_t n = 0;
    int rc;
    if ((rc = omni_pcafit_stats(f, &n, nullptr))) return rc;
    std::vector<double> m((size_t)omni::pca::kDim * (omni::pca::kDim + 1));
    if ((rc = omni_pcafit_moments(f, m.data(), m.data() + omni::pca::kDim))) return rc;
    return omni_pca_solve_host(n, m.data(), m.data() + omni::pca::kDim, pca_dim, components, components_f32, mean, mean_f32, explained_variance, total_variance);
}

}  // extern "C"
