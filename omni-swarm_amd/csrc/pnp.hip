// omni_pnp_ransac_multi: the RANSAC half of compute_relative_pose (swarm_loop/src/loop_detector.cpp:355-413: cv::solvePnPRansac over EPnP models of five points)
// on the GPU, f64.  The arithmetic is pnp_plan.h's -- this file only spreads it over lanes:
//   pnp_ransac_kernel  one workgroup of 256 lanes per candidate, the candidate's points in LDS (static: 2 048 points x 20 bytes = 40 KB; the entry refuses more).
//                      It proceeds in rounds (pnp_plan.h): lane 0 draws the next R groups of five distinct indices from the multiply-with-carry stream (serial
//                      by nature, about six draws a group), every lane runs one EPnP hypothesis and counts its inliers (form (a) of docs/kernels.md: the
//                      12 x 12 Jacobi's two matrices and EPnP's tables in the lane's private memory, i.e. scratch), then lane 0 scans the stop rule.  R = 64 in
//                      the first round (one wave: a true loop stops after about five iterations), 256 afterwards; a round never holds more iterations than the
//                      stop rule still allows at its start (the scan cannot reach the others: niters only falls).
//     mask             the best model's, recomputed from its (R, t) by all lanes at the end.
// Every loop is bounded: at most kSubsetDrawBudget draws a group, 60 Jacobi sweeps, kMaxIters iterations.
// Built with contraction off (Makefile; the header's pragma says the same): products and sums round one by one, as the host's.
#include "common.h"
#include "pnp_plan.h"

namespace omni {

#define PNP_THREADS 256
static_assert(pnp::kRound <= PNP_THREADS && pnp::kRoundFirst <= pnp::kRound, "one lane per hypothesis");
static_assert(pnp::kMaxN * 20 + 8192 <= 65536, "the points and the round's tables fit the static LDS limit");

__global__ __launch_bounds__(PNP_THREADS) void pnp_ransac_kernel(int max_n, const float* __restrict__ X_g, const float* __restrict__ u_g, const int* __restrict__ count_g,
                                                                 const int* __restrict__ iters_g, const int* __restrict__ T_g, int T_stride, int* __restrict__ status_g,
                                                                 uint8_t* __restrict__ mask_g, double* __restrict__ Rt_g, int* __restrict__ info_g) {
    __shared__ float s_X[3 * pnp::kMaxN], s_u[2 * pnp::kMaxN];
    __shared__ unsigned short s_idx[pnp::kRound][pnp::kModelPoints];
    __shared__ int s_good[PNP_THREADS];
    __shared__ double s_best[12];
    __shared__ uint64_t s_state;
    __shared__ pnp::Scan s_scan;
    __shared__ int s_avail, s_over, s_status, s_best_j;
    const int c = blockIdx.x, lane = threadIdx.x;
    const size_t at = (size_t)c * max_n;
    int count = count_g[c], max_iters = iters_g[c];
    // (the entry refuses counts and limits outside these ranges; the clamps stay because this is where the LDS arrays are indexed: a second caller that forgot
    // the checks would write past them, not merely compute nonsense)
    count = count < 0 ? 0 : (count > max_n ? max_n : count);
    count = count > pnp::kMaxN ? pnp::kMaxN : count;
    max_iters = max_iters < 1 ? 1 : (max_iters > pnp::kMaxIters ? pnp::kMaxIters : max_iters);
    for (int i = lane; i < 3 * count; i += PNP_THREADS) s_X[i] = X_g[3 * at + i];
    for (int i = lane; i < 2 * count; i += PNP_THREADS) s_u[i] = u_g[2 * at + i];
    if (lane == 0) {
        pnp::scan_init(s_scan, max_iters);
        s_state = 0xffffffffffffffffull; s_over = 0;
        for (int k = 0; k < 12; ++k) s_best[k] = 0;
        s_status = count < 6 ? OMNI_PNP_SKIPPED : -1;
        if (count < 6) {                                          // (mask and Rt stay as the entry zeroed them)
            pnp::put_info(info_g + 4 * c, count, s_scan);
            status_g[c] = OMNI_PNP_SKIPPED;
        }
    }
    __syncthreads();
    if (s_status >= 0) return;
    const int* T = T_g + (size_t)c * T_stride;
    int base = 0, R = pnp::kRoundFirst;
    pnp::Rt rt;
    for (;;) {
        if (lane == 0) {                                          // ---- the round's subsets, in stream order
            const int left = s_scan.niters - base, want = left < R ? left : R;
            uint64_t st = s_state;
            int avail = 0, over = s_over;
            while (avail < want && !over) {
                int idx[pnp::kModelPoints];
                if (pnp::next_subset(st, count, idx)) { for (int k = 0; k < pnp::kModelPoints; ++k) s_idx[avail][k] = (unsigned short)idx[k]; ++avail; }
                else over = 1;
            }
            s_state = st; s_over = over; s_avail = avail;
        }
        __syncthreads();
        const int avail = s_avail;                                // ---- the round's hypotheses, one per lane
        int good = -1;
        if (lane < avail) {
            int idx[pnp::kModelPoints];
            for (int k = 0; k < pnp::kModelPoints; ++k) idx[k] = s_idx[lane][k];
            good = pnp::hypothesis(s_X, s_u, count, idx, rt);
        }
        s_good[lane] = good;
        __syncthreads();
        if (lane == 0) {                                          // ---- the stop rule, iteration by iteration
            pnp::Scan s = s_scan;
            int st = -1, best_j = -1;
            for (int j = 0; j <= R; ++j) {
                if (base + j >= s.niters) { st = pnp::scan_status(s); break; }
                if (j == R) break;
                if (j >= avail) { st = OMNI_PNP_HOST; break; }
                if (pnp::scan_step(s, base + j, s_good[j], T)) best_j = j;
            }
            s_scan = s; s_status = st; s_best_j = best_j;
        }
        __syncthreads();
        if (lane == s_best_j) pnp::put_rt(s_best, rt);
        __syncthreads();
        if (s_status >= 0) break;
        base += R;
        R = pnp::kRound;
    }
    const int st = s_status;
    const pnp::Rt best = pnp::get_rt(s_best);
    for (int i = lane; i < count; i += PNP_THREADS) mask_g[at + i] = st == OMNI_PNP_OK && pnp::inlier(best, s_X, s_u, i) ? 1 : 0;
    if (lane == 0) {
        pnp::put_info(info_g + 4 * c, count, s_scan);
        for (int k = 0; k < 12; ++k) Rt_g[12 * c + k] = st == OMNI_PNP_OK ? s_best[k] : 0.0;
        status_g[c] = st;
    }
}

// the stop rule's row of one count, T[good] for good <= count (pnp_plan.h: fill_T), computed once per context; the rows a call needs travel with its upload
static const int* pnp_T_row(omni_ctx* ctx, int count) {
    if ((int)ctx->pnp_T.size() <= count) ctx->pnp_T.resize((size_t)count + 1);
    std::vector<int>& row = ctx->pnp_T[(size_t)count];
    if (row.empty()) { row.assign((size_t)count + 1, 0); if (count > 0) pnp::fill_T(count, row.data()); }
    return row.data();
}
static size_t pnp_up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace omni

extern "C" {

int omni_pnp_ransac_multi(omni_ctx* ctx, int n_cands, int max_n, const float* X_xyz, const float* u_xy, const int* count, const int* max_iters, int* status, uint8_t* mask,
                          double* Rt, int* info) {
    using namespace omni;
    OMNI_REQUIRE(ctx && X_xyz && u_xy && count && max_iters && status && mask && Rt && info, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(n_cands >= 1 && n_cands <= 64, OMNI_ERR_CAPACITY, "n_cands=%d outside [1,64]", n_cands);
    OMNI_REQUIRE(max_n >= 1 && max_n <= pnp::kMaxN, OMNI_ERR_CAPACITY, "max_n=%d outside [1,%d]", max_n, pnp::kMaxN);
    for (int c = 0; c < n_cands; ++c) {
        OMNI_REQUIRE(count[c] >= 0 && count[c] <= max_n, OMNI_ERR_CAPACITY, "candidate %d: count=%d outside [0,%d]", c, count[c], max_n);
        OMNI_REQUIRE(max_iters[c] >= 1 && max_iters[c] <= pnp::kMaxIters, OMNI_ERR_CAPACITY, "candidate %d: max_iters=%d outside [1,%d]", c, max_iters[c], pnp::kMaxIters);
    }
    TraceRange trace_range("PnP RANSAC");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    // device scratch layout: X [C][max_n][3] | u [C][max_n][2] f32 | count [64] | max_iters [64] | T [C][max_n + 1] || status [64] | info [64][4] | Rt [64][12] f64 |
    // mask [C][max_n]
    const size_t C = (size_t)n_cands, T_stride = (size_t)max_n + 1;
    const size_t off_u = pnp_up256(C * max_n * 12), off_cnt = off_u + pnp_up256(C * max_n * 8), off_it = off_cnt + 256, off_T = off_it + 256;
    const size_t off_out = off_T + pnp_up256(C * T_stride * 4), off_info = off_out + 256, off_Rt = off_info + 1024, off_mask = off_Rt + 64 * 96;
    const size_t total = off_mask + pnp_up256(C * max_n);
    int rc;
    if ((rc = ctx->scratch.ensure(total))) return rc;
    if ((rc = ctx->hstage.ensure(total))) return rc;
    char *d = ctx->scratch.as<char>(), *h = ctx->hstage.as<char>();
    memcpy(h, X_xyz, C * max_n * 12);
    memcpy(h + off_u, u_xy, C * max_n * 8);
    memcpy(h + off_cnt, count, C * 4);
    memcpy(h + off_it, max_iters, C * 4);
    for (int c = 0; c < n_cands; ++c) memcpy(h + off_T + (size_t)c * T_stride * 4, pnp_T_row(ctx, count[c]), ((size_t)count[c] + 1) * 4);
    OMNI_HIP_TRY(hipMemcpyAsync(d, h, off_out, hipMemcpyHostToDevice, ctx->stream));
    OMNI_HIP_TRY(hipMemsetAsync(d + off_out, 0, total - off_out, ctx->stream));
    hipLaunchKernelGGL(pnp_ransac_kernel, dim3(n_cands), dim3(PNP_THREADS), 0, ctx->stream, max_n, (const float*)d, (const float*)(d + off_u), (const int*)(d + off_cnt),
                       (const int*)(d + off_it), (const int*)(d + off_T), (int)T_stride, (int*)(d + off_out), (uint8_t*)(d + off_mask), (double*)(d + off_Rt),
                       (int*)(d + off_info));
    OMNI_LAUNCH_CHECK();
    OMNI_HIP_TRY(hipMemcpyAsync(h + off_out, d + off_out, total - off_out, hipMemcpyDeviceToHost, ctx->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(status, h + off_out, C * 4);
    memcpy(info, h + off_info, C * 16);
    memcpy(Rt, h + off_Rt, C * 96);
    memcpy(mask, h + off_mask, C * max_n);
    return OMNI_OK;
}

}  // extern "C"
