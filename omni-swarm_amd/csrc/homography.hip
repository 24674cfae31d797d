// omni_homography_ransac_multi / omni_bf_match_homography_multi: the flag filter and the homography RANSAC of compute_correspond_features
// (swarm_loop/src/loop_detector.cpp:574-598) on the GPU, f64.  The arithmetic is ransac_plan.h's -- this file only spreads it over lanes:
//   hg_filter_kernel   one workgroup per pair: wave 0 walks the matcher's list 64 matches at a time, ballot + popcount keep the order (as bf_cross_kernel);
//                      the kept positions, and the two pixels of every kept match as the RANSAC kernel's point lists;
//   hg_ransac_kernel   one workgroup of 256 lanes per pair, the pair's points in LDS.  It proceeds in rounds (ransac_plan.h): the next R subsets, their R
//                      hypotheses one per lane (the two 9 x 9 matrices of the cyclic Jacobi in the lane's private memory), then the scan of the stop rule on
//                      lane 0; R = 64 in the first round (a true loop stops after about ten iterations), 256 afterwards.
//     subsets          the multiply-with-carry stream is serial: lane 0 draws 256 numbers, all lanes reduce them modulo count (an exact integer remainder);
//                      where an attempt (four distinct indices) starts is only known in stream order, so EVERY position is tried as a start by its own lane
//                      (its end, its indices, check_subset), and lane 0 then only hops from end to end, appends the passing attempts in stream order and
//                      keeps the budgets.  Attempts beyond the round's R stay queued for the next round.
//     mask             the best model's, recomputed from its H by all lanes at the end.
// Built with contraction off (Makefile; the header's pragma says the same): products and sums round one by one, as the host's.
#include "common.h"
#include "ransac_plan.h"
#include "corr_plan.h"

namespace omni {

int bf_launch(omni_ctx* ctx, int n_pairs, int max_n, int dim, int mode, const float* q, int64_t qs, const int* nq, const float* t, int64_t ts, const int* nt, int* oq,
              int* ot, float* od, int* on);                  // bfmatch.hip

int corr_launch(hipStream_t stream, const omni_corr_io& io);      // corr_assemble.hip

#define HG_THREADS 256
static_assert(rs::kRound <= HG_THREADS && rs::kRawChunk == HG_THREADS && rs::kRoundFirst <= rs::kRound, "one lane per hypothesis and per drawn number");

__global__ __launch_bounds__(64) void hg_filter_kernel(int max_n, const int* __restrict__ n_matches, const int* __restrict__ q_idx, const int* __restrict__ t_idx,
                                                               const float* __restrict__ q_xy, const float* __restrict__ t_xy, const uint8_t* __restrict__ flags,
                                                               const int* __restrict__ nq_arr, const int* __restrict__ nt_arr, const int* __restrict__ n_flags,
                                                               int* __restrict__ kept, int* __restrict__ n_kept, float* __restrict__ src, float* __restrict__ dst) {
    const int p = blockIdx.x, tid = threadIdx.x;                  // one wave
    const size_t at = (size_t)p * max_n;
    int n = n_matches[p], nf = n_flags[p];
    n = n < 0 ? 0 : (n > max_n ? max_n : n);
    nf = nf < 0 ? 0 : (nf > max_n ? max_n : nf);
    const int nq = nq_arr[p], nt = nt_arr[p];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {                      // (uniform trip count: every lane reaches the ballot)
        const int i = i0 + tid;
        int qi = 0, ti = 0;
        bool keep = false;
        if (i < n) {
            qi = q_idx[at + i]; ti = t_idx[at + i];
            keep = rs::flag_keep(qi, flags + at, nf) && qi < nq && ti >= 0 && ti < nt;      // (the matcher's indices lie inside their images)
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const size_t pos = at + base + __popcll(m & ((1ull << tid) - 1ull));
            kept[pos] = i;
            src[2 * pos] = t_xy[2 * (at + ti)]; src[2 * pos + 1] = t_xy[2 * (at + ti) + 1];
            dst[2 * pos] = q_xy[2 * (at + qi)]; dst[2 * pos + 1] = q_xy[2 * (at + qi) + 1];
        }
        base += __popcll(m);
    }
    if (tid == 0) n_kept[p] = base;
}

__global__ __launch_bounds__(HG_THREADS) void hg_ransac_kernel(int max_n, const float* __restrict__ src_g, const float* __restrict__ dst_g, const int* __restrict__ count_g,
                                                               const int* __restrict__ T_tab, int T_stride, int* __restrict__ status_g, uint8_t* __restrict__ mask_g,
                                                               double* __restrict__ H_g, int* __restrict__ info_g) {
    __shared__ float s_src[2 * rs::kMaxN], s_dst[2 * rs::kMaxN];
    __shared__ unsigned s_raw[rs::kRawChunk];
    __shared__ unsigned s_next[rs::kRawChunk];
    __shared__ unsigned short s_idx4[rs::kRawChunk][4], s_queue[rs::kRound + rs::kAttChunk][4];
    __shared__ int s_good[HG_THREADS];
    __shared__ double s_best[9];
    __shared__ rs::Gen s_gen;
    __shared__ rs::Scan s_scan;
    __shared__ int s_nq, s_status, s_best_j, s_any;
    const int p = blockIdx.x, lane = threadIdx.x;
    const size_t at = (size_t)p * max_n;
    int count = count_g[p];
    count = count < 0 ? 0 : (count > max_n ? max_n : count);
    for (int i = lane; i < 2 * count; i += HG_THREADS) { s_src[i] = src_g[2 * at + i]; s_dst[i] = dst_g[2 * at + i]; }
    if (lane == 0) s_any = 0;
    __syncthreads();
    if (count > 4 && count <= rs::kEnumMax && rs::any_valid_subset(s_src, s_dst, count, lane, HG_THREADS)) s_any = 1;      // (every writer stores the same 1)
    __syncthreads();
    if (lane == 0) {
        int tie;
        s_status = rs::special_cases(s_src, s_dst, count, s_any != 0, mask_g + at, H_g + 9 * p, info_g + 4 * p, &tie);
        if (s_status >= 0) status_g[p] = s_status;
        rs::gen_init(s_gen); rs::scan_init(s_scan);
        s_nq = 0;
    }
    __syncthreads();
    if (s_status >= 0) return;
    const int* T = T_tab + (size_t)count * T_stride;
    int base = 0, R = rs::kRoundFirst;
    double H[9];
    for (;;) {
        for (;;) {                                                // ---- subsets until the round is full or a budget is passed
            __syncthreads();
            if (s_nq >= R || s_gen.over) break;
            if (lane == 0) { uint64_t st = s_gen.state; for (int d = 0; d < rs::kRawChunk; ++d) s_raw[d] = rs::rng_next(st); s_gen.state = st; }
            __syncthreads();
            s_raw[lane] = rs::rng_residue(s_raw[lane], count);
            __syncthreads();
            {                                                     // every position as if an attempt started there: its end, its indices, its verdict
                int idx[4] = {0, 0, 0, 0};
                const int end = rs::gen_attempt_at(s_raw, lane, rs::kRawChunk, idx);
                const bool pass = end != 0 && rs::check_subset(s_src, s_dst, idx);
                s_next[lane] = (unsigned)end | (pass ? 1u << 16 : 0u);
                for (int k = 0; k < 4; ++k) s_idx4[lane][k] = (unsigned short)idx[k];
            }
            __syncthreads();
            if (lane == 0) {                                      // the attempts that ARE in the stream, in order: from end to end
                rs::Gen g = s_gen;
                const int draws0 = g.draws;
                int nq = s_nq, pos = 0;
                while (pos < rs::kRawChunk && g.i != 0)           // the attempt the last chunk left unfinished
                    if (rs::gen_feed(g, (int)s_raw[pos++])) {
                        const int idx[4] = {g.idx[0], g.idx[1], g.idx[2], g.idx[3]};
                        if (rs::gen_attempt(g, rs::check_subset(s_src, s_dst, idx), g.draws) == 1) { for (int k = 0; k < 4; ++k) s_queue[nq][k] = (unsigned short)idx[k]; ++nq; }
                    }
                if (g.i == 0) {
                    while (pos < rs::kRawChunk) {
                        const unsigned ne = s_next[pos];
                        const int end = (int)(ne & 0xffffu);
                        if (end == 0) break;
                        if (rs::gen_attempt(g, (ne >> 16) != 0, draws0 + end) == 1) { for (int k = 0; k < 4; ++k) s_queue[nq][k] = s_idx4[pos][k]; ++nq; }
                        pos = end;
                    }
                    while (pos < rs::kRawChunk) rs::gen_feed(g, (int)s_raw[pos++]);      // the first numbers of the attempt the next chunk finishes
                }
                g.draws = draws0 + rs::kRawChunk;
                s_gen = g; s_nq = nq;
            }
        }
        const int nq = s_nq, avail = nq < R ? nq : R;             // ---- the round's hypotheses, one per lane
        int good = -1, tie = 0;
        if (lane < avail) { const int idx[4] = {s_queue[lane][0], s_queue[lane][1], s_queue[lane][2], s_queue[lane][3]}; good = rs::hypothesis(s_src, s_dst, count, idx, H, &tie); }
        s_good[lane] = good;
        __syncthreads();
        if (lane == 0) {                                          // ---- the stop rule, iteration by iteration
            rs::Scan s = s_scan;
            int st = -1, best_j = -1;
            for (int j = 0; j < R; ++j) {
                if (base + j >= s.niters) { st = s.max_good > 0 ? OMNI_HG_OK : OMNI_HG_NO_MODEL; break; }
                if (j >= avail) { st = OMNI_HG_HOST; break; }
                if (rs::scan_step(s, base + j, s_good[j], T)) best_j = j;
            }
            s_scan = s; s_status = st; s_best_j = best_j;
        }
        unsigned short keep4[4] = {0, 0, 0, 0};                    // the attempts queued beyond this round move to the front (at most kAttChunk - 1 of them)
        const bool mv = R + lane < nq;
        if (mv) for (int k = 0; k < 4; ++k) keep4[k] = s_queue[R + lane][k];
        __syncthreads();
        if (lane == s_best_j) for (int k = 0; k < 9; ++k) s_best[k] = H[k];
        if (mv) for (int k = 0; k < 4; ++k) s_queue[lane][k] = keep4[k];
        if (lane == 0) s_nq = nq > R ? nq - R : 0;
        __syncthreads();
        if (s_status >= 0) break;
        base += R;
        R = rs::kRound;
    }
    const int st = s_status;
    for (int i = lane; i < count; i += HG_THREADS) mask_g[at + i] = st == OMNI_HG_OK && rs::inlier(s_best, s_src, s_dst, i) ? 1 : 0;
    if (lane == 0) {
        rs::put_info(info_g + 4 * p, count, s_scan);
        for (int k = 0; k < 9; ++k) H_g[9 * p + k] = st == OMNI_HG_OK ? s_best[k] : 0.0;
        status_g[p] = st;
    }
}

// the stop rule's table in HBM: T[count][good] for count <= n, row stride n + 1 (ransac_plan.h: fill_T); grows with the largest max_n seen
static int ensure_T(omni_ctx* ctx, int max_n) {
    if (ctx->ransac_T_n >= max_n) return OMNI_OK;
    const int n = max_n < 256 ? 256 : max_n, stride = n + 1;
    std::vector<int> tab((size_t)stride * stride, 0);
    for (int c = 1; c <= n; ++c) rs::fill_T(c, tab.data() + (size_t)c * stride);
    int rc;
    OMNI_HIP_TRY(hipStreamSynchronize(ctx->stream));              // (a kernel in flight may still read the smaller table)
    ctx->ransac_T_n = 0;
    if ((rc = ctx->ransac_T.ensure(tab.size() * 4))) return rc;
    OMNI_HIP_TRY(hipMemcpy(ctx->ransac_T.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    ctx->ransac_T_n = n;
    return OMNI_OK;
}
static int ransac_launch(omni_ctx* ctx, int n_pairs, int max_n, const float* src, const float* dst, const int* count, int* status, uint8_t* mask, double* H, int* info) {
    hipLaunchKernelGGL(hg_ransac_kernel, dim3(n_pairs), dim3(HG_THREADS), 0, ctx->stream, max_n, src, dst, count, ctx->ransac_T.as<int>(), ctx->ransac_T_n + 1, status, mask, H,
                       info);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}
static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// what omni_bf_match_homography_corr_multi adds to the round trip: the candidates, the gathers' sources and where the stage's outputs go (all host memory)
struct CorrHost {
    int n_cands; const omni_corr_cand* cands; int cap; const float* const* q_3d; const float* const* t_norm; const double* dq_old;
    float *X, *u; int *n_corr, *matched_dir_count, *gate, *new_idx, *old_idx, *n_pair_corr;
};

}  // namespace omni

extern "C" {

int omni_homography_ransac_multi(omni_ctx* ctx, int n_pairs, int max_n, const float* src_xy, const float* dst_xy, const int* count, int* status, uint8_t* mask, double* H,
                                 int* info) {
    using namespace omni;
    OMNI_REQUIRE(ctx && src_xy && dst_xy && count && status && mask && H && info, OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(n_pairs >= 1 && n_pairs <= 64, OMNI_ERR_CAPACITY, "n_pairs=%d outside [1,64]", n_pairs);
    OMNI_REQUIRE(max_n >= 1 && max_n <= rs::kMaxN, OMNI_ERR_CAPACITY, "max_n=%d outside [1,%d]", max_n, rs::kMaxN);
    for (int p = 0; p < n_pairs; ++p) OMNI_REQUIRE(count[p] >= 0 && count[p] <= max_n, OMNI_ERR_CAPACITY, "pair %d: count=%d outside [0,%d]", p, count[p], max_n);
    TraceRange trace_range("homography RANSAC");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    // device scratch layout: src | dst [P][max_n][2] f32 | count [64] || status [64] | info [64][4] | H [64][9] f64 | mask [P][max_n]
    const size_t P = (size_t)n_pairs, f_pts = up256(P * max_n * 8), off_dst = f_pts, off_cnt = 2 * f_pts, off_out = off_cnt + 256;
    const size_t off_info = off_out + 256, off_H = off_info + 1024, off_mask = off_H + 64 * 72, total = off_mask + up256(P * max_n);
    int rc;
    if ((rc = ensure_T(ctx, max_n))) return rc;
    if ((rc = ctx->scratch.ensure(total))) return rc;
    if ((rc = ctx->hstage.ensure(total))) return rc;
    char *d = ctx->scratch.as<char>(), *h = ctx->hstage.as<char>();
    memcpy(h, src_xy, P * max_n * 8);
    memcpy(h + off_dst, dst_xy, P * max_n * 8);
    memcpy(h + off_cnt, count, P * 4);
    OMNI_HIP_TRY(hipMemcpyAsync(d, h, off_out, hipMemcpyHostToDevice, ctx->stream));
    OMNI_HIP_TRY(hipMemsetAsync(d + off_out, 0, total - off_out, ctx->stream));
    if ((rc = ransac_launch(ctx, n_pairs, max_n, (const float*)d, (const float*)(d + off_dst), (const int*)(d + off_cnt), (int*)(d + off_out), (uint8_t*)(d + off_mask),
                            (double*)(d + off_H), (int*)(d + off_info))))
        return rc;
    OMNI_HIP_TRY(hipMemcpyAsync(h + off_out, d + off_out, total - off_out, hipMemcpyDeviceToHost, ctx->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(status, h + off_out, P * 4);
    memcpy(info, h + off_info, P * 16);
    memcpy(H, h + off_H, P * 72);
    memcpy(mask, h + off_mask, P * max_n);
    return OMNI_OK;
}

}  // extern "C"

// the round trip of both entries; corr == nullptr: omni_bf_match_homography_multi's, to the byte
static int bf_match_homography_run(omni_ctx* ctx, int n_pairs, const float* const* q_host, const int* nq, const float* const* t_host, const int* nt, int dim, int mode,
                                   int max_n, const float* const* q_xy, const float* const* t_xy, const uint8_t* const* q_flags, const int* n_flags, int* q_idx, int* t_idx,
                                   float* dist, int* n_matches, int* kept, int* n_kept, uint8_t* mask, double* H, int* info, int* status, const omni::CorrHost* corr) {
    using namespace omni;
    OMNI_REQUIRE(ctx && q_host && t_host && nq && nt && q_xy && t_xy && q_flags && n_flags && q_idx && t_idx && dist && n_matches && kept && n_kept && mask && H && info && status,
                 OMNI_ERR_INVALID, "null argument");
    OMNI_REQUIRE(n_pairs >= 1 && n_pairs <= 64, OMNI_ERR_CAPACITY, "n_pairs=%d outside [1,64]", n_pairs);
    OMNI_REQUIRE(max_n >= 1 && max_n <= rs::kMaxN && dim >= 4 && dim <= 256, OMNI_ERR_CAPACITY, "max_n=%d dim=%d", max_n, dim);
    for (int p = 0; p < n_pairs; ++p) {
        OMNI_REQUIRE(nq[p] >= 0 && nt[p] >= 0 && nq[p] <= max_n && nt[p] <= max_n, OMNI_ERR_CAPACITY, "pair %d: nq=%d nt=%d outside [0,%d]", p, nq[p], nt[p], max_n);
        OMNI_REQUIRE(n_flags[p] >= 0 && n_flags[p] <= max_n, OMNI_ERR_CAPACITY, "pair %d: n_flags=%d outside [0,%d]", p, n_flags[p], max_n);
        OMNI_REQUIRE((nq[p] == 0 || (q_host[p] && q_xy[p])) && (nt[p] == 0 || (t_host[p] && t_xy[p])) && (n_flags[p] == 0 || q_flags[p]), OMNI_ERR_INVALID,
                     "pair %d: null descriptors, points or flags", p);
    }
    TraceRange trace_range("BF match + flag filter + homography RANSAC");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    // device scratch layout.  Up: q | t [P][max_n][dim] | q_xy | t_xy [P][max_n][2] | flags [P][max_n] | nq nt n_flags [3][64].  Work: src | dst [P][max_n][2].
    // Down: oq | ot | od | kept [P][max_n] | on | n_kept | status [64] | info [64][4] | H [64][9] | mask [P][max_n]
    const size_t P = (size_t)n_pairs, slab = (size_t)max_n * dim * 4, fq = up256(P * slab), f_xy = up256(P * max_n * 8), f_fl = up256(P * max_n), fo = up256(P * max_n * 4);
    const size_t off_t = fq, off_qxy = 2 * fq, off_txy = off_qxy + f_xy, off_fl = off_txy + f_xy, off_n = off_fl + f_fl, off_src = off_n + 768, off_dst = off_src + f_xy;
    const size_t off_oq = off_dst + f_xy, off_ot = off_oq + fo, off_od = off_ot + fo, off_kept = off_od + fo, off_on = off_kept + fo, off_nk = off_on + 256;
    const size_t off_st = off_nk + 256, off_info = off_st + 256, off_H = off_info + 1024, off_mask = off_H + 64 * 72, hg_total = off_mask + f_fl;
    // the correspondence stage behind it.  Down (behind mask, so that the one download takes it along): new_idx | old_idx [P][max_n] | n_corr | matched | gate |
    // n_pair_corr [64] | X [C][cap][3] | u [C][cap][2].  Up (a second copy): cands [64] | dq_old [64][4] | q_3d [P][max_n][3] | t_norm [P][max_n][2]
    const size_t C = corr ? (size_t)corr->n_cands : 0, cap = corr ? (size_t)corr->cap : 0, f_X = up256(C * cap * 12), f_u = up256(C * cap * 8), f_3d = up256(P * max_n * 12);
    const size_t off_ni = hg_total, off_oi = off_ni + fo, off_nc = off_oi + fo, off_X = off_nc + 1024, off_u = off_X + f_X, down_end = corr ? off_u + f_u : hg_total;
    const size_t off_cd = down_end, off_dq = off_cd + 64 * sizeof(omni_corr_cand), off_3d = off_dq + 64 * 32, off_tn = off_3d + f_3d;
    const size_t total = corr ? off_tn + f_xy : hg_total;
    int rc;
    if ((rc = ensure_T(ctx, max_n))) return rc;
    if ((rc = ctx->scratch.ensure(total))) return rc;
    if ((rc = ctx->hstage.ensure(total))) return rc;
    char *d = ctx->scratch.as<char>(), *h = ctx->hstage.as<char>();
    if (corr) {
        memcpy(h + off_cd, corr->cands, C * sizeof(omni_corr_cand));
        memcpy(h + off_dq, corr->dq_old, P * 32);
        for (int p = 0; p < n_pairs; ++p) {
            if (nq[p]) memcpy(h + off_3d + (size_t)p * max_n * 12, corr->q_3d[p], (size_t)nq[p] * 12);
            if (nt[p]) memcpy(h + off_tn + (size_t)p * max_n * 8, corr->t_norm[p], (size_t)nt[p] * 8);
        }
        OMNI_HIP_TRY(hipMemcpyAsync(d + off_cd, h + off_cd, total - off_cd, hipMemcpyHostToDevice, ctx->stream));
    }
    for (int p = 0; p < n_pairs; ++p) {
        if (nq[p]) { memcpy(h + (size_t)p * slab, q_host[p], (size_t)nq[p] * dim * 4); memcpy(h + off_qxy + (size_t)p * max_n * 8, q_xy[p], (size_t)nq[p] * 8); }
        if (nt[p]) { memcpy(h + off_t + (size_t)p * slab, t_host[p], (size_t)nt[p] * dim * 4); memcpy(h + off_txy + (size_t)p * max_n * 8, t_xy[p], (size_t)nt[p] * 8); }
        if (n_flags[p]) memcpy(h + off_fl + (size_t)p * max_n, q_flags[p], (size_t)n_flags[p]);
        ((int*)(h + off_n))[p] = nq[p]; ((int*)(h + off_n))[64 + p] = nt[p]; ((int*)(h + off_n))[128 + p] = n_flags[p];
    }
    OMNI_HIP_TRY(hipMemcpyAsync(d, h, off_src, hipMemcpyHostToDevice, ctx->stream));
    OMNI_HIP_TRY(hipMemsetAsync(d + off_st, 0, down_end - off_st, ctx->stream));
    const int *nq_d = (const int*)(d + off_n), *nt_d = nq_d + 64, *nf_d = nq_d + 128;
    if ((rc = bf_launch(ctx, n_pairs, max_n, dim, mode, (const float*)d, (int64_t)max_n * dim, nq_d, (const float*)(d + off_t), (int64_t)max_n * dim, nt_d, (int*)(d + off_oq),
                        (int*)(d + off_ot), (float*)(d + off_od), (int*)(d + off_on))))
        return rc;
    hipLaunchKernelGGL(hg_filter_kernel, dim3(n_pairs), dim3(64), 0, ctx->stream, max_n, (const int*)(d + off_on), (const int*)(d + off_oq), (const int*)(d + off_ot),
                       (const float*)(d + off_qxy), (const float*)(d + off_txy), (const uint8_t*)(d + off_fl), nq_d, nt_d, nf_d, (int*)(d + off_kept), (int*)(d + off_nk),
                       (float*)(d + off_src), (float*)(d + off_dst));
    OMNI_LAUNCH_CHECK();
    if ((rc = ransac_launch(ctx, n_pairs, max_n, (const float*)(d + off_src), (const float*)(d + off_dst), (const int*)(d + off_nk), (int*)(d + off_st), (uint8_t*)(d + off_mask),
                            (double*)(d + off_H), (int*)(d + off_info))))
        return rc;
    if (corr) {
        omni_corr_io io{};
        io.n_cands = corr->n_cands; io.n_pairs = n_pairs; io.max_n = max_n; io.cap = corr->cap;
        io.cands = (const omni_corr_cand*)(d + off_cd);
        io.q_idx = (const int*)(d + off_oq); io.t_idx = (const int*)(d + off_ot); io.n_matches = (const int*)(d + off_on);
        io.q_flags = (const uint8_t*)(d + off_fl); io.n_flags = nf_d; io.nq = nq_d; io.nt = nt_d;
        io.mask = (const uint8_t*)(d + off_mask); io.hg_status = (const int*)(d + off_st);
        io.q_3d = (const float*)(d + off_3d); io.t_norm = (const float*)(d + off_tn); io.dq_old = (const double*)(d + off_dq);
        io.X = (float*)(d + off_X); io.u = (float*)(d + off_u);
        io.n_corr = (int*)(d + off_nc); io.matched_dir_count = io.n_corr + 64; io.gate = io.n_corr + 128; io.n_pair_corr = io.n_corr + 192;
        io.new_idx = (int*)(d + off_ni); io.old_idx = (int*)(d + off_oi);
        if ((rc = corr_launch(ctx->stream, io))) return rc;
    }
    OMNI_HIP_TRY(hipMemcpyAsync(h + off_oq, d + off_oq, down_end - off_oq, hipMemcpyDeviceToHost, ctx->stream));
    OMNI_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (corr) {
        const int* nc = (const int*)(h + off_nc);
        memcpy(corr->n_corr, nc, C * 4); memcpy(corr->matched_dir_count, nc + 64, C * 4); memcpy(corr->gate, nc + 128, C * 4); memcpy(corr->n_pair_corr, nc + 192, P * 4);
        for (size_t c = 0; c < C; ++c) {
            const size_t n = (size_t)(nc[c] < 0 ? 0 : ((size_t)nc[c] > cap ? (int)cap : nc[c]));
            memcpy(corr->X + c * cap * 3, h + off_X + c * cap * 12, n * 12);
            memcpy(corr->u + c * cap * 2, h + off_u + c * cap * 8, n * 8);
        }
        for (int p = 0; p < n_pairs; ++p) {
            const int k = nc[192 + p] < 0 ? 0 : (nc[192 + p] > max_n ? max_n : nc[192 + p]);
            memcpy(corr->new_idx + (size_t)p * max_n, h + off_ni + (size_t)p * max_n * 4, (size_t)k * 4);
            memcpy(corr->old_idx + (size_t)p * max_n, h + off_oi + (size_t)p * max_n * 4, (size_t)k * 4);
        }
    }
    memset(mask, 0, P * max_n);
    for (int p = 0; p < n_pairs; ++p) {
        const size_t row = (size_t)p * max_n;
        const int n = (nq[p] && nt[p]) ? ((int*)(h + off_on))[p] : 0, nk = ((int*)(h + off_nk))[p];      // BFMatcher on an empty set returns no matches
        memcpy(q_idx + row, h + off_oq + row * 4, (size_t)n * 4);
        memcpy(t_idx + row, h + off_ot + row * 4, (size_t)n * 4);
        memcpy(dist + row, h + off_od + row * 4, (size_t)n * 4);
        memcpy(kept + row, h + off_kept + row * 4, (size_t)nk * 4);
        memcpy(mask + row, h + off_mask + row, (size_t)nk);
        n_matches[p] = n; n_kept[p] = nk;
    }
    memcpy(status, h + off_st, P * 4);
    memcpy(info, h + off_info, P * 16);
    memcpy(H, h + off_H, P * 72);
    return OMNI_OK;
}

extern "C" {

int omni_bf_match_homography_multi(omni_ctx* ctx, int n_pairs, const float* const* q_host, const int* nq, const float* const* t_host, const int* nt, int dim, int mode,
                                   int max_n, const float* const* q_xy, const float* const* t_xy, const uint8_t* const* q_flags, const int* n_flags, int* q_idx, int* t_idx,
                                   float* dist, int* n_matches, int* kept, int* n_kept, uint8_t* mask, double* H, int* info, int* status) {
    return bf_match_homography_run(ctx, n_pairs, q_host, nq, t_host, nt, dim, mode, max_n, q_xy, t_xy, q_flags, n_flags, q_idx, t_idx, dist, n_matches, kept, n_kept, mask, H,
                                   info, status, nullptr);
}

int omni_bf_match_homography_corr_multi(omni_ctx* ctx, int n_pairs, const float* const* q_host, const int* nq, const float* const* t_host, const int* nt, int dim,
                                        int mode, int max_n, const float* const* q_xy, const float* const* t_xy, const uint8_t* const* q_flags, const int* n_flags,
                                        int n_cands, const omni_corr_cand* cands, int cap, const float* const* q_3d, const float* const* t_norm, const double* dq_old,
                                        int* q_idx, int* t_idx, float* dist, int* n_matches, int* kept, int* n_kept, uint8_t* mask, double* H, int* info, int* status,
                                        float* X, float* u, int* n_corr, int* matched_dir_count, int* gate, int* new_idx, int* old_idx, int* n_pair_corr) {
    using namespace omni;
    OMNI_REQUIRE(cands && q_3d && t_norm && dq_old && X && u && n_corr && matched_dir_count && gate && new_idx && old_idx && n_pair_corr && nq && nt, OMNI_ERR_INVALID,
                 "omni_bf_match_homography_corr_multi: null argument");
    const char* why = n_pairs < 1 ? "n_pairs < 1" : corr::refusal(n_cands, n_pairs, max_n, cap, cands);
    OMNI_REQUIRE(!why, OMNI_ERR_CAPACITY, "omni_bf_match_homography_corr_multi: %s (n_cands %d, n_pairs %d, max_n %d, cap %d)", why, n_cands, n_pairs, max_n, cap);
    for (int p = 0; p < n_pairs && p < 64; ++p)
        OMNI_REQUIRE((nq[p] <= 0 || q_3d[p]) && (nt[p] <= 0 || t_norm[p]), OMNI_ERR_INVALID, "omni_bf_match_homography_corr_multi: pair %d: null landmarks", p);
    const CorrHost corr{n_cands, cands, cap, q_3d, t_norm, dq_old, X, u, n_corr, matched_dir_count, gate, new_idx, old_idx, n_pair_corr};
    return bf_match_homography_run(ctx, n_pairs, q_host, nq, t_host, nt, dim, mode, max_n, q_xy, t_xy, q_flags, n_flags, q_idx, t_idx, dist, n_matches, kept, n_kept, mask, H,
                                   info, status, &corr);
}

}  // extern "C"
