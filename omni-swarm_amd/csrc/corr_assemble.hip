// The correspondences of the loop candidates of one matcher round trip, assembled on the GPU behind the homography kernels (csrc/corr_plan.h has the arithmetic, the
// gate and the refusals -- this file only spreads it over lanes):
//   one workgroup of 256 lanes (4 waves) per candidate;
//   compaction   wave j takes the candidate's pair j (at most 4: MAX_DIRS).  It walks the matcher's list 64 matches at a time twice: once to count the flagged
//                matches (the quirk of loop_detector.cpp:200 needs the count first), once to keep, of the flagged ones, those the homography mask leaves -- ballot +
//                popcount keep the match order (as hg_filter_kernel).  The kept index pairs go to LDS and to new_idx / old_idx;
//   scan         after one barrier every lane sums the (at most 4) pair counts in front of its pair: the candidate's list is the pairs' lists in pairing order;
//   gathers      all 256 lanes: X = landmarks_3d of the new image, u = landmarks_2d_norm of the old one rotated by the pair's dq_old (f64, cast to float), written
//                at the candidate's slots in the layout omni_pnp_ransac_multi takes (X [n][3], u [n][2]);
//   lane 0       n_corr, matched_dir_count and the gate.
// No atomics, no scratch; no workgroup reads what another wrote or waits for one; every loop's trip count is bounded by max_n or by 4, launch arguments and a
// constant.  Every count and index read from memory is clamped before it addresses anything.  Built with contraction off (Makefile; the header's pragma says the same).
#include "common.h"
#include "corr_plan.h"

namespace omni {

__global__ __launch_bounds__(corr::THREADS) void corr_assemble_kernel(const omni_corr_io io) {
    __shared__ unsigned short s_q[corr::kMaxPairs][rs::kMaxN], s_t[corr::kMaxPairs][rs::kMaxN];
    __shared__ int s_cnt[corr::kMaxPairs];
    const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (c >= io.n_cands) return;
    const omni_corr_cand cd = io.cands[c];
    int pair_count = cd.pair_count < 0 ? 0 : (cd.pair_count > corr::kMaxPairs ? corr::kMaxPairs : cd.pair_count);
    if (cd.pair_first < 0 || cd.pair_first + pair_count > io.n_pairs) pair_count = 0;
    if ((long long)pair_count * io.max_n > io.cap) pair_count = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (wave < pair_count) {
        const int p = cd.pair_first + wave, n = corr::n_matches(io, p);
        const size_t at = (size_t)p * io.max_n;
        int n_kept = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {                      // (uniform trip count over the wave: every lane reaches the ballot)
            int qi, ti;
            const bool k = i0 + lane < n && corr::keep(io, p, i0 + lane, &qi, &ti);
            n_kept += __popcll(__ballot(k));
        }
        int rank0 = 0, count = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            int qi = 0, ti = 0;
            const bool k = i0 + lane < n && corr::keep(io, p, i0 + lane, &qi, &ti);
            const unsigned long long mk = __ballot(k);
            const bool s = k && corr::survives(io, p, n_kept, rank0 + __popcll(mk & below));
            const unsigned long long ms = __ballot(s);
            if (s) {
                const int pos = count + __popcll(ms & below);
                s_q[wave][pos] = (unsigned short)qi; s_t[wave][pos] = (unsigned short)ti;
                io.new_idx[at + pos] = qi; io.old_idx[at + pos] = ti;
            }
            rank0 += __popcll(mk); count += __popcll(ms);
        }
        if (lane == 0) { s_cnt[wave] = count; io.n_pair_corr[p] = count; }
    } else if (lane == 0) {
        s_cnt[wave] = 0;
    }
    __syncthreads();
    int off = 0;
    for (int j = 0; j < pair_count; ++j) {
        const int p = cd.pair_first + j, cnt = s_cnt[j];
        for (int k = tid; k < cnt; k += corr::THREADS) {
            const size_t slot = (size_t)c * io.cap + off + k;
            corr::gather(io, p, s_q[j][k], s_t[j][k], io.X + 3 * slot, io.u + 2 * slot);
        }
        off += cnt;
    }
    if (tid == 0) {
        int matched = 0;
        bool any_host = false;
        for (int j = 0; j < pair_count; ++j) { if (s_cnt[j] >= cd.min_match_pre_dir) ++matched; if (io.hg_status[cd.pair_first + j] == OMNI_HG_HOST) any_host = true; }
        io.n_corr[c] = off; io.matched_dir_count[c] = matched; io.gate[c] = corr::gate(cd, off, matched, any_host);
    }
}

// io: every pointer in device memory.  Asynchronous on the stream; the caller has run corr::refusal on the host's copy of the table
int corr_launch(hipStream_t stream, const omni_corr_io& io) {
    hipLaunchKernelGGL(corr_assemble_kernel, dim3((unsigned)io.n_cands), dim3(corr::THREADS), 0, stream, io);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace omni

// The kernel alone on arrays from the host (omni_homography_ransac_multi's counterpart): io as omni_corr_assemble_host takes it.  Blocking.  *kernel_us (may be
// NULL): the launch's time between two events on the stream.
extern "C" int omni_corr_assemble_multi(omni_ctx* ctx, const omni_corr_io* hio, float* kernel_us) {
    using namespace omni;
    OMNI_REQUIRE(ctx && hio && hio->cands && hio->n_corr && hio->matched_dir_count && hio->gate && hio->X && hio->u, OMNI_ERR_INVALID, "omni_corr_assemble_multi: null argument");
    const char* why = corr::refusal(hio->n_cands, hio->n_pairs, hio->max_n, hio->cap, hio->cands);
    OMNI_REQUIRE(!why, OMNI_ERR_CAPACITY, "omni_corr_assemble_multi: %s (n_cands %d, n_pairs %d, max_n %d, cap %d)", why, hio->n_cands, hio->n_pairs, hio->max_n, hio->cap);
    OMNI_REQUIRE(hio->n_pairs == 0 || (hio->q_idx && hio->t_idx && hio->n_matches && hio->q_flags && hio->n_flags && hio->nq && hio->nt && hio->mask && hio->hg_status &&
                                       hio->q_3d && hio->t_norm && hio->dq_old && hio->new_idx && hio->old_idx && hio->n_pair_corr),
                 OMNI_ERR_INVALID, "omni_corr_assemble_multi: pairs and no arrays");
    TraceRange trace_range("loop candidate correspondences");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    // Up: cands [64] | ints [7][64] (n_matches n_flags nq nt hg_status, 2 spare) | dq_old [64][4] | q_idx | t_idx [P][max_n] | q_flags | mask [P][max_n] u8 |
    // q_3d [P][max_n][3] | t_norm [P][max_n][2].  Down: counts [4][64] | new_idx | old_idx [P][max_n] | X [C][cap][3] | u [C][cap][2]
    const size_t P = (size_t)hio->n_pairs, C = (size_t)hio->n_cands, mn = (size_t)hio->max_n, cap = (size_t)hio->cap;
    const size_t fi = up256(P * mn * 4), fb = up256(P * mn), off_ints = 64 * sizeof(omni_corr_cand), off_dq = off_ints + 7 * 256, off_qi = off_dq + 64 * 32, off_ti = off_qi + fi;
    const size_t off_fl = off_ti + fi, off_mk = off_fl + fb, off_3d = off_mk + fb, off_tn = off_3d + up256(P * mn * 12), off_down = off_tn + up256(P * mn * 8);
    const size_t off_ni = off_down + 1024, off_oi = off_ni + fi, off_X = off_oi + fi, off_u = off_X + up256(C * cap * 12), total = off_u + up256(C * cap * 8);
    int rc;
    if ((rc = ctx->scratch.ensure(total))) return rc;
    if ((rc = ctx->hstage.ensure(total))) return rc;
    char *d = ctx->scratch.as<char>(), *h = ctx->hstage.as<char>();
    memset(h, 0, off_down);
    memcpy(h, hio->cands, C * sizeof(omni_corr_cand));
    int* ints = (int*)(h + off_ints);
    if (P) {
        memcpy(ints, hio->n_matches, P * 4); memcpy(ints + 64, hio->n_flags, P * 4); memcpy(ints + 128, hio->nq, P * 4); memcpy(ints + 192, hio->nt, P * 4);
        memcpy(ints + 256, hio->hg_status, P * 4);
        memcpy(h + off_dq, hio->dq_old, P * 32);
        memcpy(h + off_qi, hio->q_idx, P * mn * 4); memcpy(h + off_ti, hio->t_idx, P * mn * 4);
        memcpy(h + off_fl, hio->q_flags, P * mn); memcpy(h + off_mk, hio->mask, P * mn);
        memcpy(h + off_3d, hio->q_3d, P * mn * 12); memcpy(h + off_tn, hio->t_norm, P * mn * 8);
    }
    OMNI_HIP_TRY(hipMemcpyAsync(d, h, off_down, hipMemcpyHostToDevice, ctx->stream));
    OMNI_HIP_TRY(hipMemsetAsync(d + off_down, 0, total - off_down, ctx->stream));
    omni_corr_io io = *hio;
    const int* ints_d = (const int*)(d + off_ints);
    io.cands = (const omni_corr_cand*)d;
    io.n_matches = ints_d; io.n_flags = ints_d + 64; io.nq = ints_d + 128; io.nt = ints_d + 192; io.hg_status = ints_d + 256;
    io.dq_old = (const double*)(d + off_dq); io.q_idx = (const int*)(d + off_qi); io.t_idx = (const int*)(d + off_ti);
    io.q_flags = (const uint8_t*)(d + off_fl); io.mask = (const uint8_t*)(d + off_mk); io.q_3d = (const float*)(d + off_3d); io.t_norm = (const float*)(d + off_tn);
    io.n_corr = (int*)(d + off_down); io.matched_dir_count = io.n_corr + 64; io.gate = io.n_corr + 128; io.n_pair_corr = io.n_corr + 192;
    io.new_idx = (int*)(d + off_ni); io.old_idx = (int*)(d + off_oi); io.X = (float*)(d + off_X); io.u = (float*)(d + off_u);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (kernel_us) { OMNI_HIP_TRY(hipEventCreate(&e0)); OMNI_HIP_TRY(hipEventCreate(&e1)); OMNI_HIP_TRY(hipEventRecord(e0, ctx->stream)); }
    rc = corr_launch(ctx->stream, io);
    if (kernel_us && !rc) (void)hipEventRecord(e1, ctx->stream);
    hipError_t err = rc ? hipSuccess : hipMemcpyAsync(h + off_down, d + off_down, total - off_down, hipMemcpyDeviceToHost, ctx->stream);
    if (!rc && err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (kernel_us) {
        float ms = 0;
        if (!rc && err == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *kernel_us = ms * 1000.f;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    if (rc) return rc;
    OMNI_HIP_TRY(err);
    const int* nc = (const int*)(h + off_down);
    memcpy(hio->n_corr, nc, C * 4); memcpy(hio->matched_dir_count, nc + 64, C * 4); memcpy(hio->gate, nc + 128, C * 4);
    if (P) {
        memcpy(hio->n_pair_corr, nc + 192, P * 4);
        memcpy(hio->new_idx, h + off_ni, P * mn * 4); memcpy(hio->old_idx, h + off_oi, P * mn * 4);
    }
    memcpy(hio->X, h + off_X, C * cap * 12); memcpy(hio->u, h + off_u, C * cap * 8);
    return OMNI_OK;
}
