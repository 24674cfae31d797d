// The 4-DoF pose graph on the GPU (csrc/pgo_plan.h has the residual, the Jacobians, the loss, the sums' shapes and the whole Levenberg-Marquardt / conjugate-gradient
// solver -- this file only gives it a team of lanes).  omni_pgo_solve_multi solves K initial pose sets of ONE graph in ONE launch between one upload and one download:
//   pgo_solve_kernel    grid K, 256 lanes: workgroup k runs pgo::solve_team on start k.  Lanes take edges in the per-edge passes and poses in the per-pose passes,
//                       __syncthreads between phases; the header's fixed-shape sum is what the workgroup executes, its tree in 16 KiB of LDS.
// A workgroup owns its start completely: a slab of pgo::slab_doubles(n, m) doubles in HBM holds its poses, candidate poses, the CG vectors, the diagonal blocks with
// their factors, two sets of per-edge linearisations and J p.  The slab is in HBM at EVERY size: at the limits (4096 poses, 16384 edges) it is 5.2 MB, and a window
// of 3 drones x 50 key frames (150 poses, 160 edges: 56 x 150 + 28 x 160 doubles = 103 KB) would fit the 160 KiB of LDS only without the second linearisation --
// one placement, one code path, and the slab of a window-sized start stays in L2.  The graph itself (edges, incidence lists, the active bytes) is shared and read-only.  No workgroup waits for another or
// reads what another wrote; every loop's trip count is a launch argument (n, m, max_iterations, max_lambda_retries, max_cg_iterations, the lists' lengths from the
// uploaded offsets, which the host built); no atomics.  Every index is inside its array by the refusals of omni_pgo_solve_multi (pgo::graph_refusal: i, j < n) and by
// plan_graph's construction (offsets[n] = 2 m).  Built with contraction off (Makefile; the header's pragma says the same).
#include "common.h"
#include "pgo_plan.h"

struct omni_pgo {
    omni_ctx* ctx = nullptr;
    omni::DevBuf in, slabs, out;          // in: edges | poses_in | offsets | incident | active;  out: poses_out | stats
    omni::HostBuf hin, hout;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around the launch, for kernel_us: made once with the handle
    std::mutex mu;
};

namespace omni {

struct DevTeam {
    double* red;
    __device__ int tid() const { return (int)threadIdx.x; }
    __device__ int size() const { return pgo::THREADS; }
    __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(pgo::THREADS) void pgo_solve_kernel(const pgo::Graph G, const omni_pgo_params pr, const double* __restrict__ poses_in, double* __restrict__ slabs,
                                                                 size_t slab_doubles, double* __restrict__ poses_out, omni_pgo_stats* __restrict__ stats, int n_starts) {
    __shared__ double red[pgo::kRedDoubles];
    const int k = (int)blockIdx.x;
    if (k >= n_starts) return;
    DevTeam team;
    team.red = red;
    pgo::solve_team(team, G, pr, poses_in + (size_t)k * 4 * G.n, slabs + (size_t)k * slab_doubles, poses_out + (size_t)k * 4 * G.n, stats + k);
}

static inline size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

}  // namespace omni

extern "C" int omni_pgo_create(omni_ctx* ctx, omni_pgo** out) {
    using namespace omni;
    OMNI_REQUIRE(ctx && out, OMNI_ERR_INVALID, "omni_pgo_create: null argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    omni_pgo* p = new omni_pgo;
    p->ctx = ctx;
    if (hipEventCreate(&p->e0) != hipSuccess || hipEventCreate(&p->e1) != hipSuccess) {
        set_error("omni_pgo_create: hipEventCreate failed");
        if (p->e0) (void)hipEventDestroy(p->e0);
        delete p;
        return OMNI_ERR_HIP;
    }
    *out = p;
    return OMNI_OK;
}

extern "C" void omni_pgo_destroy(omni_pgo* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    p->in.release(); p->slabs.release(); p->out.release();
    p->hin.release(); p->hout.release();
    (void)hipEventDestroy(p->e0); (void)hipEventDestroy(p->e1);
    delete p;
}

extern "C" int omni_pgo_solve_multi(omni_pgo* p, const omni_pgo_params* params, const double* poses_in, const uint8_t* fixed, const omni_pgo_edge* edges, int n_poses,
                                    int n_edges, int n_starts, double* poses_out, omni_pgo_stats* stats_out, int* best, float* kernel_us) {
    using namespace omni;
    OMNI_REQUIRE(p && params && poses_in && fixed && (edges || n_edges <= 0) && poses_out && stats_out && best, OMNI_ERR_INVALID, "omni_pgo_solve_multi: null argument");
    const char* why = pgo::graph_refusal(edges, n_poses, n_edges);
    if (!why) why = pgo::starts_refusal(n_starts);
    if (!why) why = pgo::params_refusal(*params);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "omni_pgo_solve_multi: %s", why);
    TraceRange trace_range("pgo solve");
    std::lock_guard<std::mutex> lk(p->mu);
    omni_ctx* ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t n = (size_t)n_poses, m = (size_t)n_edges, K = (size_t)n_starts;
    const size_t o_edges = 0, o_poses = up64(o_edges + m * sizeof(omni_pgo_edge)), o_off = up64(o_poses + K * n * 32), o_inc = up64(o_off + (n + 1) * 4),
                 o_act = up64(o_inc + 2 * m * 4), in_bytes = up64(o_act + n);
    const size_t slab = pgo::slab_doubles(n_poses, n_edges), o_stats = up64(K * n * 32), out_bytes = o_stats + K * sizeof(omni_pgo_stats);
    int rc = p->hin.ensure(in_bytes);
    if (!rc) rc = p->hout.ensure(out_bytes);
    if (!rc) rc = p->in.ensure(in_bytes);
    if (!rc) rc = p->out.ensure(out_bytes);
    if (!rc) rc = p->slabs.ensure(K * slab * sizeof(double));
    if (rc) return rc;
    char* h = p->hin.as<char>();
    if (m) memcpy(h + o_edges, edges, m * sizeof(omni_pgo_edge));
    memcpy(h + o_poses, poses_in, K * n * 32);
    pgo::Graph G;
    G.n = n_poses; G.m = n_edges;
    G.n_active = pgo::plan_graph(fixed, edges, n_poses, n_edges, (int32_t*)(h + o_off), (int32_t*)(h + o_inc), (uint8_t*)(h + o_act));
    char* d = p->in.as<char>();
    G.edges = (const omni_pgo_edge*)(d + o_edges); G.offsets = (const int32_t*)(d + o_off); G.incident = (const int32_t*)(d + o_inc); G.active = (const uint8_t*)(d + o_act);
    OMNI_HIP_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (kernel_us) OMNI_HIP_TRY(hipEventRecord(p->e0, ctx->stream));
    char* o = p->out.as<char>();
    hipLaunchKernelGGL(pgo_solve_kernel, dim3((unsigned)n_starts), dim3(pgo::THREADS), 0, ctx->stream, G, *params, (const double*)(d + o_poses), p->slabs.as<double>(), slab,
                       (double*)o, (omni_pgo_stats*)(o + o_stats), n_starts);
    hipError_t err = hipGetLastError();
    if (kernel_us && err == hipSuccess) (void)hipEventRecord(p->e1, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(p->hout.as<char>(), o, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (kernel_us) {
        float ms = 0;
        if (err == hipSuccess && hipEventElapsedTime(&ms, p->e0, p->e1) == hipSuccess) *kernel_us = ms * 1000.f;
    }
    OMNI_HIP_TRY(err);
    memcpy(poses_out, p->hout.as<char>(), K * n * 32);
    memcpy(stats_out, p->hout.as<char>() + o_stats, K * sizeof(omni_pgo_stats));
    *best = pgo::pick_best(stats_out, n_starts);
    return OMNI_OK;
}
