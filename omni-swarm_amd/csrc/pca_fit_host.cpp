// pca_plan.h for host callers: plain g++, no HIP header, no GPU, no context (omni_pca_moments_host, omni_pca_solve_host, omni_pca_write_csv)
#include <new>
#include <vector>

#include "../../include/omni_hip.h"
#include "pca_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}

extern "C" {

int omni_pca_moments_host(const float* raw_desc, const float* norm_partial, const int* n_kps, int batch, int max_num, int64_t* n, int64_t* skipped, double* s256,
                          double* S_full) {
    if (!raw_desc || !norm_partial || !n_kps || !n || !skipped || !s256 || !S_full) { omni::set_error("null argument"); return OMNI_ERR_INVALID; }
    if (batch < 1 || max_num < 1 || max_num > 1024) { omni::set_error("batch=%d (>= 1) / max_num=%d (1..1024) out of range", batch, max_num); return OMNI_ERR_INVALID; }
    if (*n < 0 || *skipped < 0) { omni::set_error("negative count (n %lld, skipped %lld)", (long long)*n, (long long)*skipped); return OMNI_ERR_INVALID; }
    omni::pca::Moments m;
    m.n = *n; m.skipped = *skipped; m.s = s256; m.S = S_full;
    omni::pca::moments_host(m, raw_desc, norm_partial, n_kps, batch, max_num);
    omni::pca::mirror(S_full);
    *n = m.n; *skipped = m.skipped;
    return OMNI_OK;
}

int omni_pca_solve_host(int64_t n, const double* s256, const double* S_full, int pca_dim, double* components, float* components_f32, double* mean, float* mean_f32,
                        double* explained_variance, double* total_variance) {
    if (!s256 || !S_full) { omni::set_error("null argument"); return OMNI_ERR_INVALID; }
    const int why = omni::pca::check_solve(n, pca_dim);
    if (why) { omni::set_error("%s (n %lld, pca_dim %d)", omni::pca::refusal_text(why), (long long)n, pca_dim); return OMNI_ERR_INVALID; }
    std::vector<double> work;
    std::vector<int> order;
    try { work.resize((size_t)omni::pca::kSolveWorkDoubles); order.resize(omni::pca::kDim); }
    catch (const std::bad_alloc&) { omni::set_error("out of host memory for the PCA solve"); return OMNI_ERR_NOMEM; }
    omni::pca::solve(n, s256, S_full, pca_dim, work.data(), order.data(), components, components_f32, mean, mean_f32, explained_variance, total_variance);
    return OMNI_OK;
}

int omni_pca_write_csv(const char* comp_path, const char* mean_path, const float* components_f32, const float* mean_f32, int pca_dim) {
    if (!comp_path || !mean_path || !components_f32 || !mean_f32) { omni::set_error("null argument"); return OMNI_ERR_INVALID; }
    if (pca_dim < 1 || pca_dim > omni::pca::kDim) { omni::set_error("%s (pca_dim %d)", omni::pca::refusal_text(omni::pca::SOLVE_BAD_DIM), pca_dim); return OMNI_ERR_INVALID; }
    if (!omni::pca::write_csv(comp_path, mean_path, components_f32, mean_f32, pca_dim)) { omni::set_error("cannot write %s / %s", comp_path, mean_path); return OMNI_ERR_INVALID; }
    return OMNI_OK;
}

}  // extern "C"
