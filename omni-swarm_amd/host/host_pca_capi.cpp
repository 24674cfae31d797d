// host_pca_capi.cpp -> lib/libomni_host_pca.so: the C entry points of KeyframePipeline::Config::fit_pca (keyframe_pipeline.hpp).
// A library of its own next to libomni_host.so, whose set of entry points is fixed; the handle is the same (host_capi_types.hpp).
#include <algorithm>
#include <string>

#include "host_capi_types.hpp"
#include "omni_host_pca.h"      // include/: the declarations of everything below (a mismatch is a compile error)

namespace {
thread_local std::string g_err;

template <class F> int guarded(omni_pipeline* h, const char* what, F&& f) {
    try {
        if (!h) throw std::invalid_argument(std::string(what) + ": null pipeline");
        f(*h->p);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}
}  // namespace

extern "C" {

const char* omni_pca_host_last_error(void) { return g_err.c_str(); }

int omni_pipeline_set_fit_pca(omni_pipeline* h, int on) {
    return guarded(h, "omni_pipeline_set_fit_pca", [&](omni::KeyframePipeline& p) { p.set_fit_pca(on != 0); });
}

int omni_pipeline_get_fit_pca(omni_pipeline* h, int* on) {
    return guarded(h, "omni_pipeline_get_fit_pca", [&](omni::KeyframePipeline& p) {
        if (!on) throw std::invalid_argument("omni_pipeline_get_fit_pca: null argument");
        *on = p.fit_pca() ? 1 : 0;
    });
}

int omni_pipeline_pca_fit_stats(omni_pipeline* h, int64_t* n, int64_t* skipped) {
    return guarded(h, "omni_pipeline_pca_fit_stats", [&](omni::KeyframePipeline& p) {
        const omni::PcaMoments m = p.pca_fit_moments();
        if (n) *n = m.n;
        if (skipped) *skipped = m.skipped;
    });
}

int omni_pipeline_pca_fit_moments(omni_pipeline* h, int64_t* n, int64_t* skipped, double* s256, double* S_full) {
    return guarded(h, "omni_pipeline_pca_fit_moments", [&](omni::KeyframePipeline& p) {
        const omni::PcaMoments m = p.pca_fit_moments();
        if (n) *n = m.n;
        if (skipped) *skipped = m.skipped;
        if (s256) std::copy(m.s.begin(), m.s.end(), s256);
        if (S_full) std::copy(m.S.begin(), m.S.end(), S_full);
    });
}

int omni_pipeline_pca_fit_solve(omni_pipeline* h, int pca_dim, double* components, float* components_f32, double* mean, float* mean_f32, double* explained_variance,
                                double* total_variance) {
    return guarded(h, "omni_pipeline_pca_fit_solve", [&](omni::KeyframePipeline& p) {
        const omni::PcaSolution o = p.pca_fit(pca_dim);
        if (components) std::copy(o.components.begin(), o.components.end(), components);
        if (components_f32) std::copy(o.components_f32.begin(), o.components_f32.end(), components_f32);
        if (mean) std::copy(o.mean.begin(), o.mean.end(), mean);
        if (mean_f32) std::copy(o.mean_f32.begin(), o.mean_f32.end(), mean_f32);
        if (explained_variance) std::copy(o.explained_variance.begin(), o.explained_variance.end(), explained_variance);
        if (total_variance) *total_variance = o.total_variance;
    });
}

int omni_pipeline_pca_fit_write(omni_pipeline* h, const char* comp_path, const char* mean_path, int pca_dim) {
    return guarded(h, "omni_pipeline_pca_fit_write", [&](omni::KeyframePipeline& p) {
        if (!comp_path || !mean_path) throw std::invalid_argument("omni_pipeline_pca_fit_write: null path");
        p.pca_fit_write(comp_path, mean_path, pca_dim);
    });
}

int omni_pipeline_pca_fit_reset(omni_pipeline* h) {
    return guarded(h, "omni_pipeline_pca_fit_reset", [&](omni::KeyframePipeline& p) { p.pca_fit_reset(); });
}

}  // extern "C"
