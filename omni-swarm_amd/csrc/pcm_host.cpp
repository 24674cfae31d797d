// csrc/pcm_plan.h compiled by g++ into libomni_hip.so: omni_pcm_rows_host gives host callers and the tests the bits of the GPU rows (pcm.hip) without a GPU and
// without a context; omni_pcm_max_clique_host is the clique heuristic, which runs on the host only; omni_pcm_atan2 is the header's arctangent for the tests.
#include <vector>

#include "pcm_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}  // namespace omni

extern "C" int omni_pcm_rows_host(const omni_pcm_edge* edges, int n_total, int first, const omni_pcm_params* params, int stride_words, uint64_t* rows_out,
                                  int32_t* degree_add, double* smd_out) {
    if (!edges || !params || !rows_out || !degree_add) { omni::set_error("omni_pcm_rows_host: null argument"); return OMNI_ERR_INVALID; }
    if (n_total < 1 || first < 0 || first >= n_total || stride_words < 1 || (int64_t)stride_words * 64 < n_total) {
        omni::set_error("omni_pcm_rows_host: n_total %d, first %d, stride_words %d", n_total, first, stride_words);
        return OMNI_ERR_INVALID;
    }
    omni::pcm::rows_host(edges, n_total, first, *params, stride_words, rows_out, degree_add, smd_out);
    return OMNI_OK;
}

extern "C" int omni_pcm_max_clique_host(const uint64_t* rows, int n, int stride_words, int32_t* clique_out, int* size_out) {
    if (!rows || !clique_out || !size_out) { omni::set_error("omni_pcm_max_clique_host: null argument"); return OMNI_ERR_INVALID; }
    if (n < 0 || stride_words < 1 || (int64_t)stride_words * 64 < n) { omni::set_error("omni_pcm_max_clique_host: n %d, stride_words %d", n, stride_words); return OMNI_ERR_INVALID; }
    std::vector<int32_t> deg((size_t)n + 1), cur((size_t)n + 1);
    std::vector<uint64_t> work((size_t)2 * stride_words);
    *size_out = omni::pcm::max_clique(rows, n, stride_words, deg.data(), work.data(), clique_out, cur.data());
    return OMNI_OK;
}

extern "C" double omni_pcm_atan2(double y, double x) { return omni::pcm::atan2_plan(y, x); }
