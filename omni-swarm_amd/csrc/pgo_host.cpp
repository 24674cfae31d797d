// csrc/pgo_plan.h compiled by g++ into libomni_hip.so: omni_pgo_solve_host gives host callers and the tests the bits of the GPU solve (pgo.hip) without a GPU and
// without a context; omni_pgo_residuals_host, omni_pgo_plan_graph_host, omni_pgo_sincos, omni_pgo_normalize_angle and omni_pgo_sum_host open the header's pieces to
// the tests.
#include "pgo_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}  // namespace omni

extern "C" int omni_pgo_default_params(omni_pgo_params* out) {
    if (!out) { omni::set_error("omni_pgo_default_params: null argument"); return OMNI_ERR_INVALID; }
    *out = omni::pgo::default_params();
    return OMNI_OK;
}

extern "C" int omni_pgo_solve_host(const omni_pgo_params* params, const double* poses_in, const uint8_t* fixed, const omni_pgo_edge* edges, int n_poses, int n_edges,
                                   int n_starts, double* poses_out, omni_pgo_stats* stats_out, int* best) {
    if (!params || !poses_in || !fixed || (!edges && n_edges > 0) || !poses_out || !stats_out || !best) { omni::set_error("omni_pgo_solve_host: null argument"); return OMNI_ERR_INVALID; }
    const char* why = omni::pgo::solve_host(*params, poses_in, fixed, edges, n_poses, n_edges, n_starts, poses_out, stats_out, best);
    if (why) { omni::set_error("omni_pgo_solve_host: %s", why); return OMNI_ERR_INVALID; }
    return OMNI_OK;
}

extern "C" int omni_pgo_residuals_host(const double* poses, const omni_pgo_edge* edges, int n_poses, int n_edges, double* res_out, double* jac_i_out, double* jac_j_out,
                                       double* cost_out) {
    using namespace omni::pgo;
    if (!poses || (!edges && n_edges > 0)) { omni::set_error("omni_pgo_residuals_host: null argument"); return OMNI_ERR_INVALID; }
    const char* why = graph_refusal(edges, n_poses, n_edges);
    if (why) { omni::set_error("omni_pgo_residuals_host: %s", why); return OMNI_ERR_INVALID; }
    for (int e = 0; e < n_edges; ++e) {
        EdgeLin l;
        const double cost = linearize(edges[e], poses, &l);
        if (res_out) for (int q = 0; q < 4; ++q) res_out[(size_t)4 * e + q] = l.r[q];
        if (jac_i_out) jacobian(l, 0, jac_i_out + (size_t)16 * e);
        if (jac_j_out) jacobian(l, 1, jac_j_out + (size_t)16 * e);
        if (cost_out) cost_out[e] = cost;
    }
    return OMNI_OK;
}

extern "C" int omni_pgo_plan_graph_host(const uint8_t* fixed, const omni_pgo_edge* edges, int n_poses, int n_edges, int32_t* offsets_out, int32_t* incident_out,
                                        uint8_t* active_out, int* n_active_out) {
    using namespace omni::pgo;
    if (!fixed || (!edges && n_edges > 0) || !offsets_out || (!incident_out && n_edges > 0) || !active_out || !n_active_out) {
        omni::set_error("omni_pgo_plan_graph_host: null argument");
        return OMNI_ERR_INVALID;
    }
    const char* why = graph_refusal(edges, n_poses, n_edges);
    if (why) { omni::set_error("omni_pgo_plan_graph_host: %s", why); return OMNI_ERR_INVALID; }
    *n_active_out = plan_graph(fixed, edges, n_poses, n_edges, offsets_out, incident_out, active_out);
    return OMNI_OK;
}

extern "C" void omni_pgo_sincos(double yaw, double* sin_out, double* cos_out) { omni::pgo::sincos_plan(yaw, sin_out, cos_out); }
extern "C" double omni_pgo_normalize_angle(double a) { return omni::pgo::normalize_angle(a); }
extern "C" double omni_pgo_sum_host(const double* v, int n) {
    std::vector<double> red((size_t)omni::pgo::kRedDoubles);
    omni::pgo::HostTeam team;
    team.red = red.data();
    return omni::pgo::reduce(team, n, [&](int k) { return v[k]; });
}
