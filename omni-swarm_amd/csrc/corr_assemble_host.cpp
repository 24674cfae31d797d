// csrc/corr_plan.h compiled by g++ into libomni_hip.so: omni_corr_assemble_host gives host callers and the tests the bits of the GPU stage (corr_assemble.hip)
// without a GPU and without a context.
#include "corr_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}  // namespace omni

extern "C" int omni_corr_assemble_host(const omni_corr_io* io) {
    if (!io || !io->cands || !io->n_corr || !io->matched_dir_count || !io->gate || !io->X || !io->u) {
        omni::set_error("omni_corr_assemble_host: null argument");
        return OMNI_ERR_INVALID;
    }
    if (const char* why = omni::corr::refusal(io->n_cands, io->n_pairs, io->max_n, io->cap, io->cands)) {
        omni::set_error("omni_corr_assemble_host: %s (n_cands %d, n_pairs %d, max_n %d, cap %d)", why, io->n_cands, io->n_pairs, io->max_n, io->cap);
        return OMNI_ERR_INVALID;
    }
    if (io->n_pairs > 0 && (!io->q_idx || !io->t_idx || !io->n_matches || !io->q_flags || !io->n_flags || !io->nq || !io->nt || !io->mask || !io->hg_status || !io->q_3d ||
                            !io->t_norm || !io->dq_old || !io->new_idx || !io->old_idx || !io->n_pair_corr)) {
        omni::set_error("omni_corr_assemble_host: pairs and no arrays");
        return OMNI_ERR_INVALID;
    }
    omni::corr::assemble_host(*io);
    return OMNI_OK;
}
