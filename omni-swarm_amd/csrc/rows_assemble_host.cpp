// csrc/rows_plan.h compiled by g++ into libomni_hip.so: omni_rows_assemble_host gives host callers and the tests the bits of the GPU stage (rows_assemble.hip)
// without a GPU and without a context.
#include "rows_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}  // namespace omni

extern "C" int omni_rows_assemble_host(int64_t n_rows, int dim, const omni_row_source* table, const float* unit_rows, int64_t n_unit_rows, const float* staged_rows,
                                       int64_t n_staged_rows, float* out) {
    if (!table || !out) {
        omni::set_error("omni_rows_assemble_host: null argument");
        return OMNI_ERR_INVALID;
    }
    if (const char* why = omni::rows::refusal(table, n_rows, dim, n_unit_rows, n_staged_rows)) {
        omni::set_error("omni_rows_assemble_host: %s (n_rows %lld, dim %d, unit rows %lld, staged rows %lld)", why, (long long)n_rows, dim, (long long)n_unit_rows,
                        (long long)n_staged_rows);
        return OMNI_ERR_INVALID;
    }
    if ((!unit_rows && n_unit_rows > 0) || (!staged_rows && n_staged_rows > 0)) {
        omni::set_error("omni_rows_assemble_host: a block with rows and no address");
        return OMNI_ERR_INVALID;
    }
    omni::rows::assemble_host(table, n_rows, dim, unit_rows, n_unit_rows, staged_rows, n_staged_rows, out);
    return OMNI_OK;
}
