// omni_rows_assemble_enqueue_dev: the rows of a mixed detector batch gathered into one contiguous block (csrc/rows_plan.h has the table, the refusals and the rule
// for the two paths -- this file only spreads a row over lanes):
//   one workgroup per output row, 256 lanes (4 waves); the row's table entry is read once per lane (uniform over the workgroup: a broadcast);
//   16-byte path  lane l moves float4 l, l + 256, ... of the row: consecutive lanes, consecutive 16 bytes (1 KiB per wave and instruction);
//   dword path    the same sweep in floats, for a dim that is no multiple of 4 or a base off the 16-byte grid;
//   a ZERO entry, or one that points outside its block, stores zeros.
// A pure copy at HBM's pace: ONE launch per batch instead of one copy per run of rows.  No atomics, no LDS; no workgroup reads what another wrote; every loop's trip
// count is bounded by dim, a launch argument.  Loads and stores move bits (global_load / global_store): NaN payloads survive.
#include "common.h"
#include "rows_plan.h"

namespace omni {

template <typename V>
__global__ __launch_bounds__(rows::THREADS) void rows_assemble_kernel(int n_rows, int dim, const omni_row_source* __restrict__ table, const float* __restrict__ unit_rows,
                                                                       long long n_unit_rows, const float* __restrict__ staged_rows, long long n_staged_rows,
                                                                       float* __restrict__ out) {
    const int r = blockIdx.x;
    if (r >= n_rows) return;
    const int dim_v = dim / (int)(sizeof(V) / sizeof(float));              // (V = float4: the launcher has checked dim % 4 == 0 and the bases, rows::vec16)
    const V* src = reinterpret_cast<const V*>(rows::source_row(table[r], dim, unit_rows, n_unit_rows, staged_rows, n_staged_rows));
    V* dst = reinterpret_cast<V*>(out + (size_t)r * dim);
    if (src) { for (int i = threadIdx.x; i < dim_v; i += rows::THREADS) dst[i] = src[i]; }
    else { const V zero = {}; for (int i = threadIdx.x; i < dim_v; i += rows::THREADS) dst[i] = zero; }
}

int rows_assemble_launch(hipStream_t stream, int64_t n_rows, int dim, const omni_row_source* table, const float* unit_rows, int64_t n_unit_rows, const float* staged_rows,
                         int64_t n_staged_rows, float* out) {
    if (rows::vec16(dim, unit_rows, staged_rows, out))
        hipLaunchKernelGGL(rows_assemble_kernel<float4>, dim3((unsigned)n_rows), dim3(rows::THREADS), 0, stream, (int)n_rows, dim, table, unit_rows, (long long)n_unit_rows,
                           staged_rows, (long long)n_staged_rows, out);
    else
        hipLaunchKernelGGL(rows_assemble_kernel<float>, dim3((unsigned)n_rows), dim3(rows::THREADS), 0, stream, (int)n_rows, dim, table, unit_rows, (long long)n_unit_rows,
                           staged_rows, (long long)n_staged_rows, out);
    OMNI_LAUNCH_CHECK();
    return OMNI_OK;
}

}  // namespace omni

extern "C" int omni_rows_assemble_enqueue_dev(omni_ctx* ctx, int64_t n_rows, int dim, const omni_row_source* table_dev, const float* unit_rows_dev, int64_t n_unit_rows,
                                              const float* staged_rows_dev, int64_t n_staged_rows, float* out_dev) {
    OMNI_REQUIRE(ctx && table_dev && out_dev, OMNI_ERR_INVALID, "omni_rows_assemble_enqueue_dev: null argument");
    const char* why = omni::rows::refusal(nullptr, n_rows, dim, n_unit_rows, n_staged_rows);
    OMNI_REQUIRE(!why, OMNI_ERR_INVALID, "omni_rows_assemble_enqueue_dev: %s (n_rows %lld, dim %d, unit rows %lld, staged rows %lld)", why, (long long)n_rows, dim,
                 (long long)n_unit_rows, (long long)n_staged_rows);
    OMNI_REQUIRE((unit_rows_dev || n_unit_rows == 0) && (staged_rows_dev || n_staged_rows == 0), OMNI_ERR_INVALID,
                 "omni_rows_assemble_enqueue_dev: a block with rows and no address");
    OMNI_REQUIRE(((uintptr_t)table_dev | (uintptr_t)unit_rows_dev | (uintptr_t)staged_rows_dev | (uintptr_t)out_dev) % 4 == 0, OMNI_ERR_INVALID,
                 "omni_rows_assemble_enqueue_dev: a base that is not 4-byte aligned");
    omni::TraceRange trace_range("detector rows assemble");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    return omni::rows_assemble_launch(ctx->stream, n_rows, dim, table_dev, unit_rows_dev, n_unit_rows, staged_rows_dev, n_staged_rows, out_dev);
}
