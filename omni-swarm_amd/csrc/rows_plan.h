// Where the rows of a mixed detector batch come from, stated ONCE: LoopDetectorCore's batch (host/omni_swarm.hpp) wants one contiguous [n_rows][dim] fp32 block in
// frame order whose rows lie in three places -- a key-frame unit's MobileNetVLAD output in HBM (UNIT), the global descriptors of frames other drones sent, staged on
// the host and uploaded with the table (STAGED), and nothing at all for an image without a descriptor (ZERO).  The plan is the table of (source, index) per output
// row, what is refused, and which of the kernel's two paths a call takes.  rows_assemble.hip only spreads a row over lanes; rows_assemble_host.cpp is this header
// under g++ (omni_rows_assemble_host: the kernel's stand-in).  Plain host C++, no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define ROWS_HD __host__ __device__ inline
#else
#define ROWS_HD inline
#endif

namespace omni {
namespace rows {

constexpr int THREADS = 256;                         // rows_assemble_kernel: one workgroup per output row

// What both entries refuse before they touch anything; NULL when the call may go ahead.  table == nullptr: the table lives in device memory, its maker has checked
// it with this function before the upload (the kernel itself writes zeros for an entry it cannot serve, and never reads outside the two blocks)
inline const char* refusal(const omni_row_source* table, int64_t n_rows, int dim, int64_t n_unit_rows, int64_t n_staged_rows) {
    if (n_rows < 1) return "n_rows < 1";
    if (n_rows > 0x7fffffff) return "more than 2^31 - 1 rows";
    if (dim < 1) return "dim < 1";
    if (n_unit_rows < 0 || n_staged_rows < 0) return "a negative row count";
    if (!table) return nullptr;
    for (int64_t r = 0; r < n_rows; ++r) {
        const omni_row_source& e = table[r];
        if (e.source == OMNI_ROW_ZERO) continue;
        if (e.source != OMNI_ROW_UNIT && e.source != OMNI_ROW_STAGED) return "an unknown row source";
        if (e.index < 0 || e.index >= (e.source == OMNI_ROW_UNIT ? n_unit_rows : n_staged_rows)) return "a row index out of range";
    }
    return nullptr;
}

// The 16-byte path: every row of all three blocks starts on a 16-byte boundary -- dim a multiple of 4 floats and the three bases aligned (a block that is not
// there counts as aligned).  Everything else moves dwords.
inline bool vec16(int dim, const void* unit_rows, const void* staged_rows, const void* out) {
    return dim % 4 == 0 && ((uintptr_t)unit_rows | (uintptr_t)staged_rows | (uintptr_t)out) % 16 == 0;
}

// where output row r reads (nullptr: zeros): what the kernel's lanes and the host loop both ask.  An entry the refusal would have named reads nothing
ROWS_HD const float* source_row(const omni_row_source e, int dim, const float* unit_rows, int64_t n_unit_rows, const float* staged_rows, int64_t n_staged_rows) {
    if (e.source == OMNI_ROW_UNIT && e.index >= 0 && e.index < n_unit_rows) return unit_rows + (size_t)e.index * dim;
    if (e.source == OMNI_ROW_STAGED && e.index >= 0 && e.index < n_staged_rows) return staged_rows + (size_t)e.index * dim;
    return nullptr;
}

// the whole assembly on the host, bit for bit (memcpy: NaN payloads survive)
inline void assemble_host(const omni_row_source* table, int64_t n_rows, int dim, const float* unit_rows, int64_t n_unit_rows, const float* staged_rows, int64_t n_staged_rows,
                          float* out) {
    for (int64_t r = 0; r < n_rows; ++r) {
        const float* src = source_row(table[r], dim, unit_rows, n_unit_rows, staged_rows, n_staged_rows);
        if (src) std::memcpy(out + (size_t)r * dim, src, (size_t)dim * 4);
        else std::memset(out + (size_t)r * dim, 0, (size_t)dim * 4);
    }
}

// The one block a caller uploads per batch: the table in front (padded to 256 bytes, so the staged rows behind it start aligned), then the staged rows
inline size_t table_bytes(int64_t n_rows) { return ((size_t)n_rows * sizeof(omni_row_source) + 255) / 256 * 256; }
inline size_t upload_bytes(int64_t n_rows, int dim, int64_t n_staged_rows) { return table_bytes(n_rows) + (size_t)n_staged_rows * dim * 4; }
inline size_t out_offset(int64_t n_rows, int dim, int64_t n_staged_rows) { return (upload_bytes(n_rows, dim, n_staged_rows) + 255) / 256 * 256; }
inline size_t device_bytes(int64_t n_rows, int dim, int64_t n_staged_rows) { return out_offset(n_rows, dim, n_staged_rows) + (size_t)n_rows * dim * 4; }

}  // namespace rows
}  // namespace omni
