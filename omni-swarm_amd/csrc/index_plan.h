// How the loop-closure index (index.hip) answers a search, decided ONCE per search by a pure function of what the handle is (IndexFacts) and of the search
// itself (queries, k, rows): which path, how many candidates, how large the key buffers, which scan kernel covers which queries with which grid -- and how
// the row buffers grow.  This header is the one statement of those rules: index.hip only switches over the plan.  Plain host C++, no HIP:
// tests/cpp/index_plan_pin.cpp compiles it under g++ and tests/test_index_plan_cpu.py compares every combination against an independent restatement.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/omni_hip.h"
#include "topk_sizes.h"

namespace omni {

// ---- sizes (the kernels and the plan read the same constants) ----
constexpr int SCAN_THREADS = 256;                                  // ip_scan_kernel, ip_scan_rows_kernel, ip_scan_t16_kernel
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SCAN_MAX_QB = 8;                                     // queries of one pass of those kernels
constexpr int SCAN_ROWS_R = 4;                                     // ip_scan_rows_kernel: rows a wave walks at once
constexpr int SCAN_ROWS_MIN_QB = 4;                                // ... and the smallest query block it is compiled for
constexpr int INDEX_QUERY_LDS_BYTES = 131072;                      // the query block lives in LDS: <= 128 KB of it
constexpr int MQ_THREADS = 512;                                    // ip_scan_mq_kernel
constexpr int MQ_WAVES = 8;
constexpr int MQ_RT = 4;                                           // 16-row tiles per wave
constexpr int MQ_NQ = 64;                                          // queries of one pass
constexpr int MQ_KS = 256;                                         // k per query slice
constexpr int MQ_SLICE_BYTES = 2 * MQ_NQ * MQ_KS * 2;              // [hi|lo][64 q][256 k] halfs
constexpr int MQ_SMEM = 2 * MQ_SLICE_BYTES;                        // two slices: one feeds the MFMAs, the next streams in

// Everything a search's path depends on besides the search itself
struct IndexFacts {
    int dim = 0;
    int storage = OMNI_STORE_F32;
    bool has_mirror = false;             // an fp32 shard that holds the fp16 mirror of its rows
    int n_cu = 256;                      // index_n_cu(the device's compute units)
    int mq_min = 1 << 30;                // index_mq_min(OMNI_MQ_MIN): queries from which a search runs on the matrix cores
    int rows_min_qb = 4;                 // OMNI_SCAN_ROWS_MIN: fp32 rows, query block from which ip_scan_rows_kernel scans
    int64_t mirror_min_rows = 32768;     // OMNI_INDEX_MIRROR_MIN_ROWS: smaller databases stay on the exact kernels (their scans are launch-bound: the mirror's
                                         // extra launches and its host check would cost more than the halved HBM traffic saves)
};
inline int index_n_cu(int multi_processor_count) { return multi_processor_count > 0 ? multi_processor_count : 256; }
inline int index_mq_min(int omni_mq_min) { return omni_mq_min <= 0 ? (1 << 30) : omni_mq_min; }      // 0 = never, 1 = always

inline int64_t index_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// queries per pass of the VALU scans
inline int index_query_block(int dim) {
    const int qb = (int)((size_t)INDEX_QUERY_LDS_BYTES / ((size_t)dim * 4));
    return qb > SCAN_MAX_QB ? SCAN_MAX_QB : (qb < 1 ? 1 : qb);
}

enum IndexScanForm {
    INDEX_SCAN_F32_ONE = 0,              // ip_scan_kernel<float, QB>: fp32 rows, a wave walks one row at a time
    INDEX_SCAN_F32_ROWS,                 // ip_scan_rows_kernel<QB, SCAN_ROWS_R>: fp32 rows, QB >= 4
    INDEX_SCAN_T16,                      // ip_scan_t16_kernel<QB>: fp16 rows on the VALU
    INDEX_SCAN_MQ,                       // ip_scan_mq_kernel: fp16 rows (a shard's own or an fp32 shard's mirror), <= MQ_NQ queries on the matrix cores
};

// the kernel of a pass of qb queries that does not run on the matrix cores
inline IndexScanForm index_scan_form(const IndexFacts& f, int qb) {
    if (f.storage == OMNI_STORE_F16) return INDEX_SCAN_T16;
    return qb >= SCAN_ROWS_MIN_QB && qb >= f.rows_min_qb ? INDEX_SCAN_F32_ROWS : INDEX_SCAN_F32_ONE;
}

struct IndexScanLaunch { int grid = 1, threads = 0; size_t smem_bytes = 0; };

// A VALU scan's waves walk rows (fp32), groups of SCAN_ROWS_R rows or 16-row blocks (fp16), at most 8 workgroups per compute unit; the matrix-core scan is one
// workgroup per compute unit (128 KB of LDS each) walking 512-row blocks b, b + grid, ...  (n >= 1)
inline IndexScanLaunch index_scan_launch(const IndexFacts& f, IndexScanForm form, int64_t n, int qb) {
    IndexScanLaunch l;
    if (form == INDEX_SCAN_MQ) {
        const int64_t blocks = index_cdiv(index_cdiv(n, 16), MQ_WAVES * MQ_RT);
        l.grid = (int)(blocks < f.n_cu ? blocks : f.n_cu);
        l.threads = MQ_THREADS;
        l.smem_bytes = MQ_SMEM;
        return l;
    }
    const int64_t units = form == INDEX_SCAN_T16 ? index_cdiv(n, 16) : form == INDEX_SCAN_F32_ROWS ? index_cdiv(n, SCAN_ROWS_R) : n;
    const int64_t want = index_cdiv(units, SCAN_WAVES), cap = (int64_t)f.n_cu * 8;
    l.grid = (int)(want < cap ? want : cap);
    if (l.grid < 1) l.grid = 1;
    l.threads = SCAN_THREADS;
    l.smem_bytes = (size_t)qb * f.dim * sizeof(float);
    return l;
}
// the matrix-core scan's query buffer: the <= MQ_NQ queries as fp16 hi + lo, one slice per MQ_KS k
inline size_t index_mq_query_bytes(int dim) { return (size_t)(dim / MQ_KS) * MQ_SLICE_BYTES; }

// The scan passes of `nq` queries in launch order: pass i covers queries [q0, q0 + qb), `width` of them but for the last pass
struct IndexScanPass { int q0 = 0, qb = 0; IndexScanForm form = INDEX_SCAN_F32_ONE; };
struct IndexScanPasses {
    int nq = 0, width = 1;
    bool mq = false;                     // every pass on the matrix cores; otherwise a pass's kernel follows from its own qb
    IndexFacts facts;
    int count() const { return (int)index_cdiv(nq, width); }
    IndexScanPass pass(int i) const {
        IndexScanPass p;
        p.q0 = i * width;
        p.qb = nq - p.q0 < width ? nq - p.q0 : width;
        p.form = mq ? INDEX_SCAN_MQ : index_scan_form(facts, p.qb);
        return p;
    }
};
inline IndexScanPasses index_scan_passes(const IndexFacts& f, bool mq, int nq) {
    IndexScanPasses p;
    p.nq = nq; p.width = mq ? MQ_NQ : index_query_block(f.dim); p.mq = mq; p.facts = f;
    return p;
}

enum IndexSearchPath {
    INDEX_PATH_MIRROR_CERT = 0,          // fp32 shard with a mirror, a batch: ONE matrix-core pass over the mirror, kp candidates per query re-scored exactly, a
                                         // certificate per query; the uncertified queries again through the exact passes (fallback_passes)
    INDEX_PATH_MQ_F16,                   // fp16 shard, a batch: matrix-core passes of <= MQ_NQ queries
    INDEX_PATH_EXACT_SCAN,               // VALU passes of <= index_query_block queries over the shard's own rows
};

struct IndexSearchPlan {
    IndexSearchPath path = INDEX_PATH_EXACT_SCAN;
    int kp = 0;                          // candidates per query of the mirror pass
    int64_t key_elems_per_query = 0;     // keys_a / keys_b hold a scan's n keys per query and every level of the top-k
    size_t keys_bytes = 0;               // each of keys_a, keys_b
    size_t cert_keys_bytes = 0, cert_flags_bytes = 0, hflags_bytes = 0;      // INDEX_PATH_MIRROR_CERT only
    IndexScanPasses passes;              // none over an empty index (n == 0): the top-k and the decode still run, over nothing
    IndexScanPasses fallback_passes(int nfl) const { return index_scan_passes(passes.facts, false, nfl); }       // nfl uncertified queries, staged back to back
};

// nq queries, the best k of rows [0, n)
inline IndexSearchPlan index_search_plan(const IndexFacts& f, int nq, int k, int64_t n) {
    IndexSearchPlan p;
    p.kp = k + 24 > 2 * k ? k + 24 : 2 * k;
    const int64_t chunks = index_cdiv(n > 0 ? n : 1, TOPK_CHUNK);
    p.key_elems_per_query = n > chunks * k ? n : chunks * k;
    p.keys_bytes = (size_t)nq * p.key_elems_per_query * 8;
    const bool batch = nq >= f.mq_min;
    if (n > 0 && n >= f.mirror_min_rows && f.storage == OMNI_STORE_F32 && f.has_mirror && batch && nq <= MQ_NQ && p.kp <= TOPK_SEL_MAX_K) {
        p.path = INDEX_PATH_MIRROR_CERT;
        p.cert_keys_bytes = (size_t)nq * p.kp * 8;
        p.cert_flags_bytes = p.hflags_bytes = (size_t)MQ_NQ * 4;
    } else if (n > 0 && f.storage == OMNI_STORE_F16 && batch) {
        p.path = INDEX_PATH_MQ_F16;
    }
    p.passes = index_scan_passes(f, p.path != INDEX_PATH_EXACT_SCAN, n > 0 ? nq : 0);
    return p;
}

// ---- the row buffers ----
// growth: 1024 rows at first, doubling, whole 16-row blocks (fp16 T16 layout)
inline int64_t index_grown_capacity(int64_t capacity, int64_t rows) {
    if (rows <= capacity) return capacity;
    int64_t cap = capacity > 0 ? capacity : 1024;
    while (cap < rows) cap *= 2;
    return (cap + 15) & ~(int64_t)15;
}
// a snapshot's rows: exactly as many whole blocks as it holds (one block for none)
inline int64_t index_loaded_capacity(int64_t ntotal) { return ((ntotal > 0 ? ntotal : 1) + 15) & ~(int64_t)15; }

}  // namespace omni
