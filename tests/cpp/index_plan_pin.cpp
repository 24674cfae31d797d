// The plan of an index search (omni-swarm_amd/csrc/index_plan.h) on the host, for tests/test_index_plan_cpu.py.
//   index_plan_pin plans OUT
//     every combination of storage {f32, f16} x has_mirror x dim x nq x k x n x mq_min x rows_min_qb x mirror_min_rows x n_cu (the lists below, the first
//     slowest) as one PlanRow each in the file OUT: those ten inputs, the plan's fields, and of its pass list the number of passes, the sums of q0 and qb, the
//     passes per kernel, the first pass's kernel and grid and the whole last pass with its launch
//   index_plan_pin passes
//     per dim x on the matrix cores {0, 1} x rows_min_qb {4, 9} x nq, for an fp32 shard (fp16 where on the matrix cores): "dim mq rows_min nq count" and per
//     pass " q0 qb form"; then per dim x nfl = 1 .. 64 the same for fallback_passes(nfl) of a mirror search's plan, mq printed as 2
//   index_plan_pin launch
//     per form x dim x n_cu x n >= 1 x qb 1 .. 8: "form dim n_cu n qb grid threads smem_bytes"; per dim "mqbytes dim bytes"
//   index_plan_pin forms       per storage x rows_min_qb {1, 4, 5, 9} x qb 1 .. 8: "storage rows_min qb form"
//   index_plan_pin qblock      per dim 512, 1024 .. 8192 and 16384, 32768, 65536: "dim index_query_block"
//   index_plan_pin capacity    per capacity x rows: "capacity rows grown"; per ntotal: "loaded ntotal capacity"
//   index_plan_pin sizes       the constants, "NAME value"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../omni-swarm_amd/csrc/index_plan.h"

using namespace omni;

static const int kDims[] = {512, 1024, 4096, 8192};
static const int kNq[] = {1, 2, 3, 4, 5, 7, 8, 9, 17, 33, 64, 65, 130, 4096};
static const int kK[] = {1, 5, 32, 33, 40, 64, 65, 1024};
static const int64_t kN[] = {0, 1, 15, 16, 17, 2047, 2048, 2049, 32767, 32768, 100000, 125000, 400000};
static const int kMqMin[] = {0, 1, 4};                            // OMNI_MQ_MIN as set: never, always, the default
static const int kRowsMin[] = {4, 5, 9};                          // OMNI_SCAN_ROWS_MIN: the default (4), 5, 9
static const int64_t kMirrorMin[] = {0, 32768};
static const int kCu[] = {8, 256};

struct PlanRow {
    int64_t per_q, keys_bytes, cert_keys_bytes, n, mirror_min, sum_q0;
    int32_t storage, mirror, dim, nq, k, mq_min, rows_min, n_cu;
    int32_t path, kp, cert_flags_bytes, hflags_bytes, count, width, mq, sum_qb, nform[4], first_form, first_grid, last_q0, last_qb, last_form, last_grid,
        last_threads, last_smem;
};

static int plans(const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) return 1;
    std::vector<PlanRow> rows;
    for (int storage : {OMNI_STORE_F32, OMNI_STORE_F16})
    for (int mirror = 0; mirror < 2; ++mirror)
    for (int dim : kDims) {
        rows.clear();
        for (int nq : kNq) for (int k : kK) for (int64_t n : kN) for (int mq_min : kMqMin) for (int rows_min : kRowsMin) for (int64_t mirror_min : kMirrorMin) for (int n_cu : kCu) {
            IndexFacts fa;
            fa.dim = dim; fa.storage = storage; fa.has_mirror = mirror != 0; fa.n_cu = index_n_cu(n_cu); fa.mq_min = index_mq_min(mq_min); fa.rows_min_qb = rows_min;
            fa.mirror_min_rows = mirror_min;
            const IndexSearchPlan p = index_search_plan(fa, nq, k, n);
            PlanRow r;
            memset(&r, 0, sizeof(r));
            r.storage = storage; r.mirror = mirror; r.dim = dim; r.nq = nq; r.k = k; r.n = n; r.mq_min = mq_min; r.rows_min = rows_min; r.mirror_min = mirror_min; r.n_cu = n_cu;
            r.path = p.path; r.kp = p.kp; r.per_q = p.key_elems_per_query; r.keys_bytes = (int64_t)p.keys_bytes; r.cert_keys_bytes = (int64_t)p.cert_keys_bytes;
            r.cert_flags_bytes = (int32_t)p.cert_flags_bytes; r.hflags_bytes = (int32_t)p.hflags_bytes;
            r.count = p.passes.count(); r.width = p.passes.width; r.mq = p.passes.mq;
            for (int i = 0; i < r.count; ++i) {
                const IndexScanPass s = p.passes.pass(i);
                r.sum_q0 += s.q0; r.sum_qb += s.qb; r.nform[s.form]++;
                if (i == 0 || i == r.count - 1) {
                    const IndexScanLaunch l = index_scan_launch(fa, s.form, n, s.qb);
                    if (i == 0) { r.first_form = s.form; r.first_grid = l.grid; }
                    r.last_q0 = s.q0; r.last_qb = s.qb; r.last_form = s.form; r.last_grid = l.grid; r.last_threads = l.threads; r.last_smem = (int32_t)l.smem_bytes;
                }
            }
            rows.push_back(r);
        }
        if (fwrite(rows.data(), sizeof(PlanRow), rows.size(), f) != rows.size()) return 1;
    }
    return fclose(f) != 0;
}

static void print_passes(const IndexScanPasses& p, int dim, int mq, int rows_min) {
    printf("%d %d %d %d %d", dim, mq, rows_min, p.nq, p.count());
    for (int i = 0; i < p.count(); ++i) { const IndexScanPass s = p.pass(i); printf(" %d %d %d", s.q0, s.qb, (int)s.form); }
    printf("\n");
}

int main(int argc, char** argv) {
    const char* mode = argc >= 2 ? argv[1] : "";
    if (!strcmp(mode, "plans") && argc == 3) return plans(argv[2]);
    if (!strcmp(mode, "passes")) {
        for (int dim : kDims) for (int mq = 0; mq < 2; ++mq) for (int rows_min : {4, 9}) for (int nq : kNq) {
            IndexFacts fa;
            fa.dim = dim; fa.storage = mq ? OMNI_STORE_F16 : OMNI_STORE_F32; fa.rows_min_qb = rows_min;
            print_passes(index_scan_passes(fa, mq != 0, nq), dim, mq, rows_min);
        }
        for (int dim : kDims) for (int nfl = 1; nfl <= MQ_NQ; ++nfl) {
            IndexFacts fa;
            fa.dim = dim; fa.has_mirror = true; fa.mq_min = 4; fa.mirror_min_rows = 0;
            const IndexSearchPlan p = index_search_plan(fa, MQ_NQ, 5, 100000);
            if (p.path != INDEX_PATH_MIRROR_CERT) return 1;
            print_passes(p.fallback_passes(nfl), dim, 2, fa.rows_min_qb);
        }
        return 0;
    }
    if (!strcmp(mode, "launch")) {
        for (int form = 0; form < 4; ++form) for (int dim : kDims) for (int n_cu : kCu) for (int64_t n : kN) for (int qb = 1; n >= 1 && qb <= SCAN_MAX_QB; ++qb) {
            IndexFacts fa;
            fa.dim = dim; fa.n_cu = n_cu;
            const IndexScanLaunch l = index_scan_launch(fa, (IndexScanForm)form, n, qb);
            printf("%d %d %d %lld %d %d %d %zu\n", form, dim, n_cu, (long long)n, qb, l.grid, l.threads, l.smem_bytes);
        }
        for (int dim : kDims) printf("mqbytes %d %zu\n", dim, index_mq_query_bytes(dim));
        return 0;
    }
    if (!strcmp(mode, "forms")) {
        for (int storage : {OMNI_STORE_F32, OMNI_STORE_F16}) for (int rows_min : {1, 4, 5, 9}) for (int qb = 1; qb <= SCAN_MAX_QB; ++qb) {
            IndexFacts fa;
            fa.storage = storage; fa.rows_min_qb = rows_min;
            printf("%d %d %d %d\n", storage, rows_min, qb, (int)index_scan_form(fa, qb));
        }
        return 0;
    }
    if (!strcmp(mode, "qblock")) {
        for (int dim = 512; dim <= 8192; dim += 512) printf("%d %d\n", dim, index_query_block(dim));
        for (int dim : {16384, 32768, 65536}) printf("%d %d\n", dim, index_query_block(dim));
        return 0;
    }
    if (!strcmp(mode, "capacity")) {
        for (int64_t cap : {0, 16, 1000, 1024, 1040, 2048, 100000, 1 << 20}) for (int64_t rows : {0, 1, 15, 16, 17, 1000, 1023, 1024, 1025, 1030, 2048, 2049, 4097, 100001, 400000, 3000001})
            printf("%lld %lld %lld\n", (long long)cap, (long long)rows, (long long)index_grown_capacity(cap, rows));
        for (int64_t nt : {0, 1, 15, 16, 17, 1030, 100000, 400001}) printf("loaded %lld %lld\n", (long long)nt, (long long)index_loaded_capacity(nt));
        return 0;
    }
    if (!strcmp(mode, "sizes")) {
        printf("SCAN_THREADS %d\nSCAN_WAVES %d\nSCAN_MAX_QB %d\nSCAN_ROWS_R %d\nMQ_THREADS %d\nMQ_WAVES %d\nMQ_RT %d\nMQ_NQ %d\nMQ_KS %d\nMQ_SLICE_BYTES %d\nMQ_SMEM %d\n"
               "INDEX_QUERY_LDS_BYTES %d\nTOPK_CHUNK %d\nTOPK_MAX_K %d\nTOPK_SEL_MAX_K %d\n",
               SCAN_THREADS, SCAN_WAVES, SCAN_MAX_QB, SCAN_ROWS_R, MQ_THREADS, MQ_WAVES, MQ_RT, MQ_NQ, MQ_KS, MQ_SLICE_BYTES, MQ_SMEM, INDEX_QUERY_LDS_BYTES, TOPK_CHUNK,
               TOPK_MAX_K, TOPK_SEL_MAX_K);
        return 0;
    }
    fprintf(stderr, "usage: %s plans OUT | passes | launch | forms | qblock | capacity | sizes\n", argv[0]);
    return 2;
}
