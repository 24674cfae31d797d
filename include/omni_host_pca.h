/* omni_host_pca.h -- C entry points of libomni_host_pca.so (omni-swarm_amd/host/host_pca_capi.cpp): the PCA fit of the key-frame pipeline of omni_host.h.
 * With the switch on every lane of the pipeline accumulates the moments of the 256-d descriptors of every key point of the stream in HBM (omni_hip.h's
 * omni_pcafit; the reference dumps them to a text file, OUTPUT_RAW_SUPERPOINT_DESC, and fits in pca.ipynb), and these entries merge, solve and write
 * components_.csv / mean_.csv -- the files every pipeline here is created with.  The handle is omni_host.h's omni_pipeline, whoever made it.  Returns as in
 * omni_host.h: 0 on success; after a failure omni_pca_host_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_PCA_H
#define OMNI_HOST_PCA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_pca_host_last_error(void);

/* on != 0: every lane gets an accumulator attached to its SuperPoint handle; on == 0 (the default): none, and a key-frame unit launches what it launched
 * before.  The pipeline's hits, candidates, edges and messages do not depend on the switch.  Refused: after the first key frame, and on the sharded database. */
int omni_pipeline_set_fit_pca(omni_pipeline* h, int on);
int omni_pipeline_get_fit_pca(omni_pipeline* h, int* on);
/* all four wait for the units in flight and merge the lanes' accumulators in a fixed order; refused with the switch off.
 * stats: kept rows and rows left out (a non-finite element).  moments: s [256], S [256][256] (symmetric), f64.  Any output may be NULL */
int omni_pipeline_pca_fit_stats(omni_pipeline* h, int64_t* n, int64_t* skipped);
int omni_pipeline_pca_fit_moments(omni_pipeline* h, int64_t* n, int64_t* skipped, double* s256, double* S_full);
/* omni_hip.h's omni_pca_solve_host on the merged moments: components [pca_dim][256] and mean [256] in f64 and f32, explained_variance [pca_dim],
 * *total_variance; any output may be NULL.  Refused: n < 2, pca_dim outside 1 .. 256, n <= pca_dim */
int omni_pipeline_pca_fit_solve(omni_pipeline* h, int pca_dim, double* components, float* components_f32, double* mean, float* mean_f32,
                                double* explained_variance, double* total_variance);
/* ... and written as components_.csv / mean_.csv ("%.9g": read back to the same f32) */
int omni_pipeline_pca_fit_write(omni_pipeline* h, const char* comp_path, const char* mean_path, int pca_dim);
/* every lane's accumulator back to zero */
int omni_pipeline_pca_fit_reset(omni_pipeline* h);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_PCA_H */
