// pca_plan.h -- the fit half of the reference's PCA workflow (OUTPUT_RAW_SUPERPOINT_DESC dumps every key point's 256-d descriptor, loop_cam.cpp:51-53, 577-582;
// pca.ipynb fits sklearn.decomposition.PCA(64) on the dump and writes components_.csv / mean_.csv with np.savetxt), stated once.  Plain C++ for g++ AND hipcc:
// pca_fit.hip runs rows_keep / row_value / the fma chain on the GPU, pca_fit_host.cpp (omni_pca_moments_host) and tests/cpp/pcafit_pin.cpp run the same functions
// on the host; nothing else restates the arithmetic.  Every product and sum rounds on its own (contraction off) except the ONE fused multiply-add that is
// written as fma(); IEEE division and square root.
//
// Row        x[c] = raw[c] / chan_norm(b, c) in f32, chan_norm = sqrtf of the eight segment sums of norm_partial added in order (sp_post.hip's chan_norm_of): the
//            value copy_raw_desc_kernel stores, i.e. the 256-d descriptor a handle without PCA returns.  Then widened to f64 (exact).
// Skip rule  image b has rows 0 .. clamp(n_kps[b], 0, max_num) - 1; a row with any non-finite element is left out and counted in `skipped` (a channel that is
//            zero at every key point of an image gives 0/0 for the whole image, in the reference too).
// Moments    n (int64), s[256], S[i][j] for i <= j (32 896 entries; stored in a full [256][256] array whose lower triangle is never touched).  Per kept row, in
//            STREAM ORDER (images in order, key points in order, calls in order): n += 1, s[c] += x[c], S[i][j] = fma(x[i], x[j], S[i][j]).  One strict chain
//            per entry: the order of additions into an entry is a function of the row sequence alone, not of launch geometry, batch size or how the stream
//            was cut into calls.
// Merge      left.n += right.n, left.s += right.s, left.S += right.S element-wise.
// Solve      (host only, f64) C[i][j] = (S[i][j] - s[i] * s[j] / n) / (n - 1), mean = s / n; cyclic Jacobi with pnp_plan.h's jacobi_eigen rotation order, skip
//            rule (|A[p][q]| < 1e-300) and stop rule (off <= 1e-30 * (diag + 1e-300), 60 sweeps) at a run-time size on heap storage; eigenvalues descending, ties
//            to the lower index; the first pca_dim eigenvectors are the rows of `components`; sign: the entry of largest magnitude of each row is positive,
//            ties to the lowest column (scikit-learn's svd_flip on the rows of Vt).
// CSV        components_.csv one component per line, comma separated; mean_.csv one value per line; "%.9g", which std::stof reads back to the same f32.  A value
//            below the smallest normal f32 in magnitude is written as 0: std::stof (load_csv_floats, the reader of every handle) refuses denormals.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define PCA_HD __host__ __device__ inline
#else
#define PCA_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace omni {
namespace pca {

constexpr int kDim = 256;          // SuperPoint's descriptor length
constexpr int kNormSegs = 8;       // sp_post.hip's NORM_SEGS: norm_partial is [B][8][256]
constexpr int kTriangle = kDim * (kDim + 1) / 2;
constexpr float kFltMax = 3.402823466e38f;

enum Refusal { SOLVE_OK = 0, SOLVE_FEW_ROWS = 1, SOLVE_BAD_DIM = 2, SOLVE_ROWS_LE_DIM = 3 };

PCA_HD int clamp_count(int n_raw, int max_num) { return n_raw < 0 ? 0 : (n_raw > max_num ? max_num : n_raw); }
PCA_HD bool finite_f32(float v) { return fabsf(v) <= kFltMax; }      // std::isfinite (false for NaN)

// sp_post.hip's chan_norm_of: eight segment sums added in order, then the square root
PCA_HD float chan_norm(const float* norm_partial, int b, int c) {
    float ss = 0.f;
    for (int s = 0; s < kNormSegs; ++s) ss += norm_partial[((int64_t)b * kNormSegs + s) * kDim + c];
    return sqrtf(ss);
}
// an element of a row from its raw value and the image's norm of its channel (f32, IEEE division), and the same widened for the moments
PCA_HD float normalised(float raw, float norm) { return raw / norm; }
PCA_HD double widened(float raw, float norm) { return (double)normalised(raw, norm); }
// element c of row (b, i), given the image's norm of that channel
PCA_HD float row_value(const float* raw_desc, int max_num, int b, int i, int c, float norm) { return normalised(raw_desc[((int64_t)b * max_num + i) * kDim + c], norm); }

// the chain's one step for one entry
PCA_HD double step(double x_i, double x_j, double S_ij) { return fma(x_i, x_j, S_ij); }

struct Moments {          // host form of the accumulator: S full [256][256], entries i <= j used
    int64_t n = 0, skipped = 0;
    double* s = nullptr;  // [256]
    double* S = nullptr;  // [256][256]
};

// host form of one enqueue on the arrays of omni_pcafit_enqueue_rows_dev: what the kernels compute, sequentially.  raw_desc [batch][max_num][256],
// norm_partial [batch][8][256], n_kps [batch]
inline void moments_host(Moments& m, const float* raw_desc, const float* norm_partial, const int* n_kps, int batch, int max_num) {
    float norm[kDim], xf[kDim];
    double x[kDim];
    for (int b = 0; b < batch; ++b) {
        const int n = clamp_count(n_kps[b], max_num);
        if (n == 0) continue;
        for (int c = 0; c < kDim; ++c) norm[c] = chan_norm(norm_partial, b, c);
        for (int i = 0; i < n; ++i) {
            bool keep = true;
            for (int c = 0; c < kDim; ++c) { xf[c] = row_value(raw_desc, max_num, b, i, c, norm[c]); keep = keep && finite_f32(xf[c]); }
            if (!keep) { m.skipped += 1; continue; }
            m.n += 1;
            for (int c = 0; c < kDim; ++c) { x[c] = (double)xf[c]; m.s[c] += x[c]; }      // (= widened(raw, norm))
            for (int r = 0; r < kDim; ++r) {
                double* Sr = m.S + (int64_t)r * kDim;
                const double xr = x[r];
                for (int c = r; c < kDim; ++c) Sr[c] = step(xr, x[c], Sr[c]);
            }
        }
    }
}

inline void merge(Moments& left, const Moments& right) {
    left.n += right.n; left.skipped += right.skipped;
    for (int c = 0; c < kDim; ++c) left.s[c] += right.s[c];
    for (int r = 0; r < kDim; ++r) for (int c = r; c < kDim; ++c) left.S[(int64_t)r * kDim + c] += right.S[(int64_t)r * kDim + c];
}

// lower triangle := upper triangle (how the moments are handed out)
inline void mirror(double* S) { for (int r = 0; r < kDim; ++r) for (int c = 0; c < r; ++c) S[(int64_t)r * kDim + c] = S[(int64_t)c * kDim + r]; }

inline const char* refusal_text(int why) {
    switch (why) {
    case SOLVE_FEW_ROWS: return "a PCA needs at least two rows (n < 2)";
    case SOLVE_BAD_DIM: return "pca_dim outside [1, 256]";
    case SOLVE_ROWS_LE_DIM: return "a PCA of pca_dim components needs more than pca_dim rows (n <= pca_dim)";
    default: return "";
    }
}
inline int check_solve(int64_t n, int pca_dim) {
    if (pca_dim < 1 || pca_dim > kDim) return SOLVE_BAD_DIM;
    if (n < 2) return SOLVE_FEW_ROWS;
    if (n <= pca_dim) return SOLVE_ROWS_LE_DIM;
    return SOLVE_OK;
}

// pnp_plan.h's jacobi_eigen<N> at a run-time size: A [N][N] (destroyed), V [N][N] (eigenvectors as ROWS, unsorted), W [N] = the diagonal.  Returns the sweeps used
inline int jacobi_eigen_n(int N, double* A, double* W, double* V) {
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) V[(int64_t)i * N + j] = i == j ? 1.0 : 0.0;
    int sweep = 0;
    for (; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < N; ++i) { diag += A[(int64_t)i * N + i] * A[(int64_t)i * N + i]; for (int j = i + 1; j < N; ++j) off += A[(int64_t)i * N + j] * A[(int64_t)i * N + j]; }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                double* Ap = A + (int64_t)p * N; double* Aq = A + (int64_t)q * N;
                if (fabs(Ap[q]) < 1e-300) continue;
                const double theta = (Aq[q] - Ap[p]) / (2 * Ap[q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < N; ++k) { double* Ak = A + (int64_t)k * N; const double akp = Ak[p], akq = Ak[q]; Ak[p] = c * akp - s * akq; Ak[q] = s * akp + c * akq; }
                for (int k = 0; k < N; ++k) { const double apk = Ap[k], aqk = Aq[k]; Ap[k] = c * apk - s * aqk; Aq[k] = s * apk + c * aqk; }
                double* Vp = V + (int64_t)p * N; double* Vq = V + (int64_t)q * N;
                for (int k = 0; k < N; ++k) { const double vpk = Vp[k], vqk = Vq[k]; Vp[k] = c * vpk - s * vqk; Vq[k] = s * vpk + c * vqk; }
            }
    }
    for (int i = 0; i < N; ++i) W[i] = A[(int64_t)i * N + i];
    return sweep;
}

// HOST ONLY.  S: full [256][256] of which i <= j is read; work: [2 * 256 * 256 + 256] doubles; order: [256] ints.  Outputs (any may be null): components
// [pca_dim][256] f64 / f32, mean [256] f64 / f32, explained_variance [pca_dim], *total_variance = trace(C).  Returns a Refusal
inline int solve(int64_t n, const double* s, const double* S, int pca_dim, double* work, int* order, double* comp64, float* comp32, double* mean64, float* mean32,
                 double* explained, double* total_variance) {
    const int why = check_solve(n, pca_dim);
    if (why) return why;
    const int N = kDim;
    double* A = work; double* V = work + (int64_t)N * N; double* W = V + (int64_t)N * N;
    const double dn = (double)n, dn1 = (double)(n - 1);
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) { const double v = (S[(int64_t)i * N + j] - s[i] * s[j] / dn) / dn1; A[(int64_t)i * N + j] = v; A[(int64_t)j * N + i] = v; }
    double tr = 0;
    for (int i = 0; i < N; ++i) tr += A[(int64_t)i * N + i];
    if (total_variance) *total_variance = tr;
    for (int c = 0; c < N; ++c) { const double m = s[c] / dn; if (mean64) mean64[c] = m; if (mean32) mean32[c] = (float)m; }
    jacobi_eigen_n(N, A, W, V);
    // descending, ties to the lower index: a stable insertion sort
    for (int i = 0; i < N; ++i) order[i] = i;
    for (int i = 1; i < N; ++i) { const int val = order[i]; int j = i; while (j > 0 && W[val] > W[order[j - 1]]) { order[j] = order[j - 1]; --j; } order[j] = val; }
    for (int k = 0; k < pca_dim; ++k) {
        const double* v = V + (int64_t)order[k] * N;
        int arg = 0;
        for (int c = 1; c < N; ++c) if (fabs(v[c]) > fabs(v[arg])) arg = c;
        const double sign = v[arg] < 0 ? -1.0 : 1.0;
        for (int c = 0; c < N; ++c) { const double e = sign * v[c]; if (comp64) comp64[(int64_t)k * N + c] = e; if (comp32) comp32[(int64_t)k * N + c] = (float)e; }
        if (explained) explained[k] = W[order[k]];
    }
    return SOLVE_OK;
}
constexpr int64_t kSolveWorkDoubles = 2 * (int64_t)kDim * kDim + kDim;

// components_.csv / mean_.csv as np.savetxt(delimiter=',') lays them out, "%.9g".  false: a file could not be written
inline double csv_value(float v) { return fabsf(v) < 1.17549435e-38f ? 0.0 : (double)v; }
inline bool write_csv(const char* comp_path, const char* mean_path, const float* comp32, const float* mean32, int pca_dim) {
    FILE* f = fopen(comp_path, "w");
    if (!f) return false;
    bool ok = true;
    for (int k = 0; k < pca_dim && ok; ++k)
        for (int c = 0; c < kDim && ok; ++c) ok = fprintf(f, c + 1 < kDim ? "%.9g," : "%.9g\n", csv_value(comp32[(int64_t)k * kDim + c])) > 0;
    ok = (fclose(f) == 0) && ok;
    if (!ok) return false;
    f = fopen(mean_path, "w");
    if (!f) return false;
    for (int c = 0; c < kDim && ok; ++c) ok = fprintf(f, "%.9g\n", csv_value(mean32[c])) > 0;
    return (fclose(f) == 0) && ok;
}

}  // namespace pca
}  // namespace omni
