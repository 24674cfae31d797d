// pcafit_pin.cpp -- csrc/pca_plan.h as a stand-alone g++ program (built with ASan + UBSan by tests/test_pca_plan_cpu.py): every buffer is a heap allocation of
// exactly the promised size, so a read or write one element beyond raw_desc [batch][max_num][256], norm_partial [batch][8][256], n_kps [batch], s [256],
// S [256][256], the solve's work area or its outputs stops the program.  Cases: n_kps 0, 1 and max_num, batch 1 and 3, counts outside 0 .. max_num; the same rows
// cut into calls; merge; solve, its refusals and the CSV writer.  Prints one line per check and "OK" at the end; any failure exits non-zero.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../omni-swarm_amd/csrc/pca_plan.h"

using namespace omni::pca;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static float next_float() {          // xorshift: values in (-1, 1), never 0
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return ((float)((g_rng >> 40) + 1) / 16777217.0f) * 2.0f - 1.0f;
}
static void fail(const char* what) { std::printf("FAIL %s\n", what); std::exit(1); }

struct Acc {
    std::unique_ptr<double[]> s{new double[kDim]()}, S{new double[(size_t)kDim * kDim]()};
    Moments m;
    Acc() { m.s = s.get(); m.S = S.get(); }
};
struct Pass {
    int batch, max_num;
    std::unique_ptr<float[]> raw, part;
    std::unique_ptr<int[]> n_kps;
    Pass(int b, int mn, const int* counts) : batch(b), max_num(mn), raw(new float[(size_t)b * mn * kDim]), part(new float[(size_t)b * kNormSegs * kDim]), n_kps(new int[b]) {
        for (size_t i = 0; i < (size_t)b * mn * kDim; ++i) raw[i] = next_float();
        for (size_t i = 0; i < (size_t)b * kNormSegs * kDim; ++i) part[i] = 0.5f + std::fabs(next_float());
        for (int i = 0; i < b; ++i) n_kps[i] = counts[i];
    }
    void add_to(Acc& a) const { moments_host(a.m, raw.get(), part.get(), n_kps.get(), batch, max_num); }
};
static bool same(const Acc& a, const Acc& b) {
    if (a.m.n != b.m.n || a.m.skipped != b.m.skipped || std::memcmp(a.s.get(), b.s.get(), kDim * 8)) return false;
    for (int r = 0; r < kDim; ++r) if (std::memcmp(a.S.get() + (size_t)r * kDim + r, b.S.get() + (size_t)r * kDim + r, (size_t)(kDim - r) * 8)) return false;
    return true;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    // counts 0, 1, max_num; batch 1 and 3; counts beyond the range are clamped
    const int mns[2] = {8, 40};
    for (int mn : mns) {
        const int singles[5] = {0, 1, mn, -5, mn + 9};
        const int64_t want[5] = {0, 1, mn, 0, mn};
        for (int k = 0; k < 5; ++k) {
            Acc a;
            Pass(1, mn, &singles[k]).add_to(a);
            if (a.m.n != want[k] || a.m.skipped != 0) fail("batch 1 count");
        }
        const int three[3] = {mn, 0, 1};
        Acc a;
        Pass p(3, mn, three);
        p.add_to(a);
        if (a.m.n != mn + 1) fail("batch 3 count");
        // lower triangle never touched
        for (int r = 1; r < kDim; ++r) for (int c = 0; c < r; ++c) if (a.S[(size_t)r * kDim + c] != 0.0) fail("lower triangle written");
        // the same rows, one image per call: bit-identical
        Acc b;
        for (int i = 0; i < 3; ++i) moments_host(b.m, p.raw.get() + (size_t)i * mn * kDim, p.part.get() + (size_t)i * kNormSegs * kDim, p.n_kps.get() + i, 1, mn);
        if (!same(a, b)) fail("cut into calls");
        std::printf("max_num %d: counts, clamping, cut independence ok (n %lld)\n", mn, (long long)a.m.n);
    }
    // skip rule: a zero channel (all eight segment sums 0) -> 0/0 in every row of the image
    {
        const int counts[3] = {5, 8, 3};
        Pass p(3, 8, counts);
        for (int s = 0; s < kNormSegs; ++s) p.part[((size_t)1 * kNormSegs + s) * kDim + 17] = 0.f;
        for (int i = 0; i < 8; ++i) p.raw[((size_t)1 * 8 + i) * kDim + 17] = 0.f;
        Acc a;
        p.add_to(a);
        if (a.m.n != 8 || a.m.skipped != 8) fail("skip rule");
        for (int c = 0; c < kDim; ++c) if (!std::isfinite(a.s[c]) || !std::isfinite(a.S[(size_t)c * kDim + c])) fail("a skipped row reached the moments");
        std::printf("skip rule ok (n %lld skipped %lld)\n", (long long)a.m.n, (long long)a.m.skipped);
    }
    // merge + solve + refusals + CSV on 300 rows
    {
        const int counts[3] = {100, 100, 100};
        Pass p(3, 100, counts);
        Acc whole, left, right;
        p.add_to(whole);
        moments_host(left.m, p.raw.get(), p.part.get(), p.n_kps.get(), 1, 100);
        moments_host(right.m, p.raw.get() + (size_t)100 * kDim, p.part.get() + (size_t)kNormSegs * kDim, p.n_kps.get() + 1, 2, 100);
        merge(left.m, right.m);
        if (left.m.n != whole.m.n) fail("merge n");
        double worst = 0;
        for (int r = 0; r < kDim; ++r) for (int c = r; c < kDim; ++c) worst = std::fmax(worst, std::fabs(left.S[(size_t)r * kDim + c] - whole.S[(size_t)r * kDim + c]));
        if (!(worst < 1e-9)) fail("merge S");
        mirror(whole.S.get());
        std::unique_ptr<double[]> work(new double[(size_t)kSolveWorkDoubles]), comp(new double[64 * kDim]), mean(new double[kDim]), ev(new double[64]);
        std::unique_ptr<float[]> comp32(new float[64 * kDim]), mean32(new float[kDim]);
        std::unique_ptr<int[]> order(new int[kDim]);
        double tv = 0;
        if (solve(whole.m.n, whole.s.get(), whole.S.get(), 64, work.get(), order.get(), comp.get(), comp32.get(), mean.get(), mean32.get(), ev.get(), &tv) != SOLVE_OK) fail("solve");
        double orth = 0;
        for (int a = 0; a < 64; ++a) for (int b = a; b < 64; ++b) {
            double d = 0;
            for (int c = 0; c < kDim; ++c) d += comp[(size_t)a * kDim + c] * comp[(size_t)b * kDim + c];
            orth = std::fmax(orth, std::fabs(d - (a == b ? 1.0 : 0.0)));
        }
        for (int k = 1; k < 64; ++k) if (ev[k] > ev[k - 1]) fail("eigenvalues not descending");
        for (int k = 0; k < 64; ++k) {
            int arg = 0;
            for (int c = 1; c < kDim; ++c) if (std::fabs(comp[(size_t)k * kDim + c]) > std::fabs(comp[(size_t)k * kDim + arg])) arg = c;
            if (!(comp[(size_t)k * kDim + arg] > 0)) fail("sign rule");
        }
        if (!(orth < 1e-12) || !(tv > 0)) fail("orthonormal rows");
        if (solve(whole.m.n, whole.s.get(), whole.S.get(), 1, work.get(), order.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SOLVE_OK) fail("solve with null outputs");
        if (solve(1, whole.s.get(), whole.S.get(), 1, work.get(), order.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SOLVE_FEW_ROWS) fail("refusal n < 2");
        if (solve(300, whole.s.get(), whole.S.get(), 0, work.get(), order.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SOLVE_BAD_DIM) fail("refusal pca_dim 0");
        if (solve(300, whole.s.get(), whole.S.get(), 257, work.get(), order.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SOLVE_BAD_DIM) fail("refusal pca_dim 257");
        if (solve(64, whole.s.get(), whole.S.get(), 64, work.get(), order.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SOLVE_ROWS_LE_DIM) fail("refusal n <= pca_dim");
        const std::string cp = dir + "/components_.csv", mp = dir + "/mean_.csv";
        if (!write_csv(cp.c_str(), mp.c_str(), comp32.get(), mean32.get(), 64)) fail("write_csv");
        if (write_csv((dir + "/no/such/dir/c.csv").c_str(), mp.c_str(), comp32.get(), mean32.get(), 64)) fail("write_csv into a missing directory");
        std::printf("merge %.3e, solve: rows orthonormal within %.3e, total variance %.6f, csv written\n", worst, orth, tv);
    }
    std::printf("OK\n");
    return 0;
}
