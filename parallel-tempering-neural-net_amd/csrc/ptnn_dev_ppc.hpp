// ptnn_dev_ppc.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// posterior predictive checks (ptnn_ppc, include/ptnn.h).  Every selected occurrence i of a (w, eta)
// sample draws one replicated data set y_rep[i, .] from the model; test quantities T are evaluated on it and on the data, and
// p = P(T(y_rep, theta) >= T(y, theta)) is counted over the occurrences.
//   a. + b. as ptnn_elpd: distinct_samples (run-length pass with the eta compare), the per-shape predict_forward_kernel -- here
//      on a block of distinct vectors and ALL rows, so that one wave reduces all rows of an occurrence in one fixed order.
//   c. ppc_occurrence_kernel: one wave per job, no work-group barrier.  A job is a distinct vector of the block (T on the data:
//      it depends on the vector, not on the occurrence) or one occurrence (T on its replicate).  A regression's wave keeps its
//      standardised series -- e = (y - f) / tau or the draws z -- in LDS as doubles: lagged products read it there at any lag, and
//      every centred sum is a second pass over it.  Nothing of size [M, n_rows] goes to global memory unless z / y_rep is asked for.
//      ppc_reduce_kernel: one work-group per statistic over the occurrences: integer counts, and two-pass double sums in an
//      order that M alone fixes.
// The draw of occurrence i, row n is component n % 4 of philox4x32_10(n / 4, i, 0, STREAM_PPC, seed): a regression's z by
// box_muller (ptnn_forecast's generator), a classification's u by u23.  fp64 throughout after f / p.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int PPC_THREADS = 256;          // at most 4 waves = 4 jobs per work-group
constexpr int PPC_MAX_LAGS = 16;          // include/ptnn.h: PTNN_PPC_MAX_LAGS
constexpr uint32_t STREAM_PPC = 6;        // replicated data of ptnn_ppc (counter: row / 4, occurrence, 0)
constexpr int PPC_REG_FIXED = 7;          // mean, sd, min, max, chi2, max_abs_resid, ljung_box; then resid_acf per lag
constexpr int PPC_CLS_FIXED = 2;          // deviance, accuracy; then class_count per class

struct PpcJob {
    int n_rows, O;
    int nu;                     // distinct vectors of this block
    int u0;                     // the block's first distinct vector
    const float* fx;            // [n_rows * O][nu] outputs of the block (predict_forward_kernel layout)
    const float* eta;           // [U] eta of every distinct vector (regression)
    const float* y;             // target of row n at y[n * ys]
    int ys;
    int n_lags;
    int lags[PPC_MAX_LAGS];
    uint32_t seed_lo, seed_hi;
    long long i0;               // the block's first occurrence
    int n_occ;                  // its occurrences [i0, i0 + n_occ)
    const int* occ_u;           // [M] the distinct vector of every occurrence (non-decreasing)
    int n_stats;
    int wave_doubles;           // LDS doubles per wave
    double* t_obs;              // [U][n_stats]
    double* t_rep;              // [M][n_stats]
    float* z;                   // [M][n_rows] or null (regression)
    int* y_rep;                 // [M][n_rows] or null (classification)
};

// statistics 0-3 of a series x(n), n < N, lane l holding n = l, l + 64, ...: mean, population sd (centred: a second pass), min, max
template <class F>
__device__ __forceinline__ void ppc_level_stats(F x, int N, int lane, double* out) {
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double s = 0.0, mn = INF, mx = -INF;
    for (int n = lane; n < N; n += WAVE) {
        const double v = x(n);
        s += v; mn = fmin(mn, v); mx = fmax(mx, v);
    }
    const double m = wave_sum(s) / (double)N;
    double c = 0.0;
    for (int n = lane; n < N; n += WAVE) {
        const double d = x(n) - m;
        c += d * d;
    }
    c = wave_sum(c);
    mn = wave_min(mn); mx = wave_max(mx);
    if (m != m) { mn = m; mx = m; }                    // fmin / fmax drop a NaN; the mean does not
    if (lane == 0) { out[0] = m; out[1] = sqrt(c / (double)N); out[2] = mn; out[3] = mx; }
}

// statistics 4 .. of a standardised series v [N] in the wave's LDS: chi2 = sum v^2, max |v|, Ljung-Box over the lags, acf per lag
__device__ __forceinline__ void ppc_resid_stats(const double* v, int N, const PpcJob& a, int lane, double* out) {
    double s = 0.0, q = 0.0, mx = 0.0;
    for (int n = lane; n < N; n += WAVE) {
        const double x = v[n];
        s += x; q += x * x; mx = fmax(mx, fabs(x));
    }
    const double m = wave_sum(s) / (double)N;
    q = wave_sum(q);
    mx = wave_max(mx);
    if (q != q) mx = q;
    double c0 = 0.0, ck[PPC_MAX_LAGS];
#pragma unroll
    for (int j = 0; j < PPC_MAX_LAGS; ++j) ck[j] = 0.0;
    for (int n = lane; n < N; n += WAVE) {
        const double d = v[n] - m;
        c0 += d * d;
#pragma unroll
        for (int j = 0; j < PPC_MAX_LAGS; ++j)
            if (j < a.n_lags && n >= a.lags[j]) ck[j] += d * (v[n - a.lags[j]] - m);
    }
    c0 = wave_sum(c0);
    double lb = 0.0;
#pragma unroll
    for (int j = 0; j < PPC_MAX_LAGS; ++j) {
        if (j < a.n_lags) {
            const double r = wave_sum(ck[j]) / c0;
            lb += r * r / (double)(N - a.lags[j]);
            if (lane == 0) out[PPC_REG_FIXED + j] = r;
        }
    }
    if (lane == 0) { out[4] = q; out[5] = mx; out[6] = (double)N * (double)(N + 2) * lb; }
}

// one classification row with its label: -2 log p_label into dev, a hit into hits, the label's class count (LDS, integer)
__device__ __forceinline__ void ppc_class_row(const float* p, size_t stride, int O, int label, int arg, double& dev, long long& hits,
                                              int* count) {
    if (label >= 0 && label < O) {
        dev += -2.0 * log((double)p[(size_t)label * stride]);
        hits += label == arg;
        atomicAdd(&count[label], 1);
    } else {
        dev = __longlong_as_double(0x7ff8000000000000ll);       // no such class: the deviance is undefined
    }
}

// REG: a regression (n_out == 1) / a classification
template <bool REG>
__global__ void __launch_bounds__(PPC_THREADS) ppc_occurrence_kernel(const PpcJob a) {
    extern __shared__ __attribute__((aligned(16))) double ppc_lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long job = (long long)blockIdx.x * (blockDim.x / WAVE) + wave;
    if (job >= (long long)a.nu + a.n_occ) return;               // whole waves leave: no work-group barrier below
    const bool obs = job < a.nu;
    const long long i = obs ? 0 : a.i0 + (job - a.nu);          // the occurrence
    const int u = obs ? a.u0 + (int)job : a.occ_u[i];           // its distinct vector
    const int ul = u - a.u0;
    if (ul < 0 || ul >= a.nu) return;                           // (the host keeps occurrences inside their block)
    const int N = a.n_rows;
    double* out = obs ? a.t_obs + (size_t)u * a.n_stats : a.t_rep + (size_t)i * a.n_stats;
    const float* f = a.fx + ul;                                 // output o of row n at f[(n * O + o) * nu]
    const size_t nu = (size_t)a.nu;

    if constexpr (REG) {
        double* v = ppc_lds + (size_t)wave * a.wave_doubles;    // the standardised series of this job
        const double tau = exp(0.5 * (double)a.eta[u]);
        if (obs) {
            for (int n = lane; n < N; n += WAVE) v[n] = ((double)a.y[(size_t)n * a.ys] - (double)f[n * nu]) / tau;
            gsync<true>();
            ppc_level_stats([&](int n) { return (double)a.y[(size_t)n * a.ys]; }, N, lane, out);
        } else {
            float* zo = a.z ? a.z + (size_t)i * N : nullptr;
            for (int b = lane; 4 * b < N; b += WAVE) {
                uint32_t q[4];
                float z[4];
                philox4x32_10((uint32_t)b, (uint32_t)i, 0u, STREAM_PPC, a.seed_lo, a.seed_hi, q);
                box_muller(q[0], q[1], z[0], z[1]);
                box_muller(q[2], q[3], z[2], z[3]);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int n = 4 * b + c;
                    if (n < N) {
                        v[n] = (double)z[c];
                        if (zo) zo[n] = z[c];
                    }
                }
            }
            gsync<true>();
            ppc_level_stats([&](int n) { return (double)f[n * nu] + tau * v[n]; }, N, lane, out);
        }
        ppc_resid_stats(v, N, a, lane, out);
    } else {
        // classification: deviance, accuracy and class counts of the labels -- the data's, or the occurrence's draws
        const int O = a.O;
        int* count = reinterpret_cast<int*>(ppc_lds + (size_t)wave * a.wave_doubles);
        for (int k = lane; k < O; k += WAVE) count[k] = 0;
        gsync<true>();
        int* yo = !obs && a.y_rep ? a.y_rep + (size_t)i * N : nullptr;
        double dev = 0.0;
        long long hits = 0;
        for (int b = lane; 4 * b < N; b += WAVE) {
            uint32_t q[4] = {0u, 0u, 0u, 0u};
            if (!obs) philox4x32_10((uint32_t)b, (uint32_t)i, 0u, STREAM_PPC, a.seed_lo, a.seed_hi, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int n = 4 * b + c;
                if (n >= N) continue;
                const float* p = f + (size_t)n * O * nu;
                double total = 0.0, best = (double)p[0];
                int arg = 0;
                for (int k = 0; k < O; ++k) {
                    const double pk = (double)p[k * nu];
                    total += pk;
                    if (pk > best) { best = pk; arg = k; }
                }
                int label;
                if (obs) {
                    label = (int)a.y[(size_t)n * a.ys];
                } else {
                    const double t = (double)u23(q[c]) * total;
                    double cum = 0.0;
                    label = O - 1;
                    for (int k = 0; k < O; ++k) {
                        cum += (double)p[k * nu];
                        if (cum > t) { label = k; break; }
                    }
                    if (yo) yo[n] = label;
                }
                ppc_class_row(p, nu, O, label, arg, dev, hits, count);
            }
        }
        dev = wave_sum(dev);
        hits = wave_sum(hits);
        gsync<true>();
        if (lane == 0) { out[0] = dev; out[1] = (double)hits / (double)N; }
        for (int k = lane; k < O; k += WAVE) out[PPC_CLS_FIXED + k] = (double)count[k];
    }
}

// ---- the reduction over the occurrences: one work-group per statistic ----
struct PpcReduce {
    long long M;
    int n_stats;
    const int* occ_u;           // [M]
    const double* t_obs;        // [U][n_stats]
    const double* t_rep;        // [M][n_stats]
    long long* n_defined;       // [n_stats] each
    long long* n_greater;
    long long* n_equal;
    double* mean_obs;
    double* mean_rep;
    double* var_rep;
};

// thread t takes the occurrences t, t + 256, ...: the order of every double sum is fixed by M; an occurrence whose T is not
// finite on either side adds nothing anywhere
__global__ void __launch_bounds__(PPC_THREADS) ppc_reduce_kernel(const PpcReduce a) {
    __shared__ double shd[PPC_THREADS];
    __shared__ long long shi[PPC_THREADS];
    const int j = blockIdx.x, tid = threadIdx.x;
    long long nd = 0, ng = 0, ne = 0;
    double so = 0.0, sr = 0.0;
    for (long long i = tid; i < a.M; i += PPC_THREADS) {
        const double to = a.t_obs[(size_t)a.occ_u[i] * a.n_stats + j], tr = a.t_rep[(size_t)i * a.n_stats + j];
        if (!(isfinite(to) && isfinite(tr))) continue;
        ++nd; ng += tr > to; ne += tr == to;
        so += to; sr += tr;
    }
    nd = wg_sum<PPC_THREADS>(shi, nd); ng = wg_sum<PPC_THREADS>(shi, ng); ne = wg_sum<PPC_THREADS>(shi, ne);
    const double mo = wg_sum<PPC_THREADS>(shd, so) / (double)nd, mr = wg_sum<PPC_THREADS>(shd, sr) / (double)nd;
    double c = 0.0;
    for (long long i = tid; i < a.M; i += PPC_THREADS) {
        const double to = a.t_obs[(size_t)a.occ_u[i] * a.n_stats + j], tr = a.t_rep[(size_t)i * a.n_stats + j];
        if (!(isfinite(to) && isfinite(tr))) continue;
        c += (tr - mr) * (tr - mr);
    }
    c = wg_sum<PPC_THREADS>(shd, c);
    if (tid == 0) {
        a.n_defined[j] = nd; a.n_greater[j] = ng; a.n_equal[j] = ne;
        a.mean_obs[j] = mo; a.mean_rep[j] = mr; a.var_rep[j] = c / (double)nd;
    }
}
