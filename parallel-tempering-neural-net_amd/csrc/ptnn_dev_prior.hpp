// ptnn_dev_prior.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// prior predictive checks (ptnn_prior_predictive, include/ptnn.h).  What do the functions look like that
// the prior w ~ N(0, sigma^2) puts on the net, before any data is looked at?  Per prior scale, one after another:
//   a. evid_prior_kernel (ptnn_dev_evidence.hpp), unchanged: blocks of drawn vectors w = sigma z, z from Philox stream 5.
//   b. the per-shape predict_forward_kernel, unchanged, on the block; a 2-D device copy places its [cols][block] outputs into
//      the scale's full matrix fx [cols][n_draws], which every reduction below reads: no result depends on the block size.
//   c. predict_reduce_kernel (ptnn_dev_select.hpp), unchanged, with multiplicity 1: mean, exact order statistics and votes of
//      every column over the draws; prior_saturation_kernel: the draws of a column with f < eps or f > 1 - eps, counted.
//   d. prior_function_kernel: one lane per draw walks all rows in row order (adjacent lanes read adjacent draws of a column):
//      the statistics of the drawn function over the rows, double arithmetic on the fp32 outputs, centred sums in a second
//      pass; written [stat][draw] in double and in fp32 -- the fp32 copy is predict_reduce_kernel's column layout, which
//      gives the order statistics over the draws.  prior_target_kernel: the same statistics of the target series / labels.
//   e. prior_stat_kernel: one work-group per statistic over the draws: mean and population sd (two passes, fixed tree) and the
//      integer counts of T(f_i) against T(y); a NaN draw is left out of all of them.
// Everything is about f, the network output: tau^2 has an improper prior, so replicated y is not defined under the prior.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int PRIOR_THREADS = 256;        // 4 waves
constexpr int PRIOR_MAX_SCALES = 8;       // include/ptnn.h: PTNN_PRIOR_MAX_SCALES
constexpr int PRIOR_REG_STATS = 7;        // mean, sd, min, max, acf1, rmse, saturated
constexpr int PRIOR_CLS_FIXED = 4;        // accuracy, log_score, confidence, saturated; then class_share per class
constexpr int PRIOR_CLASS_GROUP = 16;     // classes whose counts one walk over the rows keeps in registers

__device__ __forceinline__ double prior_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// stage c: one work-group per column of fx [ncols][n]: the draws outside [eps, 1 - eps]
__global__ void __launch_bounds__(PRIOR_THREADS) prior_saturation_kernel(const float* fx, long long n, double eps, long long* count) {
    __shared__ long long shi[PRIOR_THREADS];
    const float* f = fx + (size_t)blockIdx.x * n;
    long long c = 0;
    for (long long u = threadIdx.x; u < n; u += PRIOR_THREADS) {
        const double v = (double)f[u];
        c += (v < eps || v > 1.0 - eps) ? 1 : 0;
    }
    c = wg_sum<PRIOR_THREADS>(shi, c);
    if (threadIdx.x == 0) count[blockIdx.x] = c;
}

// mean, population sd, min, max and lag-1 autocorrelation (centred) of a series x(r), r < N, walked in row order
template <class F>
__device__ __forceinline__ void prior_series_stats(F x, int N, double* mean, double* sd, double* mn_out, double* mx_out, double* acf1) {
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double s = 0.0, mn = INF, mx = -INF;
    for (int r = 0; r < N; ++r) {
        const double v = x(r);
        s += v; mn = fmin(mn, v); mx = fmax(mx, v);
    }
    const double m = s / (double)N;
    double c0 = 0.0, c1 = 0.0, prev = 0.0;
    for (int r = 0; r < N; ++r) {
        const double d = x(r) - m;
        c0 += d * d;
        if (r > 0) c1 += d * prev;
        prev = d;
    }
    if (m != m) { mn = m; mx = m; }                    // fmin / fmax drop a NaN; the mean does not
    *mean = m; *sd = sqrt(c0 / (double)N); *mn_out = mn; *mx_out = mx;
    *acf1 = c1 / c0;                                    // a constant series: 0 / 0, undefined
}

// stage d: the statistics of every drawn function over the rows
struct PriorFn {
    const float* fx;            // [n_rows * O][n] outputs of all draws (predict_forward_kernel layout, row length n)
    long long n;                // draws
    int n_rows, O;
    const float* y;             // target of row r at y[r * ys], or null
    int ys;
    double eps;
    double* t;                  // [n_stats][n]
    float* t32;                 // [n_stats][n] the same, rounded
};

template <bool REG>
__global__ void __launch_bounds__(PRIOR_THREADS) prior_function_kernel(const PriorFn a) {
    const long long u = (long long)blockIdx.x * PRIOR_THREADS + threadIdx.x;
    if (u >= a.n) return;
    const size_t n = (size_t)a.n;
    const int N = a.n_rows;
    const float* f = a.fx + u;                          // output o of row r at f[(r * O + o) * n]
    double* t = a.t + u;                                // statistic j at t[j * n]
    auto put = [&](int j, double v) { t[(size_t)j * n] = v; a.t32[(size_t)j * n + u] = (float)v; };
    if constexpr (REG) {
        double mean, sd, mn, mx, acf1;
        prior_series_stats([&](int r) { return (double)f[(size_t)r * n]; }, N, &mean, &sd, &mn, &mx, &acf1);
        double se = 0.0;
        long long sat = 0;
        for (int r = 0; r < N; ++r) {
            const double v = (double)f[(size_t)r * n];
            sat += (v < a.eps || v > 1.0 - a.eps) ? 1 : 0;
            if (a.y) { const double d = (double)a.y[(size_t)r * a.ys] - v; se += d * d; }
        }
        put(0, mean); put(1, sd); put(2, mn); put(3, mx); put(4, acf1);
        put(5, a.y ? sqrt(se / (double)N) : prior_nan());
        put(6, (double)sat / (double)N);
    } else {
        // classes in groups of PRIOR_CLASS_GROUP, one walk over the rows per group (one walk for the compiled shapes up to 16
        // classes): the group's counts stay in registers (every index below is a compile-time one)
        const int O = a.O;
        double ls = 0.0, conf = 0.0;
        long long hits = 0, sat = 0;
        for (int k0 = 0; k0 < O; k0 += PRIOR_CLASS_GROUP) {
            int cnt[PRIOR_CLASS_GROUP];
#pragma unroll
            for (int j = 0; j < PRIOR_CLASS_GROUP; ++j) cnt[j] = 0;
            for (int r = 0; r < N; ++r) {
                const float* p = f + (size_t)r * O * n;
                float best = p[0];
                int arg = 0;
                for (int k = 1; k < O; ++k) {
                    const float pk = p[(size_t)k * n];
                    if (pk > best) { best = pk; arg = k; }                            // first index wins a tie (np.argmax)
                }
#pragma unroll
                for (int j = 0; j < PRIOR_CLASS_GROUP; ++j) cnt[j] += arg == k0 + j;
                if (k0 > 0) continue;                                                 // the other statistics: the first walk's
                conf += (double)best;
                sat += (double)best > 1.0 - a.eps ? 1 : 0;
                if (a.y) {
                    const int label = (int)a.y[(size_t)r * a.ys];
                    hits += label == arg;
                    ls += label >= 0 && label < O ? -log((double)p[(size_t)label * n]) : prior_nan();    // no such class: undefined
                }
            }
            // integer counts over the same N: two shares compare as their counts do
#pragma unroll
            for (int j = 0; j < PRIOR_CLASS_GROUP; ++j)
                if (k0 + j < O) put(PRIOR_CLS_FIXED + k0 + j, (double)cnt[j] / (double)N);
        }
        put(0, a.y ? (double)hits / (double)N : prior_nan());
        put(1, a.y ? ls / (double)N : prior_nan());
        put(2, conf / (double)N);
        put(3, (double)sat / (double)N);
    }
}

// T(y): the statistics of the data that have a counterpart (the others NaN); one thread, the per-draw arithmetic
template <bool REG>
__global__ void prior_target_kernel(const float* y, int ys, int N, int O, double* t_obs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n_stats = REG ? PRIOR_REG_STATS : PRIOR_CLS_FIXED + O;
    for (int j = 0; j < n_stats; ++j) t_obs[j] = prior_nan();
    if (!y) return;
    if constexpr (REG) {
        prior_series_stats([&](int r) { return (double)y[(size_t)r * ys]; }, N, t_obs, t_obs + 1, t_obs + 2, t_obs + 3, t_obs + 4);
    } else {
        for (int k = 0; k < O; ++k) t_obs[PRIOR_CLS_FIXED + k] = 0.0;
        for (int r = 0; r < N; ++r) {
            const int label = (int)y[(size_t)r * ys];
            if (label >= 0 && label < O) t_obs[PRIOR_CLS_FIXED + label] += 1.0;
        }
        for (int k = 0; k < O; ++k) t_obs[PRIOR_CLS_FIXED + k] /= (double)N;
    }
}

// stage e: one work-group per statistic j over its draws t[j][.]: thread k takes the draws k, k + 256, ..., so the order of
// every double sum is fixed by n
struct PriorStat {
    const double* t;            // [n_stats][n]
    long long n;
    const double* t_obs;        // [n_stats] T(y), NaN where the data has no counterpart
    double *mean, *sd;          // [n_stats] each
    long long *n_greater, *n_equal, *n_defined;
};

__global__ void __launch_bounds__(PRIOR_THREADS) prior_stat_kernel(const PriorStat a) {
    __shared__ double shd[PRIOR_THREADS];
    __shared__ long long shi[PRIOR_THREADS];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double* x = a.t + (size_t)j * a.n;
    const double to = a.t_obs[j];
    long long nd = 0, ng = 0, ne = 0;
    double s = 0.0;
    for (long long i = tid; i < a.n; i += PRIOR_THREADS) {
        const double v = x[i];
        if (v != v) continue;
        ++nd; ng += v > to; ne += v == to;
        s += v;
    }
    nd = wg_sum<PRIOR_THREADS>(shi, nd); ng = wg_sum<PRIOR_THREADS>(shi, ng); ne = wg_sum<PRIOR_THREADS>(shi, ne);
    const double m = wg_sum<PRIOR_THREADS>(shd, s) / (double)nd;
    double c = 0.0;
    for (long long i = tid; i < a.n; i += PRIOR_THREADS) {
        const double v = x[i];
        if (v != v) continue;
        c += (v - m) * (v - m);
    }
    c = wg_sum<PRIOR_THREADS>(shd, c);
    if (tid == 0) {
        a.mean[j] = m; a.sd[j] = sqrt(c / (double)nd);
        a.n_greater[j] = ng; a.n_equal[j] = ne; a.n_defined[j] = nd;
    }
}
