// ptnn_dev_calibration.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// calibration and proper scores of the predictive distribution (ptnn_calibration, include/ptnn.h;
// DESIGN.md section 17).  A regression's predictive distribution of y on a data row is the mixture (1/S) sum_s c_s N(f_s, tau_s^2)
// over the U distinct (w, eta) samples with multiplicities c_s; per row: its PIT, mean, sd, quantiles and CRPS.
//   a. + b. as ptnn_elpd: distinct_samples (run-length pass with the eta compare), the per-shape predict_forward_kernel.
//   c. calib_tau_kernel: tau^2 = exp(eta), tau, 1 / tau of every distinct sample, once per call.
//      calib_row_kernel: one work-group per data row, the O(U) quantities and one bisection per quantile level.
//      calib_pair_kernel: the pair term of the CRPS, rows x the triangle of (i-tile, j-tile) pairs over U.
//      calib_finish_kernel: crps = first term - pair term.
// A classification's p_mean is predict_reduce_kernel's mean (ptnn_dev_select.hpp), unchanged.
// Every sum over samples is a 128-bit fixed-point sum of terms in [0, 1] (Fix128; ptnn_dev_elpd.hpp: fix_add), scaled by a bound formed
// from the row's exact extremes: integer addition, so a result depends on the multiset of samples only -- not on their order,
// on how repeats are grouped, on the tiling or on the row block.  The pair kernel adds its work-groups' integer sums with
// integer atomics (four 32-bit limbs in 64-bit words); no floating-point atomic anywhere.  fp64 throughout after f.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int CALIB_THREADS = 256;        // 4 waves; also the tile of the pair kernel (one i-sample per lane)
constexpr int CALIB_MAX_LEVELS = 16;      // include/ptnn.h: PTNN_CALIB_MAX_LEVELS
constexpr int CALIB_MAX_DISTINCT = 65536; // include/ptnn.h: PTNN_CALIB_MAX_DISTINCT
constexpr int CALIB_MAX_BISECT = 1200;    // > 1074 + 64 halvings: an interval of doubles cannot be halved more often

constexpr double CALIB_SQRT1_2 = 0.70710678118654752440;
constexpr double CALIB_1_SQRTPI = 0.56418958354775628695;

__device__ __forceinline__ double calib_Phi(double x) { return 0.5 * erfc(-x * CALIB_SQRT1_2); }
// A(m, v) = m (2 Phi(m / sqrt v) - 1) + 2 sqrt(v) phi(m / sqrt v), from rs = 1 / sqrt(2 v): both terms >= 0, A <= |m| + sqrt(2 v / pi)
__device__ __forceinline__ double calib_A(double m, double v2, double rs) {
    const double x = m * rs;
    return m * erf(x) + (v2 * rs) * CALIB_1_SQRTPI * exp(-x * x);
}

__global__ void __launch_bounds__(CALIB_THREADS) calib_tau_kernel(int U, const float* eta, double* tau2, double* tau, double* itau) {
    const int u = blockIdx.x * CALIB_THREADS + threadIdx.x;
    if (u >= U) return;
    const double t2 = exp((double)eta[u]), t = sqrt(t2);
    tau2[u] = t2; tau[u] = t; itau[u] = 1.0 / t;
}

// the storage of the block reductions over CALIB_THREADS threads (ptnn_dev_wg.hpp: wg_fix_sum, wg_min_max)
struct CalibShared { unsigned long long r0[CALIB_THREADS], r1[CALIB_THREADS]; };
__device__ void calib_min_max(CalibShared& sh, double& mn, double& mx) {
    wg_min_max<CALIB_THREADS>(reinterpret_cast<double*>(sh.r0), reinterpret_cast<double*>(sh.r1), mn, mx);
}

struct CalibRow {
    const float* fx;            // [nrows][U] network outputs of the block (predict_forward_kernel layout, n_out = 1)
    const double* tau2;         // [U]
    const double* tau;
    const double* itau;
    const int* cnt;             // [U] multiplicities (0 = absent)
    const float* y;             // target of global row n at y[n * ys]
    int ys, U, row0, n_rows;    // row0: global index of the block's first row; n_rows: of the whole request
    long long S;
    int n_levels;
    double p[CALIB_MAX_LEVELS], z[CALIB_MAX_LEVELS];
    int pair;                   // the pair term follows: term1 and pair_scale are wanted
    double* pit;                // [n_rows] each, at row0 + blockIdx.x
    double* pred_mean;
    double* pred_sd;
    double* quantiles;          // [n_levels][n_rows]
    double* term1;              // [n_rows] (1/S) sum c A(y - f, tau^2)
    double* pair_bound;         // [n_rows] B >= every A(f_s - f_t, tau_s^2 + tau_t^2) of the row
    int skip_nan;               // ptnn_forecast_score: a row whose target is NaN (no truth) is left alone, its outputs untouched
};

__global__ void __launch_bounds__(CALIB_THREADS) calib_row_kernel(const CalibRow a) {
    __shared__ CalibShared sh;
    const int tid = threadIdx.x, r = blockIdx.x, n = a.row0 + r;
    const float* f = a.fx + (size_t)r * a.U;
    const double y = (double)a.y[(size_t)n * a.ys];
    if (a.skip_nan && !(y == y)) return;                       // uniform over the work-group, before any barrier
    const double S = (double)a.S;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);

    // pass 1: the extremes of f and tau^2
    double fmn = INF, fmx = -INF, ntmx = INF, dummy = -INF;
    for (int u = tid; u < a.U; u += CALIB_THREADS) {
        if (a.cnt[u] == 0) continue;
        const double fv = (double)f[u];
        fmn = fmin(fmn, fv); fmx = fmax(fmx, fv); ntmx = fmin(ntmx, -a.tau2[u]);
    }
    calib_min_max(sh, fmn, fmx);
    calib_min_max(sh, ntmx, dummy);
    const double t2mx = -ntmx, R = fmx - fmn;
    // pass 2: pit, mean, the first CRPS term
    const double B1 = fmax(fabs(y - fmn), fabs(y - fmx)) + sqrt(2.0 * t2mx) * CALIB_1_SQRTPI;
    Fix128 fp{0, 0}, fm{0, 0}, fa{0, 0};
    for (int u = tid; u < a.U; u += CALIB_THREADS) {
        const unsigned c = (unsigned)a.cnt[u];
        if (c == 0) continue;
        const double fv = (double)f[u], d = y - fv;
        fix_add(fp, calib_Phi(d * a.itau[u]), c);
        if (R > 0.0) fix_add(fm, (fv - fmn) / R, c);
        if (a.pair) fix_add(fa, calib_A(d, 2.0 * a.tau2[u], a.itau[u] * CALIB_SQRT1_2) / B1, c);
    }
    const double pit = wg_fix_sum<CALIB_THREADS>(sh.r0, sh.r1, fp) / S;
    const double sm = wg_fix_sum<CALIB_THREADS>(sh.r0, sh.r1, fm);
    const double t1 = a.pair ? B1 * (wg_fix_sum<CALIB_THREADS>(sh.r0, sh.r1, fa) / S) : 0.0;
    double mean = R > 0.0 ? fmn + R * (sm / S) : fmn;
    mean = fmin(fmax(mean, fmn), fmx);
    // pass 3: the variance, centred on the mean
    const double D = t2mx + fmax((fmx - mean) * (fmx - mean), (mean - fmn) * (mean - fmn));
    Fix128 fv2{0, 0};
    for (int u = tid; u < a.U; u += CALIB_THREADS) {
        const unsigned c = (unsigned)a.cnt[u];
        if (c == 0) continue;
        const double d = (double)f[u] - mean;
        fix_add(fv2, (a.tau2[u] + d * d) / D, c);
    }
    const double var = D * (wg_fix_sum<CALIB_THREADS>(sh.r0, sh.r1, fv2) / S);
    if (tid == 0) {
        if (a.pit) a.pit[n] = pit;
        if (a.pred_mean) a.pred_mean[n] = mean;
        if (a.pred_sd) a.pred_sd[n] = sqrt(var);
        if (a.pair) {
            a.term1[n] = t1;
            a.pair_bound[n] = R + sqrt(4.0 * t2mx) * CALIB_1_SQRTPI;      // |m| <= R, v <= 2 max tau^2
        }
    }
    // the quantiles: F(z) = p by bisection from [min (f + tau z_p), max (f + tau z_p)]
    for (int k = 0; k < a.n_levels; ++k) {
        const double zp = a.z[k], p = a.p[k];
        double lo = INF, hi = -INF;
        for (int u = tid; u < a.U; u += CALIB_THREADS) {
            if (a.cnt[u] == 0) continue;
            const double e = (double)f[u] + a.tau[u] * zp;
            lo = fmin(lo, e); hi = fmax(hi, e);
        }
        calib_min_max(sh, lo, hi);
        double mid = lo;
        for (int it = 0; it < CALIB_MAX_BISECT; ++it) {        // every thread holds the same lo, hi: a uniform loop
            mid = 0.5 * lo + 0.5 * hi;
            if (!(mid > lo && mid < hi)) break;
            Fix128 fc{0, 0};
            for (int u = tid; u < a.U; u += CALIB_THREADS) {
                const unsigned c = (unsigned)a.cnt[u];
                if (c == 0) continue;
                fix_add(fc, calib_Phi((mid - (double)f[u]) * a.itau[u]), c);
            }
            const double F = wg_fix_sum<CALIB_THREADS>(sh.r0, sh.r1, fc) / S;
            if (F < p) lo = mid; else hi = mid;
        }
        if (tid == 0) a.quantiles[(size_t)k * a.n_rows + n] = mid;
    }
}

struct CalibPair {
    const float* fx;            // [nrows][U] of the block
    const double* tau2;         // [U]
    const int* cnt;             // [U]
    const double* pair_bound;   // [n_rows] (calib_row_kernel)
    int U, row0, r0;            // r0: first row of this launch inside the block
    int n_tiles;                // ceil(U / CALIB_THREADS)
    unsigned long long* limbs;  // [n_rows][4] sum c_s c_t floor(A / B 2^62), 32 bits per word (zeroed by the caller)
    const float* y_skip;        // ptnn_forecast_score: targets [n_rows], a row whose target is NaN is left alone; else null
};

// grid: x = tile pairs (ti >= tj) of the triangle, y = rows.  Lane = one i-sample in registers; the j-tile in LDS, read as
// wave-uniform broadcasts.  The diagonal tile takes its full square, an off-diagonal one counts twice.
__global__ void __launch_bounds__(CALIB_THREADS) calib_pair_kernel(const CalibPair a) {
    __shared__ double jf[CALIB_THREADS], jv[CALIB_THREADS];
    __shared__ unsigned jc[CALIB_THREADS];
    __shared__ CalibShared sh;
    const int tid = threadIdx.x;
    const int r = a.r0 + blockIdx.y, n = a.row0 + r;
    if (a.y_skip && !(a.y_skip[n] == a.y_skip[n])) return;     // uniform over the work-group, before any barrier
    // tile pair p -> (ti, tj), tj <= ti: p = ti (ti + 1) / 2 + tj
    const unsigned p = blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((unsigned)ti * (unsigned)(ti + 1) / 2u > p) --ti;
    while ((unsigned)(ti + 1) * (unsigned)(ti + 2) / 2u <= p) ++ti;
    const int tj = (int)(p - (unsigned)ti * (unsigned)(ti + 1) / 2u);
    const float* f = a.fx + (size_t)r * a.U;
    {
        const int u = tj * CALIB_THREADS + tid;
        const bool live = u < a.U;
        jf[tid] = live ? (double)f[u] : 0.0;
        jv[tid] = live ? a.tau2[u] : 1.0;
        jc[tid] = live ? (unsigned)a.cnt[u] : 0u;
    }
    const int ui = ti * CALIB_THREADS + tid;
    const bool live = ui < a.U;
    const double fi = live ? (double)f[ui] : 0.0;
    const double vi = live ? a.tau2[ui] : 1.0;
    const unsigned ci = live ? (unsigned)a.cnt[ui] : 0u;
    const double scale = 0x1p62 / a.pair_bound[n];
    __syncthreads();
    const int nj = min(CALIB_THREADS, a.U - tj * CALIB_THREADS);
    Fix128 acc{0, 0};
    for (int j = 0; j < nj; ++j) {
        const double v2 = 2.0 * (vi + jv[j]);
        const double A = calib_A(fi - jf[j], v2, rsqrt(v2));
        const double t = A * scale;
        const unsigned long long q = t < 0x1p62 ? (unsigned long long)t : (1ull << 62);
        const unsigned long long c = jc[j];
        const unsigned long long plo = q * c;
        acc.lo += plo;
        acc.hi += __umul64hi(q, c) + (acc.lo < plo ? 1ull : 0ull);
    }
    // times c_s, twice off the diagonal: k < 2^32
    const unsigned long long k = (unsigned long long)ci * (ti == tj ? 1ull : 2ull);
    sh.r0[tid] = acc.lo * k; sh.r1[tid] = acc.hi * k + __umul64hi(acc.lo, k);
    __syncthreads();
    wg_fix_tree<CALIB_THREADS>(sh.r0, sh.r1);
    if (tid < 4) {
        const unsigned long long w = (tid >> 1) ? sh.r1[0] : sh.r0[0];
        const unsigned long long limb = (tid & 1) ? (w >> 32) : (w & 0xffffffffull);
        if (limb) atomicAdd(&a.limbs[(size_t)n * 4 + tid], limb);     // integer: any order gives the same sum
    }
}

// crps_n = term1_n - B_n (sum / 2^62) / (2 S^2); the limbs hold at most 2^32 work-groups' 32-bit pieces each
__global__ void __launch_bounds__(CALIB_THREADS) calib_finish_kernel(int n_rows, const unsigned long long* limbs, const double* term1,
                                                                     const double* pair_bound, long long S, double* crps) {
    const int n = blockIdx.x * CALIB_THREADS + threadIdx.x;
    if (n >= n_rows) return;
    const unsigned long long* l = limbs + (size_t)n * 4;
    unsigned long long w[4], carry = 0;
    for (int k = 0; k < 4; ++k) {
        const unsigned long long v = l[k] + carry;         // < 2^64: l[k] < 2^64 - 2^32 as a sum of < 2^32 pieces below 2^32
        w[k] = v & 0xffffffffull;
        carry = v >> 32;
    }
    // (the total is below S^2 2^62 < 2^124: nothing is carried out of the top word)
    const double sum = (double)(w[3] << 32 | w[2]) * 0x1p64 + (double)(w[1] << 32 | w[0]);
    const double Sd = (double)S;
    crps[n] = term1[n] - pair_bound[n] * (sum * 0x1p-62) / (2.0 * Sd * Sd);
}
