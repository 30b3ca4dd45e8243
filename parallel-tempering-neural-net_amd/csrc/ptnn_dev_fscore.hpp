// ptnn_dev_fscore.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn, after ptnn_dev_elpd.hpp and
// ptnn_dev_calibration.hpp; not a stand-alone header): forecast verification (ptnn_forecast_score, include/ptnn.h; DESIGN.md
// section 27).  The k-step predictive distribution of a noisy recursive forecast is the mixture (1/M) sum_i c_i N(mu_{i,r,k},
// tau_i^2) over the trajectories of ptnn_forecast, mu the sigmoid output before the step's noise: the input form of the
// calibration kernels, which score a block's (origin, step) columns as their "rows".
//   a. + b. as ptnn_forecast: the selection and the per-shape forecast_forward_kernel, which also stores mu (ForecastFwd::mu).
//   c. calib_tau_kernel, calib_row_kernel, calib_pair_kernel, calib_finish_kernel (ptnn_dev_calibration.hpp) with fx := mu and
//      y := the truth column; a column without truth (NaN) is skipped before any arithmetic.
//      fscore_logscore_kernel: one work-group per column, log (1/M) sum c N(y; mu, tau^2) with the exact maximum of ll.
//      fscore_energy_first_kernel: one work-group per origin, (1/M) sum c |Y_i - y| and the bound B of the pair term.
//      fscore_energy_kernel: the pair term of the energy score, origins x the triangle of (i-tile, j-tile) pairs.
//      fscore_energy_finish_kernel: es = first term - pair term.
// Every sum over trajectories is a 128-bit fixed-point sum of terms in [0, 1] (Fix128), scaled by a bound formed from exact
// extremes; the pair kernel adds its work-groups' integer sums with integer atomics of 32-bit limbs.  No floating-point atomic.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int FSCORE_THREADS = CALIB_THREADS;          // 4 waves; also the tile of the energy pair kernel
constexpr int FSCORE_JGROUP = 8;                       // j-paths whose squared distances a lane accumulates at a time
constexpr int FSCORE_ENERGY_LDS = 64 * 1024;           // dynamic LDS of the pair kernel at most: + 5 KiB static, two work-groups per CU

__device__ __forceinline__ bool fscore_missing(float y) { return !(y == y); }

struct FscoreLog {
    const float* mu;            // [ncols of the block][U]
    const float* eta;           // [U]
    const int* cnt;             // [U] multiplicities (0 = absent)
    const float* y;             // truth of global column n at y[n]
    int U, col0;                // col0: global index of the block's first column
    long long S;
    double* log_score;          // [all columns], at col0 + blockIdx.x
};

// log (1/S) sum c exp(ll), ll = section 13's pointwise log-likelihood: the exact maximum, then the fixed-point sum of
// c exp(ll - max) in [0, 1] -- the operations of elpd_reduce_kernel's lppd
__global__ void __launch_bounds__(FSCORE_THREADS) fscore_logscore_kernel(const FscoreLog a) {
    __shared__ CalibShared sh;
    const int tid = threadIdx.x, n = a.col0 + blockIdx.x;
    const float yf = a.y[n];
    if (fscore_missing(yf)) return;                    // uniform: before any barrier
    const double y = (double)yf;
    const float* f = a.mu + (size_t)blockIdx.x * a.U;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    const auto ll = [&](int u) {
        const double eta = (double)a.eta[u], d = y - (double)f[u];
        return -0.5 * (ELPD_LOG_2PI + eta) - 0.5 * (d * d) * exp(-eta);
    };
    double mx = -INF;
    for (int u = tid; u < a.U; u += FSCORE_THREADS)
        if (a.cnt[u] != 0) mx = fmax(mx, ll(u));
    mx = wg_max<FSCORE_THREADS>(reinterpret_cast<double*>(sh.r0), mx);
    Fix128 fe{0, 0};
    for (int u = tid; u < a.U; u += FSCORE_THREADS) {
        const unsigned c = (unsigned)a.cnt[u];
        if (c != 0) fix_add(fe, exp(ll(u) - mx), c);
    }
    const double se = wg_fix_sum<FSCORE_THREADS>(sh.r0, sh.r1, fe);
    if (tid == 0) a.log_score[n] = mx + log(se / (double)a.S);
}

struct FscoreEnergy {
    const float* fx;            // [nr * hz][U] noisy paths of the block: column rl * hz + k (noise off: the mean paths)
    const int* cnt;             // [U]
    const float* y;             // [n_origins][hz] truth
    const int* klist;           // [n_origins][hz] the steps with finite truth of every origin, ascending, first nk[r] entries
    const int* nk;              // [n_origins] |K_r|
    int U, hz, r0;              // r0: global index of the block's first origin
    long long S;
    double* term1;              // [n_origins] (1/S) sum c |Y_i - y|
    double* bound;              // [n_origins] B = sqrt(sum_k (max_i - min_i)^2) >= every |Y_i - Y_j|
    int n_tiles, JW;            // ceil(U / FSCORE_THREADS); j-paths staged at a time (a power of two in [FSCORE_JGROUP, FSCORE_THREADS])
    unsigned long long* limbs;  // [n_origins][4] sum c_i c_j floor(|Y_i - Y_j| / B 2^62), 32 bits per word (zeroed by the caller)
};

// grid: x = the origins of the block
__global__ void __launch_bounds__(FSCORE_THREADS) fscore_energy_first_kernel(const FscoreEnergy a) {
    __shared__ CalibShared sh;
    const int tid = threadIdx.x, rl = blockIdx.x, r = a.r0 + rl;
    const int nK = a.nk[r];
    if (nK == 0) return;                               // uniform
    const int* kl = a.klist + (size_t)r * a.hz;
    const float* f = a.fx + (size_t)rl * a.hz * a.U;
    const float* yr = a.y + (size_t)r * a.hz;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    // the exact extremes of every step: B^2 = sum (max - min)^2, B1^2 = sum max(|y - min|, |y - max|)^2 >= every |Y_i - y|^2
    double B2 = 0.0, B12 = 0.0;
    for (int kk = 0; kk < nK; ++kk) {
        const int k = kl[kk];
        const float* fk = f + (size_t)k * a.U;
        double mn = INF, mx = -INF;
        for (int u = tid; u < a.U; u += FSCORE_THREADS) {
            if (a.cnt[u] == 0) continue;
            const double v = (double)fk[u];
            mn = fmin(mn, v); mx = fmax(mx, v);
        }
        calib_min_max(sh, mn, mx);
        const double R = mx - mn, yk = (double)yr[k], m = fmax(fabs(yk - mn), fabs(yk - mx));
        B2 = fma(R, R, B2); B12 = fma(m, m, B12);
    }
    const double B1 = sqrt(B12);
    Fix128 fa{0, 0};
    for (int u = tid; u < a.U; u += FSCORE_THREADS) {
        const unsigned c = (unsigned)a.cnt[u];
        if (c == 0) continue;
        double d2 = 0.0;
        for (int kk = 0; kk < nK; ++kk) {
            const int k = kl[kk];
            const double d = (double)f[(size_t)k * a.U + u] - (double)yr[k];
            d2 = fma(d, d, d2);
        }
        fix_add(fa, B1 > 0.0 ? sqrt(d2) / B1 : 0.0, c);   // B1 = 0: every path is the truth, the term counts 0
    }
    const double s = wg_fix_sum<FSCORE_THREADS>(sh.r0, sh.r1, fa);
    if (tid == 0) {
        a.term1[r] = B1 > 0.0 ? B1 * (s / (double)a.S) : 0.0;
        a.bound[r] = sqrt(B2);
    }
}

// grid: x = tile pairs (ti >= tj) of the triangle, y = the origins of the block.  Lane = one i-path, read from global memory
// (coalesced over the lanes, step by step); the j-tile's paths over the |K_r| steps with truth staged in LDS, JW paths at a time
// as js[step][j], and read as wave-uniform broadcasts of FSCORE_JGROUP consecutive j.  A lane holds the running squared
// distances to those FSCORE_JGROUP paths in registers while it walks the steps.  The diagonal tile takes its full square, an
// off-diagonal one counts twice.
__global__ void __launch_bounds__(FSCORE_THREADS) fscore_energy_kernel(const FscoreEnergy a) {
    extern __shared__ __attribute__((aligned(16))) float js[];      // [nK][JW]
    __shared__ unsigned jc[FSCORE_THREADS];
    __shared__ CalibShared sh;
    const int tid = threadIdx.x, rl = blockIdx.y, r = a.r0 + rl;
    const int nK = a.nk[r];
    if (nK == 0) return;                               // uniform
    const unsigned p = blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((unsigned)ti * (unsigned)(ti + 1) / 2u > p) --ti;
    while ((unsigned)(ti + 1) * (unsigned)(ti + 2) / 2u <= p) ++ti;
    const int tj = (int)(p - (unsigned)ti * (unsigned)(ti + 1) / 2u);
    const int* kl = a.klist + (size_t)r * a.hz;
    const float* f = a.fx + (size_t)rl * a.hz * a.U;
    const int JW = a.JW;
    {
        const int u = tj * FSCORE_THREADS + tid;
        jc[tid] = u < a.U ? (unsigned)a.cnt[u] : 0u;
    }
    const int ui = ti * FSCORE_THREADS + tid;
    const bool live = ui < a.U;
    const int uc = live ? ui : a.U - 1;                // a dead lane reads a valid path and counts 0
    const unsigned ci = live ? (unsigned)a.cnt[ui] : 0u;
    const double B = a.bound[r];
    const double scale = B > 0.0 ? 0x1p62 / B : 0.0;   // B = 0: all paths are one path, every distance counts 0
    const int nj = min(FSCORE_THREADS, a.U - tj * FSCORE_THREADS);
    Fix128 acc{0, 0};
    for (int j0 = 0; j0 < nj; j0 += JW) {
        __syncthreads();                               // the previous sub-tile has been read (first pass: jc is stored)
        for (int idx = tid; idx < nK * JW; idx += FSCORE_THREADS) {
            const int kk = idx / JW, jj = idx - kk * JW;
            const int u = tj * FSCORE_THREADS + j0 + jj;
            js[idx] = u < a.U ? f[(size_t)kl[kk] * a.U + u] : 0.0f;
        }
        __syncthreads();
        const int je = min(JW, nj - j0);
        for (int jb = 0; jb < je; jb += FSCORE_JGROUP) {
            double d2[FSCORE_JGROUP];
#pragma unroll
            for (int g = 0; g < FSCORE_JGROUP; ++g) d2[g] = 0.0;
            for (int kk = 0; kk < nK; ++kk) {
                const double xi = (double)f[(size_t)kl[kk] * a.U + uc];
                const float* row = js + kk * JW + jb;
#pragma unroll
                for (int g = 0; g < FSCORE_JGROUP; ++g) {
                    const double d = xi - (double)row[g];          // JW is a multiple of FSCORE_JGROUP: inside the row
                    d2[g] = fma(d, d, d2[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < FSCORE_JGROUP; ++g) {
                if (jb + g < je) {
                    const double t = sqrt(d2[g]) * scale;
                    const unsigned long long q = t < 0x1p62 ? (unsigned long long)t : (1ull << 62);
                    const unsigned long long c = jc[j0 + jb + g];
                    const unsigned long long plo = q * c;
                    acc.lo += plo;
                    acc.hi += __umul64hi(q, c) + (acc.lo < plo ? 1ull : 0ull);
                }
            }
        }
    }
    // times c_i, twice off the diagonal: k < 2^32
    const unsigned long long k = (unsigned long long)ci * (ti == tj ? 1ull : 2ull);
    __syncthreads();
    sh.r0[tid] = acc.lo * k; sh.r1[tid] = acc.hi * k + __umul64hi(acc.lo, k);
    __syncthreads();
    wg_fix_tree<FSCORE_THREADS>(sh.r0, sh.r1);
    if (tid < 4) {
        const unsigned long long w = (tid >> 1) ? sh.r1[0] : sh.r0[0];
        const unsigned long long limb = (tid & 1) ? (w >> 32) : (w & 0xffffffffull);
        if (limb) atomicAdd(&a.limbs[(size_t)r * 4 + tid], limb);      // integer: any order gives the same sum
    }
}

// es_r = term1_r - B_r (sum / 2^62) / (2 S^2); an origin without truth keeps the NaN its outputs were filled with
__global__ void __launch_bounds__(FSCORE_THREADS) fscore_energy_finish_kernel(int n_origins, const int* nk, const unsigned long long* limbs,
                                                                              const double* term1, const double* bound, long long S,
                                                                              double* es) {
    const int r = blockIdx.x * FSCORE_THREADS + threadIdx.x;
    if (r >= n_origins || nk[r] == 0) return;
    const unsigned long long* l = limbs + (size_t)r * 4;
    unsigned long long w[4], carry = 0;
    for (int k = 0; k < 4; ++k) {
        const unsigned long long v = l[k] + carry;
        w[k] = v & 0xffffffffull;
        carry = v >> 32;
    }
    const double sum = (double)(w[3] << 32 | w[2]) * 0x1p64 + (double)(w[1] << 32 | w[0]);
    const double Sd = (double)S, B = bound[r];
    es[r] = B > 0.0 ? term1[r] - B * (sum * 0x1p-62) / (2.0 * Sd * Sd) : term1[r];
}
