// ptnn_dev_uncertainty.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// predictive uncertainty split into its two parts (ptnn_uncertainty, include/ptnn.h).
//   a. + b. as ptnn_calibration: distinct_samples (run-length pass, a regression's with the eta compare), the per-shape
//      predict_forward_kernel; the pooled mean and the votes are predict_reduce_kernel's (ptnn_dev_select.hpp), unchanged.
//   c. unc_entropy_kernel: one work-group per data row of a classification; H_u = -sum_k p log p of every distinct sample in
//      double from the fp32 probabilities, terms added in class order; (float)H_u to an image [rows][U] that predict_reduce_kernel
//      and scatter_samples read; the expected entropy (1/S) sum c_u H_u.
//      unc_variance_kernel: one work-group per (row, output) column of a regression; the variance of f over the samples, centred
//      on predict_reduce_kernel's mean: the range of f, then the squares.
//      unc_noise_kernel: one work-group; (1/S) sum c_u exp(eta_u).
// Every sum over samples is a 128-bit fixed-point sum of terms in [0, 1] (Fix128; ptnn_dev_elpd.hpp: fix_add), scaled by a bound
// (log K; the squared range of the column; the largest exp(eta)): integer addition, so a result depends on the multiset of
// samples only -- not on their order, on how repeats are grouped or on the row block.  No atomics; nothing accumulates across
// work-groups.  fp64 throughout after f.  Nothing here writes chain state, tapes, counters or trace rows.

// T = 4 waves.  The loop body is K double-precision logs (software: some tens of fp64 VALU instructions each, no LDS, few registers
// live across them), so a wave is bound by the fp64 pipe and nothing is gained from more waves per work-group; 256 threads keep
// the reduction at 4 KiB of LDS and eight levels and let several rows share a CU (CALIB_THREADS, for the same reasons).
constexpr int UNC_THREADS = 256;

struct UncShared { unsigned long long r0[UNC_THREADS], r1[UNC_THREADS]; };
__device__ void unc_min_max(UncShared& sh, double& mn, double& mx) {
    wg_min_max<UNC_THREADS>(reinterpret_cast<double*>(sh.r0), reinterpret_cast<double*>(sh.r1), mn, mx);
}

// The mean of a fixed-point sum over the S samples, sum / (S 2^62): the tree of wg_fix_sum, then the integer quotient and remainder
// of the 128-bit sum by S (long division; sum <= S 2^62, so the high word lies below S and the quotient fits 64 bits) before
// anything is rounded.  c copies of one term t give the quotient t itself: one vector c times has the bits of the vector once.
__device__ double unc_fix_mean(UncShared& sh, Fix128 a, long long S) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh.r0[tid] = a.lo; sh.r1[tid] = a.hi;
    __syncthreads();
    wg_fix_tree<UNC_THREADS>(sh.r0, sh.r1);
    const unsigned long long lo = sh.r0[0], d = (unsigned long long)S;
    unsigned long long rem = sh.r1[0] % d, q = 0;
    __syncthreads();
    for (int b = 63; b >= 0; --b) {                            // rem < S < 2^31: the shift cannot overflow
        rem = (rem << 1) | ((lo >> b) & 1ull);
        q <<= 1;
        if (rem >= d) { rem -= d; q |= 1ull; }
    }
    return ((double)q + (double)rem / (double)d) * 0x1p-62;
}

struct UncEntropy {
    const float* fx;            // [nrows * K][U] class probabilities of the block (predict_forward_kernel layout)
    const int* cnt;             // [U] multiplicities (0 = absent)
    int U, K, row0;             // row0: global index of the block's first row
    long long S;
    double log_k;               // log K, the bound of an entropy over K classes (0 with one class)
    float* img;                 // [nrows][U] (float)H_u of the block, or null
    double* entropy_mean;       // [n_rows] at row0 + blockIdx.x
};

__global__ void __launch_bounds__(UNC_THREADS) unc_entropy_kernel(const UncEntropy a) {
    __shared__ UncShared sh;
    const int tid = threadIdx.x, r = blockIdx.x;
    const float* p = a.fx + (size_t)r * a.K * a.U;
    Fix128 acc{0, 0};
    for (int u = tid; u < a.U; u += UNC_THREADS) {
        // the K loads of a sample are coalesced across the work-group: samples are contiguous in a column
        double h = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const float pf = p[(size_t)k * a.U + u];
            if (pf > 0.0f) {                                   // 0 log 0 = 0
                const double pd = (double)pf;
                h = __dadd_rn(h, __dmul_rn(pd, log(pd)));      // product and sum rounded separately: no contraction into an fma
            }
        }
        const double H = 0.0 - h;
        if (a.img) a.img[(size_t)r * a.U + u] = (float)H;
        fix_add(acc, a.log_k > 0.0 ? H / a.log_k : 0.0, (unsigned)a.cnt[u]);
    }
    const double mean = unc_fix_mean(sh, acc, a.S);
    if (tid == 0) a.entropy_mean[a.row0 + r] = a.log_k * mean;
}

struct UncVariance {
    const float* fx;            // [ncols][U] outputs of the block, a column per (row, output)
    const int* cnt;             // [U]
    int U, col0;                // col0: global index of the block's first column
    long long S;
    const double* mean;         // [n_rows * O] predict_reduce_kernel's, read at col0 + blockIdx.x
    double* var;                // [n_rows * O] at col0 + blockIdx.x
};

__global__ void __launch_bounds__(UNC_THREADS) unc_variance_kernel(const UncVariance a) {
    __shared__ UncShared sh;
    const int tid = threadIdx.x, col = blockIdx.x;
    const float* f = a.fx + (size_t)col * a.U;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    // pass 1: the range of f over the samples present
    double fmn = INF, fmx = -INF;
    for (int u = tid; u < a.U; u += UNC_THREADS) {
        if (a.cnt[u] == 0) continue;
        const double fv = (double)f[u];
        fmn = fmin(fmn, fv); fmx = fmax(fmx, fv);
    }
    unc_min_max(sh, fmn, fmx);
    const double R = fmx - fmn;
    if (!(R > 0.0)) {                                          // uniform over the work-group: one value, no spread
        if (tid == 0) a.var[a.col0 + col] = 0.0;
        return;
    }
    // pass 2: the squares, centred on the column's mean
    const double centre = a.mean[a.col0 + col], R2 = R * R;
    Fix128 acc{0, 0};
    for (int u = tid; u < a.U; u += UNC_THREADS) {
        const unsigned c = (unsigned)a.cnt[u];
        if (c == 0) continue;
        const double d = (double)f[u] - centre;
        fix_add(acc, __dmul_rn(d, d) / R2, c);
    }
    const double share = unc_fix_mean(sh, acc, a.S);
    if (tid == 0) a.var[a.col0 + col] = R2 * share;
}

// one work-group: out[0] = (1/S) sum c_u exp(eta_u) over the samples present
__global__ void __launch_bounds__(UNC_THREADS) unc_noise_kernel(int U, const float* eta, const int* cnt, long long S, double* out) {
    __shared__ UncShared sh;
    const int tid = threadIdx.x;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double unused = INF, emx = -INF;
    for (int u = tid; u < U; u += UNC_THREADS)
        if (cnt[u] != 0) emx = fmax(emx, exp((double)eta[u]));
    unc_min_max(sh, unused, emx);
    Fix128 acc{0, 0};
    for (int u = tid; u < U; u += UNC_THREADS) {
        const unsigned c = (unsigned)cnt[u];
        if (c != 0) fix_add(acc, exp((double)eta[u]) / emx, c);
    }
    const double share = unc_fix_mean(sh, acc, S);
    if (tid == 0) out[0] = emx > 0.0 ? emx * share : 0.0;
}
