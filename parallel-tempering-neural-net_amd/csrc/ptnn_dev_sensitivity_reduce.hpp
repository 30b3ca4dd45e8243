// ptnn_dev_sensitivity_reduce.hpp -- part of ptnn_analysis.hip alone (textually included there, inside namespace ptnn, after
// ptnn_dev_select.hpp), whose object holds them: the shape-independent kernels of input sensitivity (ptnn_dev_sensitivity.hpp).

// per column of a block: the samples, multiplicities counted, whose gradient is > 0 and < 0.  Integer counts: exact in any order.
struct SensSign {
    const float* gx;            // [ncols][U]
    const int* cnt;             // [U]
    int U;
    long long col0;             // global index of the block's first column
    long long* pos;             // [ncols_total]
    long long* neg;
};

__global__ void __launch_bounds__(PRED_THREADS) sensitivity_sign_kernel(const SensSign r) {
    __shared__ long long psum[PRED_THREADS], nsum[PRED_THREADS];
    const int tid = threadIdx.x, col = blockIdx.x;
    const float* f = r.gx + (size_t)col * r.U;
    long long p = 0, n = 0;
    for (int u = tid; u < r.U; u += PRED_THREADS) {
        const float g = f[u];
        const int c = r.cnt[u];
        if (g > 0.0f) p += c;
        if (g < 0.0f) n += c;
    }
    psum[tid] = p;
    nsum[tid] = n;
    __syncthreads();
    wg_tree<PRED_THREADS>([&](int i, int j) { psum[i] += psum[j]; nsum[i] += nsum[j]; });
    if (tid == 0) { r.pos[r.col0 + col] = psum[0]; r.neg[r.col0 + col] = nsum[0]; }
}

// per distinct vector u and (o, i): |g| and g^2 summed over the rows of a block in ascending order, in double, onto what the
// earlier blocks left -- the sum over all rows is the same whatever the block size.  One thread per (u, oi), reads coalesced
// along u.  After the last block: a_s = the mean of |g| over the n_total rows as fp32, for the rank pass.
struct SensRows {
    const float* gx;            // [nrows * OI][U]
    int U, OI, nrows, last;
    double n_total;
    double* acc_abs;            // [OI][U], zeroed by the caller before the first block
    double* acc_sq;
    float* a32;                 // [OI][U]
};

__global__ void __launch_bounds__(PRED_THREADS) sensitivity_rows_kernel(const SensRows r) {
    const int u = blockIdx.x * PRED_THREADS + threadIdx.x, oi = blockIdx.y;
    if (u >= r.U) return;
    const size_t k = (size_t)oi * r.U + u;
    double sa = r.acc_abs[k], sq = r.acc_sq[k];
    const float* g = r.gx + k;
    const size_t stride = (size_t)r.OI * r.U;
    for (int n = 0; n < r.nrows; ++n) {
        const double v = (double)g[n * stride];
        sa += fabs(v);
        sq += v * v;
    }
    r.acc_abs[k] = sa;
    r.acc_sq[k] = sq;
    if (r.last) r.a32[k] = (float)(sa / r.n_total);
}

// per (o, i), one work-group: the weighted means over the distinct vectors of a_s and q_s (the row sums / n_total), in double, a
// fixed summation order for a given U
struct SensMean {
    const double* acc_abs;      // [OI][U]
    const double* acc_sq;
    const int* cnt;             // [U]
    int U;
    double n_total;
    long long M;
    double* abs_mean;           // [OI]
    double* sq_mean;
};

__global__ void __launch_bounds__(PRED_THREADS) sensitivity_mean_kernel(const SensMean r) {
    __shared__ double asum[PRED_THREADS], qsum[PRED_THREADS];
    const int tid = threadIdx.x, oi = blockIdx.x;
    double sa = 0.0, sq = 0.0;
    for (int u = tid; u < r.U; u += PRED_THREADS) {
        const double c = (double)r.cnt[u];
        sa += c * (r.acc_abs[(size_t)oi * r.U + u] / r.n_total);
        sq += c * (r.acc_sq[(size_t)oi * r.U + u] / r.n_total);
    }
    asum[tid] = sa;
    qsum[tid] = sq;
    __syncthreads();
    wg_tree<PRED_THREADS>([&](int i, int j) { asum[i] += asum[j]; qsum[i] += qsum[j]; });
    if (tid == 0) { r.abs_mean[oi] = asum[0] / (double)r.M; r.sq_mean[oi] = qsum[0] / (double)r.M; }
}
