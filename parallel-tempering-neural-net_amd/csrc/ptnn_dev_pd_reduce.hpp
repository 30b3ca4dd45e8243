// ptnn_dev_pd_reduce.hpp -- part of ptnn_analysis.hip alone (textually included there, inside namespace ptnn, after
// ptnn_dev_select.hpp), whose object holds them: the shape-independent kernels of partial dependence (ptnn_dev_pd.hpp).

// per distinct vector u and column c = (a * G + k) * O + o of a row: ICE summed over the rows of a block in ascending order, in
// double, onto what the earlier blocks left -- the sum over all rows is the same whatever the block size.  One thread per (u, c),
// reads coalesced along u.  After the last block: PD32 = the mean over the n_total rows as fp32.
struct PdRows {
    const float* fx;            // [nrows * AGO][U]
    int U, AGO, nrows, last;
    double n_total;
    double* acc;                // [AGO][U], zeroed by the caller before the first block
    float* pd32;                // [AGO][U]
};

__global__ void __launch_bounds__(PRED_THREADS) pd_rows_kernel(const PdRows r) {
    const int ublocks = (r.U + PRED_THREADS - 1) / PRED_THREADS;
    const int u = (int)(blockIdx.x % ublocks) * PRED_THREADS + threadIdx.x, c = (int)(blockIdx.x / ublocks);
    if (u >= r.U) return;
    const size_t k = (size_t)c * r.U + u;
    double s = r.acc[k];
    const float* f = r.fx + k;
    const size_t stride = (size_t)r.AGO * r.U;
    for (int n = 0; n < r.nrows; ++n) s += (double)f[n * stride];
    r.acc[k] = s;
    if (r.last) r.pd32[k] = (float)(s / r.n_total);
}

// per distinct vector u and (a, o): range = max_k PD32 - min_k PD32, the difference formed in double (exact) and rounded once
struct PdRange {
    const float* pd32;          // [A * G * O][U]
    int U, A, G, O;
    float* range;               // [A * O][U]
};

__global__ void __launch_bounds__(PRED_THREADS) pd_range_kernel(const PdRange r) {
    const int ublocks = (r.U + PRED_THREADS - 1) / PRED_THREADS;
    const int u = (int)(blockIdx.x % ublocks) * PRED_THREADS + threadIdx.x, ao = (int)(blockIdx.x / ublocks);
    if (u >= r.U) return;
    const int ai = ao / r.O, o = ao % r.O;
    const float* p = r.pd32 + ((size_t)ai * r.G * r.O + o) * r.U + u;
    const size_t stride = (size_t)r.O * r.U;
    float mx = p[0], mn = p[0];
    for (int k = 1; k < r.G; ++k) {
        const float v = p[k * stride];
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
    }
    r.range[(size_t)ao * r.U + u] = (float)((double)mx - (double)mn);
}

// per column c = (a * G + k) * O + o, one work-group: the weighted mean over the distinct vectors of the double row means, a
// fixed summation order for a given U
struct PdMean {
    const double* acc;          // [AGO][U]
    const int* cnt;             // [U]
    int U;
    double n_total;
    long long M;
    double* mean;               // [AGO]
};

__global__ void __launch_bounds__(PRED_THREADS) pd_mean_kernel(const PdMean r) {
    __shared__ double buf[PRED_THREADS];
    const int tid = threadIdx.x, c = blockIdx.x;
    double s = 0.0;
    for (int u = tid; u < r.U; u += PRED_THREADS) s += (double)r.cnt[u] * (r.acc[(size_t)c * r.U + u] / r.n_total);
    s = wg_sum<PRED_THREADS>(buf, s);
    if (tid == 0) r.mean[c] = s / (double)r.M;
}
