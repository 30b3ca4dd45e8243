// ptnn_dev_ale_reduce.hpp -- part of ptnn_analysis.hip alone (textually included there, inside namespace ptnn, after
// ptnn_dev_select.hpp), whose object holds them: the shape-independent kernels of accumulated local effects (ptnn_dev_ale.hpp).
// Every sum below is taken in double in the stated ascending order with __dadd_rn / __dmul_rn, and a mean is sum / count, so that
// numpy float64 in the same order gives the same bits.

// The bins of the call: term t < A has K bins from offset t * K, pair q = t - A has KK = K2 * K2 cells from A * K + q * KK.
__device__ __forceinline__ int ale_bin_offset(int t, int A, int K, int KK) { return t < A ? t * K : A * K + (t - A) * KK; }

// per distinct vector u, term t and output o: the local effects of a block of rows added in ascending row order, in double, into
// the accumulator of each row's bin (cell), onto what the earlier blocks left -- the sum of a bin is the same whatever the block
// size.  One thread per (u, t, o), reads coalesced along u; the bin index is wave-uniform; a run of rows in one bin stays in a register.
struct AleBins {
    const float* fx;            // [nrows * T * O][U]
    const int* bins;            // [all rows][T]
    int U, T, O, A, K, KK;
    int row0, nrows;
    double* acc;                // [A * K + Q * KK][O][U], zeroed by the caller before the first block
};

__global__ void __launch_bounds__(PRED_THREADS) ale_bins_kernel(const AleBins r) {
    const int ublocks = (r.U + PRED_THREADS - 1) / PRED_THREADS;
    const int u = (int)(blockIdx.x % ublocks) * PRED_THREADS + threadIdx.x, to = (int)(blockIdx.x / ublocks);
    if (u >= r.U) return;
    const int t = to / r.O, o = to % r.O;
    const int off = ale_bin_offset(t, r.A, r.K, r.KK);
    const float* f = r.fx + (size_t)to * r.U + u;
    const size_t stride = (size_t)r.T * r.O * r.U;
    int cur = -1;
    double s = 0.0;
    for (int n = 0; n < r.nrows; ++n) {
        const int b = r.bins[(size_t)(r.row0 + n) * r.T + t];
        if (b != cur) {
            if (cur >= 0) r.acc[((size_t)(off + cur) * r.O + o) * r.U + u] = s;
            cur = b;
            s = r.acc[((size_t)(off + cur) * r.O + o) * r.U + u];
        }
        s = __dadd_rn(s, (double)f[n * stride]);
    }
    if (cur >= 0) r.acc[((size_t)(off + cur) * r.O + o) * r.U + u] = s;
}

// the rows of every bin and cell, once per call: a thread per bin counts the rows of its term that fall in it
struct AleCount {
    const int* bins;            // [n_rows][T]
    int n_rows, T, A, K, KK, NB;
    int* count;                 // [NB]
};

__global__ void __launch_bounds__(PRED_THREADS) ale_count_kernel(const AleCount r) {
    const int nb = blockIdx.x * PRED_THREADS + threadIdx.x;
    if (nb >= r.NB) return;
    const int t = nb < r.A * r.K ? nb / r.K : r.A + (nb - r.A * r.K) / r.KK;
    const int b = nb - ale_bin_offset(t, r.A, r.K, r.KK);
    int c = 0;
    for (int n = 0; n < r.n_rows; ++n) c += r.bins[(size_t)n * r.T + t] == b ? 1 : 0;
    r.count[nb] = c;
}

// per distinct vector u and (a, o): the bin means m, the accumulated curve g, its count-weighted mean c, ALE32 = fp32(g - c) at
// the K + 1 edges, and range = max_k ALE32 - min_k ALE32 (pd_range_kernel's rule).  g is walked twice: once for c, once for the curve.
struct AleCurve {
    const double* acc;          // [A * K][O][U]
    const int* count;           // [A * K]
    int U, A, K, O;
    double n_total;
    float* ale32;               // [A * (K + 1) * O][U]
    float* range;               // [A * O][U]
};

__global__ void __launch_bounds__(PRED_THREADS) ale_curve_kernel(const AleCurve r) {
    const int ublocks = (r.U + PRED_THREADS - 1) / PRED_THREADS;
    const int u = (int)(blockIdx.x % ublocks) * PRED_THREADS + threadIdx.x, ao = (int)(blockIdx.x / ublocks);
    if (u >= r.U) return;
    const int ai = ao / r.O, o = ao % r.O, K = r.K;
    const double* p = r.acc + ((size_t)ai * K * r.O + o) * r.U + u;
    const int* cnt = r.count + ai * K;
    const size_t stride = (size_t)r.O * r.U;
    double g = 0.0, s = 0.0;
    for (int k = 0; k < K; ++k) {
        const double n = (double)cnt[k];
        g = __dadd_rn(g, cnt[k] > 0 ? p[k * stride] / n : 0.0);
        s = __dadd_rn(s, __dmul_rn(n, g));
    }
    const double c = s / r.n_total;
    float* out = r.ale32 + ((size_t)ai * (K + 1) * r.O + o) * r.U + u;
    g = 0.0;
    float v = (float)__dadd_rn(g, -c), mx = v, mn = v;
    out[0] = v;
    for (int k = 0; k < K; ++k) {
        g = __dadd_rn(g, cnt[k] > 0 ? p[k * stride] / (double)cnt[k] : 0.0);
        v = (float)__dadd_rn(g, -c);
        out[(k + 1) * stride] = v;
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
    }
    r.range[(size_t)ao * r.U + u] = (float)((double)mx - (double)mn);
}

// per distinct vector u and (q, o): the cell means D, their double running sum h, the two accumulated main effects A and B of h,
// g2 = h - A - B, its count-weighted mean, ALE2_32 = fp32(g2 - mean) at the (K2 + 1)^2 edge pairs, and inter = the count-weighted
// RMS of ALE2_32 at the cells' upper corners.  h lives in a plane of the thread's own in global memory (coalesced along u):
// work[k * E2 + m] for k, m >= 1; the border k = 0 or m = 0, where h = 0, holds A[k] at [k * E2] and B[m] at [m].
struct AleSurface {
    const double* acc;          // [Q * KK][O][U]
    const int* count;           // [Q * KK], cell (k - 1) * K2 + (m - 1)
    int U, Q, K2, O;
    double n_total;
    double* work;               // [Q * E2 * E2 * O][U]
    float* ale2;                // [Q * E2 * E2 * O][U]
    float* inter;               // [Q * O][U]
};

__global__ void __launch_bounds__(PRED_THREADS) ale2_surface_kernel(const AleSurface r) {
    const int ublocks = (r.U + PRED_THREADS - 1) / PRED_THREADS;
    const int u = (int)(blockIdx.x % ublocks) * PRED_THREADS + threadIdx.x, qo = (int)(blockIdx.x / ublocks);
    if (u >= r.U) return;
    const int q = qo / r.O, o = qo % r.O, K2 = r.K2, E2 = K2 + 1, KK = K2 * K2;
    const size_t stride = (size_t)r.O * r.U;
    const double* p = r.acc + ((size_t)q * KK * r.O + o) * r.U + u;
    const int* cnt = r.count + q * KK;
    double* w = r.work + ((size_t)q * E2 * E2 * r.O + o) * r.U + u;
    float* out = r.ale2 + ((size_t)q * E2 * E2 * r.O + o) * r.U + u;
    const auto N = [&](int k, int m) { return cnt[(k - 1) * K2 + (m - 1)]; };
    const auto h = [&](int k, int m) { return k == 0 || m == 0 ? 0.0 : w[(size_t)(k * E2 + m) * stride]; };
    // h[k, m] = h[k - 1, m] + (the running sum of D[k, 1 .. m])
    for (int k = 1; k <= K2; ++k) {
        double run = 0.0;
        for (int m = 1; m <= K2; ++m) {
            const int n = N(k, m);
            run = __dadd_rn(run, n > 0 ? p[(size_t)((k - 1) * K2 + (m - 1)) * stride] / (double)n : 0.0);
            w[(size_t)(k * E2 + m) * stride] = __dadd_rn(h(k - 1, m), run);
        }
    }
    // A[k] = A[k - 1] + (sum_m N(k, m) (h[k, m] - h[k - 1, m])) / n^j_k, and B[m] likewise along k
    double a = 0.0;
    for (int k = 1; k <= K2; ++k) {
        double s = 0.0;
        int nk = 0;
        for (int m = 1; m <= K2; ++m) {
            s = __dadd_rn(s, __dmul_rn((double)N(k, m), __dadd_rn(h(k, m), -h(k - 1, m))));
            nk += N(k, m);
        }
        a = __dadd_rn(a, nk > 0 ? s / (double)nk : 0.0);
        w[(size_t)(k * E2) * stride] = a;
    }
    double b = 0.0;
    for (int m = 1; m <= K2; ++m) {
        double s = 0.0;
        int nm = 0;
        for (int k = 1; k <= K2; ++k) {
            s = __dadd_rn(s, __dmul_rn((double)N(k, m), __dadd_rn(h(k, m), -h(k, m - 1))));
            nm += N(k, m);
        }
        b = __dadd_rn(b, nm > 0 ? s / (double)nm : 0.0);
        w[(size_t)m * stride] = b;
    }
    const auto g2 = [&](int k, int m) {
        const double ak = k == 0 ? 0.0 : w[(size_t)(k * E2) * stride], bm = m == 0 ? 0.0 : w[(size_t)m * stride];
        return __dadd_rn(__dadd_rn(h(k, m), -ak), -bm);
    };
    double s = 0.0;
    for (int k = 1; k <= K2; ++k)
        for (int m = 1; m <= K2; ++m) s = __dadd_rn(s, __dmul_rn((double)N(k, m), g2(k, m)));
    const double c = s / r.n_total;
    double sq = 0.0;
    for (int k = 0; k <= K2; ++k)
        for (int m = 0; m <= K2; ++m) {
            const float v = (float)__dadd_rn(g2(k, m), -c);
            out[(size_t)(k * E2 + m) * stride] = v;
            if (k >= 1 && m >= 1) sq = __dadd_rn(sq, __dmul_rn((double)N(k, m), __dmul_rn((double)v, (double)v)));
        }
    r.inter[(size_t)qo * r.U + u] = (float)sqrt(sq / r.n_total);
}
