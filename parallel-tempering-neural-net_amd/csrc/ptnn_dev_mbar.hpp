// ptnn_dev_mbar.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// the multistate Bennett acceptance ratio over every rung of the ladder (ptnn_mbar, include/ptnn.h).
// Items n carry U_n, b_n (stages a to d of ptnn_dev_evidence.hpp) and a weight c_n >= 0; state k has the reduced log density
// l_k(n) = g_k b_n + beta_k U_n (g_k = 0 for the prior state, whose beta is 0, else 1), N_k draws and the free energy f_k.
//   mbar_denominator_kernel  D_n = log sum_k N_k exp(f_k + l_k(n)), one lane per item, the states staged in LDS
//   mbar_free_energy_kernel  -log sum_n c_n exp(l_k(n) - D_n), one work-group per state over all items
//   mbar_pin_kernel          f_k - f_0 of the sweep, and max_k |f_k - previous f_k| into a device scalar
//   mbar_gram_kernel         M = W^T diag(c) W, W_nk = exp(f_k + l_k(n) - D_n) recomputed per tile, 64 x 64 tiles of the upper
//                            triangle over chunks of MBAR_GRAM_CHUNK items; mbar_gram_sum_kernel adds the chunks in order
//   mbar_weight_kernel       log(c_n W_n) at the target beta; mbar_weight_stats_kernel: their sum, Kish ESS and largest share
//   mbar_expect_kernel       weighted mean and population variance of the network outputs on rows x, one work-group per column
//   mbar_gather_kernel       the weight vectors of the resampled items
//   mbar_scan_kernel         the running sum of the weights over the item order, monotone; mbar_resample_kernel: systematic draws from it
// Every exp is taken relative to an exact maximum.  Every reduction runs over a fixed index order with a fixed tree and the chunk
// size is a constant, so the results depend on (U, b, c) and their order only.  Nothing here writes chain state, tapes, counters
// or trace rows.

constexpr int MBAR_THREADS = 256;          // 4 waves
constexpr int MBAR_MAX_K = 512;            // states per call (include/ptnn.h: PTNN_MBAR_MAX_STATES): 256 rungs and the prior fit; a power of two
                                           // (the work-group of mbar_pin_kernel)
constexpr int MBAR_TILE = 64;              // states per side of a Gram tile
constexpr int MBAR_GB = 32;                // items staged per step of a Gram tile
constexpr int MBAR_GRAM_CHUNK = 16384;     // items per work-group of a Gram tile (a constant: it fixes the order of the sum)
constexpr uint32_t STREAM_RESAMPLE = 7;    // the offset of ptnn_mbar's systematic resampling (counter: 0, 0, 0)

struct MbarItems {
    const double *u, *b, *c;    // [n]
    double* D;                  // [n]
    long long n;
};
struct MbarStates {
    int K;
    const double *beta, *g, *ln_n, *f;   // [K]
};

__global__ void __launch_bounds__(MBAR_THREADS) mbar_denominator_kernel(const MbarItems it, const MbarStates s) {
    __shared__ double sb[MBAR_MAX_K], sg[MBAR_MAX_K], sa[MBAR_MAX_K];
    for (int k = threadIdx.x; k < s.K; k += MBAR_THREADS) { sb[k] = s.beta[k]; sg[k] = s.g[k]; sa[k] = s.ln_n[k] + s.f[k]; }
    __syncthreads();
    const long long n = (long long)blockIdx.x * MBAR_THREADS + threadIdx.x;
    if (n >= it.n) return;
    const double u = it.u[n], b = it.b[n];
    double mx = -INFINITY;
    for (int k = 0; k < s.K; ++k) mx = fmax(mx, sa[k] + (sg[k] * b + sb[k] * u));
    double e = 0.0;
    for (int k = 0; k < s.K; ++k) e += exp(sa[k] + (sg[k] * b + sb[k] * u) - mx);
    it.D[n] = mx + log(e);
}

// state k = blockIdx.x: raw[k] = -log sum_n c_n exp(l_k(n) - D_n) over the items with c_n > 0
__global__ void __launch_bounds__(MBAR_THREADS) mbar_free_energy_kernel(const MbarItems it, const double* beta, const double* g, double* raw) {
    __shared__ double red[MBAR_THREADS];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double bk = beta[k], gk = g[k];
    double mx = -INFINITY;
    for (long long n = tid; n < it.n; n += MBAR_THREADS)
        if (it.c[n] > 0.0) mx = fmax(mx, (gk * it.b[n] + bk * it.u[n]) - it.D[n]);
    mx = wg_max<MBAR_THREADS>(red, mx);
    double e = 0.0;
    for (long long n = tid; n < it.n; n += MBAR_THREADS)
        if (it.c[n] > 0.0) e += it.c[n] * exp((gk * it.b[n] + bk * it.u[n]) - it.D[n] - mx);
    e = wg_sum<MBAR_THREADS>(red, e);
    if (tid == 0) raw[k] = -(mx + log(e));
}

// one work-group: f_k = raw_k - raw_0, *resid = max_k |f_k - previous f_k| (NaN counts as infinite)
__global__ void __launch_bounds__(MBAR_MAX_K) mbar_pin_kernel(int K, const double* raw, double* f, double* resid) {
    __shared__ double red[MBAR_MAX_K];
    const int tid = threadIdx.x;
    double d = 0.0;
    if (tid < K) {
        const double nf = raw[tid] - raw[0];
        d = fabs(nf - f[tid]);
        if (!(d == d)) d = INFINITY;
        f[tid] = nf;
    }
    d = wg_max<MBAR_MAX_K>(red, d);
    if (tid == 0) *resid = d;
}

// the upper-triangle tile pair p of nt x nt tiles, row-major: (ti, tj), ti <= tj
__device__ __host__ inline void mbar_tile_pair(int p, int nt, int* ti, int* tj) {
    int i = 0;
    while (p >= nt - i) { p -= nt - i; ++i; }
    *ti = i; *tj = i + p;
}
__device__ __host__ inline int mbar_pair_index(int ti, int tj, int nt) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }

// grid (chunks x tile pairs) in x: part[chunk][pair][64][64] = sum over the chunk's items, in item order, of c_n W_nj W_nk.
// 256 threads hold a 4 x 4 block each; MBAR_GB items are staged per step as c_n W_nj (rows) and W_nk (columns).
struct MbarGram {
    MbarItems it;
    MbarStates s;
    double* part;
};

__global__ void __launch_bounds__(MBAR_THREADS) mbar_gram_kernel(const MbarGram a) {
    __shared__ double wi[MBAR_GB][MBAR_TILE], wj[MBAR_GB][MBAR_TILE];
    __shared__ double sf[2][MBAR_TILE], sb[2][MBAR_TILE], sg[2][MBAR_TILE];
    const int tid = threadIdx.x, K = a.s.K, nt = (K + MBAR_TILE - 1) / MBAR_TILE;
    int ti, tj;
    const int npairs = nt * (nt + 1) / 2, chunk = (int)(blockIdx.x / npairs);
    mbar_tile_pair((int)(blockIdx.x % npairs), nt, &ti, &tj);
    if (tid < 2 * MBAR_TILE) {
        const int side = tid / MBAR_TILE, kk = tid % MBAR_TILE, k = (side ? tj : ti) * MBAR_TILE + kk;
        const bool in = k < K;
        sf[side][kk] = in ? a.s.f[k] : 0.0; sb[side][kk] = in ? a.s.beta[k] : 0.0; sg[side][kk] = in ? a.s.g[k] : 0.0;
    }
    __syncthreads();
    const long long n0 = (long long)chunk * MBAR_GRAM_CHUNK, n1 = n0 + MBAR_GRAM_CHUNK < a.it.n ? n0 + MBAR_GRAM_CHUNK : a.it.n;
    const int ty = tid / 16, tx = tid % 16;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (long long base = n0; base < n1; base += MBAR_GB) {
        for (int e = tid; e < MBAR_GB * MBAR_TILE; e += MBAR_THREADS) {
            const int nl = e / MBAR_TILE, kk = e % MBAR_TILE;
            const long long n = base + nl;
            double vi = 0.0, vj = 0.0;
            if (n < n1 && a.it.c[n] > 0.0) {         // an item of weight 0 adds nothing, whatever its U
                const double u = a.it.u[n], b = a.it.b[n], D = a.it.D[n], c = a.it.c[n];
                if (ti * MBAR_TILE + kk < K) vi = c * exp(sf[0][kk] + (sg[0][kk] * b + sb[0][kk] * u) - D);
                if (tj * MBAR_TILE + kk < K) vj = exp(sf[1][kk] + (sg[1][kk] * b + sb[1][kk] * u) - D);
            }
            wi[nl][kk] = vi; wj[nl][kk] = vj;
        }
        __syncthreads();
        for (int nl = 0; nl < MBAR_GB; ++nl) {
            double ra[4], rb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { ra[r] = wi[nl][ty * 4 + r]; rb[r] = wj[nl][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(ra[r], rb[c], acc[r][c]);
        }
        __syncthreads();
    }
    double* dst = a.part + (size_t)blockIdx.x * (MBAR_TILE * MBAR_TILE);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) dst[(ty * 4 + r) * MBAR_TILE + tx * 4 + c] = acc[r][c];
}

// M[j][k] = M[k][j] = the chunks of element (j, k), j <= k, added in chunk order
__global__ void __launch_bounds__(MBAR_THREADS) mbar_gram_sum_kernel(int K, int n_chunks, const double* part, double* M) {
    const int e = blockIdx.x * MBAR_THREADS + threadIdx.x;
    if (e >= K * K) return;
    const int j = e / K, k = e % K;
    if (j > k) return;
    const int nt = (K + MBAR_TILE - 1) / MBAR_TILE, npairs = nt * (nt + 1) / 2;
    const int p = mbar_pair_index(j / MBAR_TILE, k / MBAR_TILE, nt);
    const double* src = part + (size_t)p * (MBAR_TILE * MBAR_TILE) + (j % MBAR_TILE) * MBAR_TILE + k % MBAR_TILE;
    double s = 0.0;
    for (int q = 0; q < n_chunks; ++q) s += src[(size_t)q * npairs * (MBAR_TILE * MBAR_TILE)];
    M[(size_t)j * K + k] = s;
    M[(size_t)k * K + j] = s;
}

// lw_n = log c_n + b_n + beta U_n - D_n + f (f = *ft, the target's free energy); c_n = 0: -inf
__global__ void __launch_bounds__(MBAR_THREADS) mbar_weight_kernel(const MbarItems it, const double* beta, const double* ft, double* lw) {
    const long long n = (long long)blockIdx.x * MBAR_THREADS + threadIdx.x;
    if (n >= it.n) return;
    const double c = it.c[n];
    lw[n] = c > 0.0 ? log(c) + ((it.b[n] + beta[0] * it.u[n]) - it.D[n] + ft[0]) : -INFINITY;
}

// one work-group: out[0] = sum w, out[1] = (sum w)^2 / sum (w^2 / c) (the Kish ESS of the draws behind the items: item n stands
// for c_n draws of weight W_n each), out[2] = max w / sum w, w = exp(lw) = c W
__global__ void __launch_bounds__(MBAR_THREADS) mbar_weight_stats_kernel(const double* lw, const double* c, long long n, double* out) {
    __shared__ double red[MBAR_THREADS];
    const int tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0, mx = -INFINITY;
    for (long long i = tid; i < n; i += MBAR_THREADS) {
        const double w = exp(lw[i]);
        s1 += w; mx = fmax(mx, lw[i]);
        if (c[i] > 0.0) s2 += w * w / c[i];
    }
    s1 = wg_sum<MBAR_THREADS>(red, s1);
    s2 = wg_sum<MBAR_THREADS>(red, s2);
    mx = wg_max<MBAR_THREADS>(red, mx);
    if (tid == 0) { out[0] = s1; out[1] = s1 * s1 / s2; out[2] = exp(mx) / s1; }
}

// one work-group: cum[n] = w_0 + ... + w_n in item order, never decreasing (the binary search of mbar_resample_kernel needs that,
// and a tree scan does not give it in floating point): thread t adds its contiguous segment of ceil(n / 256) items in order,
// thread 0 adds the segments' totals in order, and every running sum is offset + (the segment's running sum)
__global__ void __launch_bounds__(MBAR_THREADS) mbar_scan_kernel(const double* lw, long long n, double* cum) {
    __shared__ double tot[MBAR_THREADS], offs[MBAR_THREADS];
    const int tid = threadIdx.x;
    const long long len = (n + MBAR_THREADS - 1) / MBAR_THREADS, i0 = (long long)tid * len, i1 = i0 + len < n ? i0 + len : n;
    double s = 0.0;
    for (long long i = i0; i < i1; ++i) s += exp(lw[i]);
    tot[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double o = 0.0;
        for (int t = 0; t < MBAR_THREADS; ++t) { offs[t] = o; o += tot[t]; }
    }
    __syncthreads();
    const double o = offs[tid];
    s = 0.0;
    for (long long i = i0; i < i1; ++i) { s += exp(lw[i]); cum[i] = o + s; }
}

// draw i of m takes the first item whose running sum exceeds ((u + i) / m) cum[n - 1], u = the 23-bit uniform of word 0 of
// philox4x32_10(0, 0, 0, STREAM_RESAMPLE, seed) (philox.py: resample_uniform); past the end: the last item of positive weight
__global__ void __launch_bounds__(MBAR_THREADS) mbar_resample_kernel(const double* cum, long long n, long long m, uint32_t slo, uint32_t shi,
                                                                     long long* item, double* u_out) {
    const long long i = (long long)blockIdx.x * MBAR_THREADS + threadIdx.x;
    if (i >= m) return;
    uint32_t x[4];
    philox4x32_10(0u, 0u, 0u, STREAM_RESAMPLE, slo, shi, x);
    const double u = ((double)(x[0] >> 9) + 0.5) * (1.0 / 8388608.0);
    if (i == 0) *u_out = u;
    const double t = (u + (double)i) / (double)m * cum[n - 1];
    long long lo = 0, hi = n;                      // the first index with cum > t
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo > n - 1) lo = n - 1;
    while (lo > 0 && cum[lo] == cum[lo - 1]) --lo;
    item[i] = lo;
}

// Expectations under the target weights: one work-group per (row, output) column of a block of network outputs fx [cols][U]
// (predict_forward_kernel's layout) over n items with log weights lw [n]; item i reads vector item_run[i] (null: vector i).
// Chunks of 256 items go down the wg_sum tree and are added to the column's carried sum acc[col0 + col] in order, so that the
// sum depends on the items and their order only as long as every call but the last of a column holds a multiple of 256 items.
// mean == null: acc += sum w f; else acc += sum w (f - mean)^2: the two passes of a weighted population variance.
struct MbarExpect {
    const float* fx;
    int U;
    const int* item_run;
    const double* lw;
    long long n;
    const double* mean;         // [all columns] or null
    double* acc;                // [all columns]
    int col0;
};

__global__ void __launch_bounds__(MBAR_THREADS) mbar_expect_kernel(const MbarExpect a) {
    __shared__ double red[MBAR_THREADS];
    const int col = blockIdx.x, tid = threadIdx.x;
    const float* f = a.fx + (size_t)col * a.U;
    const double m = a.mean ? a.mean[a.col0 + col] : 0.0;
    double s = a.acc[a.col0 + col];
    for (long long base = 0; base < a.n; base += MBAR_THREADS) {
        const long long i = base + tid;
        double v = 0.0;
        if (i < a.n) {
            const double w = exp(a.lw[i]), fv = (double)f[a.item_run ? a.item_run[i] : i];
            v = a.mean ? w * ((fv - m) * (fv - m)) : w * fv;
        }
        v = wg_sum<MBAR_THREADS>(red, v);
        s += v;
    }
    if (tid == 0) a.acc[a.col0 + col] = s;
}

// out[c] = acc[c] / *wsum
__global__ void __launch_bounds__(MBAR_THREADS) mbar_expect_finish_kernel(int n, const double* acc, const double* wsum, double* out) {
    const int c = blockIdx.x * MBAR_THREADS + threadIdx.x;
    if (c < n) out[c] = acc[c] / wsum[0];
}

// the weight vectors of the resampled items, [m][P]: thread (i, q) writes components 4 q .. 4 q + 3 of draw i -- a prior draw's
// (item < n_prior) as evid_prior_kernel forms them, a rung row's copied from its distinct vector
struct MbarGather {
    const long long* item;      // [m]
    long long m, n_prior;
    int P;
    float sigma;
    uint32_t slo, shi;
    const float* base;          // the rungs' vectors (null: no rung rows, host U)
    const long long* run_off;
    const int* item_run;
    float* w;                   // [m][P]
};

__global__ void __launch_bounds__(MBAR_THREADS) mbar_gather_kernel(const MbarGather a) {
    const int nq = (a.P + 3) >> 2;
    const long long j = (long long)blockIdx.x * MBAR_THREADS + threadIdx.x;
    if (j >= a.m * nq) return;
    const long long i = j / nq, it = a.item[i];
    const int q = (int)(j % nq);
    float v[4];
    if (it < a.n_prior) {
        prior_normals(q, it, a.slo, a.shi, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] *= a.sigma;
    } else {
        const float* src = a.base + a.run_off[a.item_run[it - a.n_prior]];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = 4 * q + c < a.P ? src[4 * q + c] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (4 * q + c < a.P) a.w[(size_t)i * a.P + 4 * q + c] = v[c];
}
