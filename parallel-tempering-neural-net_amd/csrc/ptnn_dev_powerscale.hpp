// ptnn_dev_powerscale.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn, after ptnn_dev_elpd.hpp
// and ptnn_dev_lfo.hpp; not a stand-alone header): power-scaling sensitivity of the sampled chains (ptnn_powerscale,
// include/ptnn.h).
//   1. powerscale_loglik_kernel / powerscale_prior_kernel: the two components per distinct vector, double, fixed order.
//   2. powerscale_smooth_kernel: one work-group per (component, alpha); psis_reduce with its EMIT hook gives the smoothed log
//      weight of every body entry and tail position, summed per distinct vector and normalised.
//   3. powerscale_keys_kernel / powerscale_gather_kernel + powerscale_sort_lds_kernel / powerscale_sort_step_kernel: per
//      quantity the 64-bit words (pred_key(value) << 32 | distinct index) in ascending order -- a segmented bitonic sort, LDS
//      tiles of PS_SORT_TILE words and global steps above that.  The order is a function of the words only.
//   4. powerscale_distance_kernel: one work-group per (quantity, perturbation); prefix sums of the base and perturbed weights in
//      sorted order, the two gap sums on the CDF and the survival side, and the moments.
// No atomics on doubles, no order that depends on scheduling: thread t owns sorted positions [t * per, (t + 1) * per), sums them
// in order, and partials meet in fixed trees.  Nothing here writes chain state, tapes, counters or trace rows.

constexpr int PS_THREADS = 256;           // 4 waves
constexpr int PS_SORT_TILE = 4096;        // words per LDS tile: 32 KiB, so that five work-groups share a CU's LDS
constexpr int PS_MAX_DISTINCT = 65536;    // include/ptnn.h: PTNN_POWERSCALE_MAX_DISTINCT
constexpr int PS_GATHER_TILE = 64;        // vectors x parameters per transposed tile

// 1a. acc[u] += ll[r][u] over the rows of a block, r ascending: the whole sum runs from 0 in row order whatever the blocks are
__global__ void __launch_bounds__(PS_THREADS) powerscale_loglik_kernel(const double* ll, int nrows, int U, double* acc) {
    const int u = blockIdx.x * PS_THREADS + threadIdx.x;
    if (u >= U) return;
    double s = acc[u];
    for (int r = 0; r < nrows; ++r) s += ll[(size_t)r * U + u];
    acc[u] = s;
}

// 1b. prior_likelihood (REG:207-221, CLS:224-230) in double from the fp32 w and eta: one wave per distinct vector, lanes over the
// parameters (p = lane, lane + 64, ...), then the fixed butterfly
struct PsPrior {
    const float* base;
    const long long* run_off;
    const float* eta;           // [U] (regression)
    int U, P, reg;
    double part1, inv_2sig2, nu1, nu2;
    double* out;                // [U]
};
__global__ void __launch_bounds__(PS_THREADS) powerscale_prior_kernel(const PsPrior a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int u = blockIdx.x * (PS_THREADS / WAVE) + (threadIdx.x >> 6);
    if (u >= a.U) return;                                        // the whole wave leaves
    const float* w = a.base + a.run_off[u];
    double s = 0.0;
    for (int p = lane; p < a.P; p += WAVE) { const double v = (double)w[p]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) {
        double pr = a.part1 - a.inv_2sig2 * s;
        if (a.reg) {
            const double eta = (double)a.eta[u];                 // log(tausq) = eta, 1 / tausq = exp(-eta)
            pr = pr - (1.0 + a.nu1) * eta - a.nu2 * exp(-eta);
        }
        a.out[u] = pr;
    }
}

// 2. the Pareto smoothing of lr = (alpha - 1) c_u
struct PsSmooth {
    const double* logp;         // [2][U] likelihood, prior
    const int* cnt;             // [U] multiplicities (0 = absent)
    int U, M;                   // M: tail length bound, <= ELPD_TAIL_CAP
    long long S;
    double am1[2];              // alpha - 1 of alpha_minus, alpha_plus
    double* wt;                 // [4][U] out: the normalised perturbed weights, k = 2 * component + sign
    double* tail_lw;            // [4][ELPD_TAIL_CAP] scratch
    int* tail_u;                // [4][ELPD_TAIL_CAP] scratch
    double* khat;               // [4]
    long long* tail_len;        // [4]
    int* n_live;                // [1] vectors with a multiplicity > 0
};
// psis_reduce's entries: the tail keeps (key(lw), u), so entries order by lw, then by distinct index, and none merge
struct PsSrc {
    const double* c;
    const int* cnt;
    double a, mx;
    double* wt;
    double* tail_lw;
    int* tail_u;
    static constexpr bool PAIR = true;
    static constexpr bool EMIT = true;
    __device__ __forceinline__ int count(int u) const { return cnt[u]; }
    __device__ __forceinline__ void get(int u, double& lw, double& t) const { lw = a * c[u] - mx; t = (double)u; }
    __device__ __forceinline__ unsigned long long key(double lw, double) const { return elpd_key(lw); }
    __device__ __forceinline__ unsigned long long second(double t) const { return (unsigned long long)t; }
    __device__ __forceinline__ void decode(unsigned long long k, unsigned long long v, double& lw, double& t) const {
        lw = elpd_unkey(k); t = (double)v;
    }
    __device__ __forceinline__ void emit_body(int u, double lw) const { wt[u] = (double)cnt[u] * exp(lw); }
    __device__ __forceinline__ void emit_tail(long long j, double t, double lw) const { tail_lw[j] = lw; tail_u[j] = (int)t; }
};

__global__ void __launch_bounds__(ELPD_THREADS) powerscale_smooth_kernel(const PsSmooth a) {
    extern __shared__ __align__(16) unsigned char ps_lds[];
    ElpdShared& sh = *reinterpret_cast<ElpdShared*>(ps_lds);
    unsigned long long* tval = reinterpret_cast<unsigned long long*>(ps_lds + LFO_TVAL_OFFSET);
    const int tid = threadIdx.x, k = blockIdx.x;
    const double* c = a.logp + (size_t)(k >> 1) * a.U;
    const double am1 = a.am1[k & 1];
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double* wt = a.wt + (size_t)k * a.U;
    double* tail_lw = a.tail_lw + (size_t)k * ELPD_TAIL_CAP;
    int* tail_u = a.tail_u + (size_t)k * ELPD_TAIL_CAP;
    double mn = INF, mx = -INF;
    long long live = 0;
    for (int u = tid; u < a.U; u += ELPD_THREADS) {
        wt[u] = 0.0;
        if (a.cnt[u] == 0) continue;
        ++live;
        const double v = am1 * c[u];
        mn = fmin(mn, v); mx = fmax(mx, v);
    }
    block_min_max(sh, mn, mx);
    live = wg_sum<ELPD_THREADS>(reinterpret_cast<long long*>(sh.r0), live);
    const PsSrc src{c, a.cnt, am1, mx, wt, tail_lw, tail_u};
    double e, khat;
    long long T;
    psis_reduce(sh, tval, src, a.U, a.S, a.M, &e, &khat, &T);
    __syncthreads();
    // smoothed (khat finite): the weight of a tail vector is the sum over its positions, which are consecutive
    if (isfinite(khat)) {
        for (long long j = tid; j < T; j += ELPD_THREADS) {
            const int u = tail_u[j];
            if (j > 0 && tail_u[j - 1] == u) continue;
            double s = 0.0;
            for (long long i = j; i < T && tail_u[i] == u; ++i) s += exp(tail_lw[i]);
            wt[u] = s;
        }
    }
    __syncthreads();
    double part = 0.0;
    for (int u = tid; u < a.U; u += ELPD_THREADS) part += wt[u];
    const double total = wg_sum<ELPD_THREADS>(reinterpret_cast<double*>(sh.r0), part);
    for (int u = tid; u < a.U; u += ELPD_THREADS) wt[u] = wt[u] / total;
    if (tid == 0) {
        a.khat[k] = khat;
        a.tail_len[k] = T;
        if (k == 0) *a.n_live = (int)live;
    }
}

// 3a. the sort words of a block of quantities: keys[q][k], k < npow; absent vectors and the padding sort last
__device__ __forceinline__ unsigned long long ps_word(float v, int u, int U, const int* cnt) {
    if (u >= U || cnt[u] == 0) return ~0ull;
    return ((unsigned long long)pred_key(v) << 32) | (unsigned)u;
}
// quantities that lie [quantity][vector] already: predict_fwd's outputs, eta (f32), or the likelihood component (f64 -> f32)
struct PsKeys {
    const float* v32;           // [nq][U], or null
    const double* v64;          // [U] (nq == 1)
    const int* cnt;
    int U, npow;
    unsigned long long* keys;   // [nq][npow]
};
__global__ void __launch_bounds__(PS_THREADS) powerscale_keys_kernel(const PsKeys a) {
    const int k = blockIdx.x * PS_THREADS + threadIdx.x, q = blockIdx.y;
    if (k >= a.npow) return;
    float v = 0.0f;
    if (k < a.U) v = a.v32 ? a.v32[(size_t)q * a.U + k] : (float)a.v64[k];
    a.keys[(size_t)q * a.npow + k] = ps_word(v, k, a.U, a.cnt);
}
// the weights: vectors lie [vector][parameter]; a 64 x 64 tile is read along the parameters and written along the vectors
// (transposed through LDS, one pad column: no bank conflict either way)
struct PsGather {
    const float* base;
    const long long* run_off;
    const int* cnt;
    int U, npow, p0, nq;        // parameters [p0, p0 + nq)
    unsigned long long* keys;
};
__global__ void __launch_bounds__(PS_THREADS) powerscale_gather_kernel(const PsGather a) {
    __shared__ float tile[PS_GATHER_TILE][PS_GATHER_TILE + 1];
    const int u0 = blockIdx.x * PS_GATHER_TILE, q0 = blockIdx.y * PS_GATHER_TILE;
    const int col = threadIdx.x & 63, row4 = threadIdx.x >> 6;
    for (int i = 0; i < PS_GATHER_TILE / 4; ++i) {
        const int ul = i * 4 + row4, u = u0 + ul, q = q0 + col;
        tile[ul][col] = (u < a.U && q < a.nq) ? a.base[a.run_off[u] + a.p0 + q] : 0.0f;
    }
    __syncthreads();
    for (int i = 0; i < PS_GATHER_TILE / 4; ++i) {
        const int ql = i * 4 + row4, q = q0 + ql, u = u0 + col;
        if (q < a.nq && u < a.npow) a.keys[(size_t)q * a.npow + u] = ps_word(tile[col][ql], u, a.U, a.cnt);
    }
}

// 3b. bitonic sort of every quantity's npow words, ascending.  Word g of a quantity is compared with g ^ stride, ascending where
// (g & size) == 0.  Strides below the tile run in LDS: merge sizes size_first .. size_last (doubling), each from stride
// min(size, tile) / 2 down to 1; the strides >= tile of a size run first, one powerscale_sort_step_kernel launch each.
__global__ void __launch_bounds__(PS_THREADS) powerscale_sort_lds_kernel(unsigned long long* keys, int npow, int tile, int size_first,
                                                                        int size_last) {
    __shared__ unsigned long long s[PS_SORT_TILE];
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * tile;                            // word of the quantity blockIdx.y
    unsigned long long* seg = keys + (size_t)blockIdx.y * npow + g0;
    for (int i = tid; i < tile; i += PS_THREADS) s[i] = seg[i];
    __syncthreads();
    for (int size = size_first; size <= size_last; size <<= 1) {
        for (int stride = min(size, tile) >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < tile / 2; t += PS_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = ((g0 + i) & size) == 0;
                const unsigned long long ki = s[i], kj = s[j];
                if ((ki > kj) == up) { s[i] = kj; s[j] = ki; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < tile; i += PS_THREADS) seg[i] = s[i];
}
__global__ void __launch_bounds__(PS_THREADS) powerscale_sort_step_kernel(unsigned long long* keys, int npow, int size, int stride) {
    const int t = blockIdx.x * PS_THREADS + threadIdx.x;
    if (t >= npow / 2) return;
    unsigned long long* seg = keys + (size_t)blockIdx.y * npow;
    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
    const bool up = (i & size) == 0;
    const unsigned long long ki = seg[i], kj = seg[j];
    if ((ki > kj) == up) { seg[i] = kj; seg[j] = ki; }
}

// 4. distance and moments of one (quantity, perturbation)
struct PsDist {
    const unsigned long long* keys;   // [nq][npow] sorted
    const int* cnt;                   // [U]
    const double* wt;                 // [4][U] normalised perturbed weights
    const int* n_live;
    int U, npow, q0, Q;               // the block's first quantity, all quantities
    double M;                         // occurrences: the base weight of u is c_u / M
    double* dist;                     // [4][Q]
    double* mean;                     // [4][Q]
    double* sd;                       // [4][Q]
    double* base_mean;                // [Q]
    double* base_sd;                  // [Q]
};
__device__ __forceinline__ double ps_h(double a, double l2m) { return a > 0.0 ? a * (log2(a) - l2m) : 0.0; }

struct PsDistShared {
    double red[PS_THREADS];
    double cp[PS_THREADS], cq[PS_THREADS];        // chunk sums, then their inclusive prefixes
};
// the gap sums of one side: position r of the side is sorted position r (CDF) or n - 1 - r with the value negated (survival);
// P_r, Q_r = the weights cumulated through r; sum over r < n - 1 of b_r [h(P, m) + h(Q, m)] and of b_r (P + Q)
__device__ double ps_side(PsDistShared& sh, const unsigned long long* seg, const PsDist& a, const double* wt, int n, int per, bool rev) {
    const int tid = threadIdx.x;
    const int r0 = min(tid * per, n), r1 = min(r0 + per, n);
    double sp = 0.0, sq = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int u = (int)(unsigned)seg[rev ? n - 1 - r : r];
        sp += (double)a.cnt[u] / a.M; sq += wt[u];
    }
    __syncthreads();
    sh.cp[tid] = sp; sh.cq[tid] = sq;
    __syncthreads();
    wg_incl_scan<PS_THREADS>(sh.cp, sh.cq, tid);                 // inclusive scan of the chunk sums: a fixed tree, 8 steps
    double P = tid ? sh.cp[tid - 1] : 0.0, Q = tid ? sh.cq[tid - 1] : 0.0, num = 0.0, den = 0.0;   // exclusive prefixes
    for (int r = r0; r < r1 && r < n - 1; ++r) {
        const unsigned long long w0 = seg[rev ? n - 1 - r : r], w1 = seg[rev ? n - 2 - r : r + 1];
        const int u = (int)(unsigned)w0;
        P += (double)a.cnt[u] / a.M; Q += wt[u];
        const double x0 = (double)pred_unkey((unsigned)(w0 >> 32)), x1 = (double)pred_unkey((unsigned)(w1 >> 32));
        const double b = rev ? x0 - x1 : x1 - x0;
        const double l2m = log2(0.5 * (P + Q));
        num += b * (ps_h(P, l2m) + ps_h(Q, l2m));
        den += b * (P + Q);
    }
    num = wg_sum<PS_THREADS>(sh.red, num);
    den = wg_sum<PS_THREADS>(sh.red, den);
    return num / den;
}

__global__ void __launch_bounds__(PS_THREADS) powerscale_distance_kernel(const PsDist a) {
    __shared__ PsDistShared sh;
    const int tid = threadIdx.x, q = blockIdx.x, k = blockIdx.y;
    const unsigned long long* seg = a.keys + (size_t)q * a.npow;
    const double* wt = a.wt + (size_t)k * a.U;
    const int n = *a.n_live;
    const int per = (n + PS_THREADS - 1) / PS_THREADS;
    const int r0 = min(tid * per, n), r1 = min(r0 + per, n);
    // moments, two passes in sorted order: base (c_u / M) and perturbed weights
    double mb = 0.0, mw = 0.0;
    for (int r = r0; r < r1; ++r) {
        const unsigned long long w = seg[r];
        const int u = (int)(unsigned)w;
        const double x = (double)pred_unkey((unsigned)(w >> 32));
        mb += (double)a.cnt[u] / a.M * x; mw += wt[u] * x;
    }
    mb = wg_sum<PS_THREADS>(sh.red, mb);
    mw = wg_sum<PS_THREADS>(sh.red, mw);
    double vb = 0.0, vw = 0.0;
    for (int r = r0; r < r1; ++r) {
        const unsigned long long w = seg[r];
        const int u = (int)(unsigned)w;
        const double x = (double)pred_unkey((unsigned)(w >> 32));
        vb += (double)a.cnt[u] / a.M * ((x - mb) * (x - mb)); vw += wt[u] * ((x - mw) * (x - mw));
    }
    vb = wg_sum<PS_THREADS>(sh.red, vb);
    vw = wg_sum<PS_THREADS>(sh.red, vw);
    // the distance: 0 when every value is the same (no gap), else the larger of the two sides
    double d = 0.0;
    if (n > 1 && (seg[0] >> 32) != (seg[n - 1] >> 32) &&
        pred_unkey((unsigned)(seg[0] >> 32)) != pred_unkey((unsigned)(seg[n - 1] >> 32))) {      // (-0 and +0 are one value)
        const double d2a = ps_side(sh, seg, a, wt, n, per, false);
        const double d2b = ps_side(sh, seg, a, wt, n, per, true);
        const double d2 = fmax(d2a, d2b);
        d = d2 > 0.0 ? sqrt(d2) : 0.0;
    }
    if (tid == 0) {
        const size_t o = (size_t)k * a.Q + a.q0 + q;
        a.dist[o] = d; a.mean[o] = mw; a.sd[o] = sqrt(vw);
        if (k == 0) { a.base_mean[a.q0 + q] = mb; a.base_sd[a.q0 + q] = sqrt(vb); }
    }
}
