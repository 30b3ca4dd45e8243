// ptnn_dev_convergence.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// convergence diagnostics of sampled traces: split-R-hat, split-ESS (ptnn_convergence, include/ptnn.h).
//
// The estimator is classic split-R-hat / split-ESS (BDA3 sections 11.4-11.5) with Geyer's initial monotone sequence, in the
// index arithmetic DESIGN.md section 12 spells out (and tests/convergence_ref.py restates in float64 numpy).  A quantity q (a
// weight or a scalar trace column) has C selected chains of n >= 4 draws; each chain is split into its first and last h = n / 2
// draws (the middle draw of an odd n is dropped): M = 2C split chains.  Draws are fp32; means, centring, products and every sum
// are double.  Four stages, the host loop in ptnn_analysis.hip: ptnn_convergence drives them over blocks of quantities:
//   1. conv_gather_kernel: one work-group per (chain, tile of 64 quantities) gathers the chain's rows (trace rows resolved as
//      ptnn_predict resolves them, trace_vector_offset; a tile is 64 consecutive floats of a row when the quantities are), writes
//      the centred split chains x[q][j][i] in double through an LDS transpose, and the split means, sum of squares, chain sums.
//      conv_gather_kernel<true> reads a double series instead (the rank-normalised series of ptnn_dev_rank.hpp), same arithmetic.
//   2. conv_moments_kernel: W, var+, r_hat, the pooled mean / variance, and the state of every ESS sequence.
//   3. conv_lags_kernel: sum_i x_i x_{i+t} for a block of lags over the open quantities -- 64 quantities x 64 lags x one chain
//      per work-group, the series staged in LDS in tiles of 32 draws, 16 consecutive lags per thread on a register window (FP64
//      FMA), a chain's two halves in one FMA chain.  conv_step_kernel (one wave per quantity, a lane per sequence) adds the
//      chains' sums in chain order into the combined sum (per-chain sums are kept for the per-chain ESS), feeds the block's
//      rho_t to the pair loop, committing each pair with the monotone edit as a running minimum; the host launches the next,
//      twice as long, block only for the quantities with a sequence still open.  Every sum is formed in the same order whatever
//      the block of lags, the block of quantities or the tile, so the result is that of evaluating all lags.
//   4. conv_finish_kernel: tau, ess, r_hat, the NaN / inf cases.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int CONV_THREADS = 256;        // gather and lag kernels: 4 waves
constexpr int CONV_TILE = 64;            // quantities per work-group (a lane each)
constexpr int CONV_LT = 16;              // consecutive lags per thread of conv_lags_kernel
constexpr int CONV_LAG_TILE = CONV_LT * (CONV_THREADS / WAVE);   // 64 lags per work-group
constexpr int CONV_ROWS = 32;            // draws per LDS tile of conv_lags_kernel
constexpr int CONV_MAX_LAGS = 512;       // longest block of lags the host launches (8 lag tiles)

// the state of one ESS sequence (the combined one of a quantity, or one chain's): the pair loop in flight and its partial sum
struct ConvSeq {
    double W, vplus;            // mean s_j^2 and var+ of the sequence's split chains
    double even, odd;           // the pair of the loop's latest iteration (initially rho[0] = 1, rho[1])
    double pend;                // rho_{t+1} while rho_{t+2} is awaited
    double sum;                 // sum of rho[0 ..] over the committed pairs, after the monotone edit
    double prevP;               // the last committed pair's sum (after the edit)
    int t, open, npairs, max_t;
};

struct ConvGather {
    // trace source
    const float* pos_w;         // d_pos_w [Rl][cap][PW]
    const float* scal;          // d_scal [Rl][cap][TR_COUNT]
    const int* replicas;        // [C] local replica indices
    int cap, PW, step0, thin, compact;
    // host source: draws [C][n][Qh]
    const float* draws;
    int Qh, host;
    const int* qcol;            // [nq] column of each quantity of the block: >= 0 a vector element (host: a draws column), < 0 scalar -1 - col
    int nq, C, n, h;
    double* x;                  // [nq][2C][h] centred split chains
    double* smean;              // [nq][2C] split-chain means
    double* ssq;                // [nq][2C] sum of squared deviations of each split chain
    double* csum;               // [nq][C] sum of the chain's n draws
    double* cm2;                // [nq][C] sum of squared deviations of the chain's n draws from their mean
    int* error;                 // a compact row referring to a row not resident (internal error)
    const double* series;       // conv_gather_kernel<true>: a double series [C][n][Qh] in place of the fp32 sources (ptnn_dev_rank.hpp)
};

__device__ __forceinline__ float conv_load(const ConvGather& a, int c, int i, int col, int* err) {
    if (a.host) return a.draws[((size_t)c * a.n + i) * a.Qh + col];
    const long long rep = a.replicas[c];
    const int step = a.step0 + i * a.thin;
    if (col < 0) return a.scal[(rep * a.cap + step % a.cap) * TR_COUNT + (-1 - col)];
    int src;
    return a.pos_w[trace_vector_offset(a.scal, rep, a.cap, a.PW, step, a.compact, err, &src) + col];
}
// the draw in double: the fp32 draw widened, or (SERIES) an element of the double series, which is never rounded to fp32
template <bool SERIES> __device__ __forceinline__ double conv_value(const ConvGather& a, int c, int i, int col, int* err) {
    if constexpr (SERIES) return a.series[((size_t)c * a.n + i) * a.Qh + col];
    else return (double)conv_load(a, c, i, col, err);
}

template <bool SERIES = false> __global__ void __launch_bounds__(CONV_THREADS) conv_gather_kernel(const ConvGather a) {
    constexpr int NW = CONV_THREADS / WAVE;
    __shared__ double stage[CONV_TILE][CONV_TILE + 1];      // [quantity][draw] of a chunk of 64 draws: the transposed store
    __shared__ double red[3][NW][CONV_TILE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int c = blockIdx.x, k0 = blockIdx.y * CONV_TILE, k = k0 + lane;
    const bool live = k < a.nq;
    const int col = a.qcol[live ? k : k0];
    const int n = a.n, h = a.h, M = 2 * a.C;
    // pass 1: sums of the first half, the second half and the middle draw
    double s1 = 0.0, s2 = 0.0, sm = 0.0;
    for (int i = wave; i < n; i += NW) {
        const double v = conv_value<SERIES>(a, c, i, col, a.error);
        if (i < h) s1 += v; else if (i >= n - h) s2 += v; else sm += v;
    }
    red[0][wave][lane] = s1; red[1][wave][lane] = s2; red[2][wave][lane] = sm;
    __syncthreads();
    s1 = red[0][0][lane]; s2 = red[1][0][lane]; sm = red[2][0][lane];
    for (int w = 1; w < NW; ++w) { s1 += red[0][w][lane]; s2 += red[1][w][lane]; sm += red[2][w][lane]; }
    const double m1 = s1 / h, m2 = s2 / h, cs = s1 + s2 + sm, mc = cs / n;
    __syncthreads();
    // pass 2: centre, sum the squares, store the split chains through the LDS transpose (64 consecutive doubles per quantity)
    double q1 = 0.0, q2 = 0.0, qc = 0.0;
    for (int i0 = 0; i0 < n; i0 += CONV_TILE) {
        for (int r = wave; r < CONV_TILE && i0 + r < n; r += NW) {
            const int i = i0 + r;
            const double v = conv_value<SERIES>(a, c, i, col, a.error);
            double d = 0.0;
            if (i < h) { d = v - m1; q1 = fma(d, d, q1); }
            else if (i >= n - h) { d = v - m2; q2 = fma(d, d, q2); }
            const double e = v - mc;
            qc = fma(e, e, qc);
            stage[lane][r] = d;
        }
        __syncthreads();
        for (int idx = tid; idx < CONV_TILE * CONV_TILE; idx += CONV_THREADS) {
            const int kk = idx / CONV_TILE, r = idx % CONV_TILE, i = i0 + r;
            if (k0 + kk >= a.nq || i >= n) continue;
            int j = -1, ii = 0;
            if (i < h) { j = 2 * c; ii = i; }
            else if (i >= n - h) { j = 2 * c + 1; ii = i - (n - h); }
            if (j >= 0) a.x[((size_t)(k0 + kk) * M + j) * h + ii] = stage[kk][r];
        }
        __syncthreads();
    }
    red[0][wave][lane] = q1; red[1][wave][lane] = q2; red[2][wave][lane] = qc;
    __syncthreads();
    if (wave == 0 && live) {
        for (int w = 1; w < NW; ++w) { q1 += red[0][w][lane]; q2 += red[1][w][lane]; qc += red[2][w][lane]; }
        a.smean[(size_t)k * M + 2 * c] = m1; a.smean[(size_t)k * M + 2 * c + 1] = m2;
        a.ssq[(size_t)k * M + 2 * c] = q1; a.ssq[(size_t)k * M + 2 * c + 1] = q2;
        a.csum[(size_t)k * a.C + c] = cs; a.cm2[(size_t)k * a.C + c] = qc;
    }
}

struct ConvMoments {
    const double *smean, *ssq, *csum, *cm2;
    int nq, C, n, h, NS;        // NS: sequences per quantity (1 combined + C per-chain, or 1)
    ConvSeq* seq;               // [nq][NS]
    double* pmean;              // [nq] pooled mean, variance (ddof 1)
    double* pvar;
};

// W and var+ of the split chains j0 .. j0 + m - 1 of quantity k
__device__ void conv_wb(const ConvMoments& a, int k, int j0, int m, double* W, double* vplus) {
    const int M = 2 * a.C, h = a.h;
    double w = 0.0, mm = 0.0;
    for (int j = j0; j < j0 + m; ++j) { w += a.ssq[(size_t)k * M + j] / (h - 1); mm += a.smean[(size_t)k * M + j]; }
    w /= m; mm /= m;
    double b = 0.0;
    for (int j = j0; j < j0 + m; ++j) { const double d = a.smean[(size_t)k * M + j] - mm; b = fma(d, d, b); }
    *W = w;
    *vplus = w * (h - 1) / h + b / (m - 1);
}

__global__ void __launch_bounds__(CONV_THREADS) conv_moments_kernel(const ConvMoments a) {
    const long long g = (long long)blockIdx.x * CONV_THREADS + threadIdx.x;
    if (g >= (long long)a.nq * a.NS) return;
    const int k = (int)(g / a.NS), s = (int)(g % a.NS);
    ConvSeq q{};
    if (s == 0) conv_wb(a, k, 0, 2 * a.C, &q.W, &q.vplus);
    else conv_wb(a, k, 2 * (s - 1), 2, &q.W, &q.vplus);
    q.even = 1.0; q.t = 1; q.open = 1; q.max_t = -1;
    a.seq[g] = q;
    if (s == 0) {                                       // pooled over every selected draw (the middle ones included)
        const double N = (double)a.C * a.n;
        double t = 0.0;
        for (int c = 0; c < a.C; ++c) t += a.csum[(size_t)k * a.C + c];
        const double mean = t / N;
        double m2 = 0.0;
        for (int c = 0; c < a.C; ++c) {
            const double d = a.csum[(size_t)k * a.C + c] / a.n - mean;
            m2 += a.cm2[(size_t)k * a.C + c] + a.n * d * d;
        }
        a.pmean[k] = mean;
        a.pvar[k] = m2 / (N - 1);
    }
}

struct ConvLags {
    const double* x;            // [nq][2C][h]
    int C, h;
    const int* open;            // [n_open] block-local indices of the quantities still open
    int n_open;
    const int* full;            // [nq] the combined sums are needed (all chains)
    const int* chain_open;      // [nq][C] chain c's own sequence is open, or null (no per-chain ESS)
    int t0;                     // lags [t0, t0 + nl), nl = 64 gridDim.y
    double* chain;              // [n_open][C][nl] per chain (its two halves in one FMA chain): sum_i x_i x_{i+t}
};

// grid (tiles of 64 open quantities, tiles of 64 lags, chains): a work-group skips a chain none of its quantities needs
__global__ void __launch_bounds__(CONV_THREADS) conv_lags_kernel(const ConvLags a) {
    constexpr int AS = CONV_ROWS + 1, BS = CONV_ROWS + CONV_LAG_TILE + 1;
    __shared__ double A[CONV_TILE * AS];               // x_i       of the tile's draws  [quantity][i]
    __shared__ double B[CONV_TILE * BS];               // x_{i + t} for the work-group's lags  [quantity][i + t - tl0]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int kb = blockIdx.x * CONV_TILE, kl = kb + lane, c = blockIdx.z;
    const int tl0 = a.t0 + blockIdx.y * CONV_LAG_TILE;   // the work-group's first lag
    const int lo = wave * CONV_LT;                       // this wave's lags: tl0 + lo .. + CONV_LT - 1
    const int h = a.h, M = 2 * a.C, nl = gridDim.y * CONV_LAG_TILE;
    const bool live = kl < a.n_open;
    const int q = live ? a.open[kl] : 0;
    const bool need = live && (a.full[q] || (a.chain_open && a.chain_open[(size_t)q * a.C + c]));
    if (!__syncthreads_or(need)) return;                 // no quantity of the tile needs this chain
    double acc[CONV_LT];
#pragma unroll
    for (int l = 0; l < CONV_LT; ++l) acc[l] = 0.0;
    for (int half = 0; half < 2; ++half) {
        const int j = 2 * c + half;
        for (int i0 = 0; i0 < h - tl0; i0 += CONV_ROWS) {   // draws i >= h - tl0 have no partner at any of these lags
            for (int idx = tid; idx < CONV_TILE * CONV_ROWS; idx += CONV_THREADS) {
                const int kk = idx / CONV_ROWS, ii = idx % CONV_ROWS, i = i0 + ii;
                double v = 0.0;
                if (kb + kk < a.n_open && i < h) v = a.x[((size_t)a.open[kb + kk] * M + j) * h + i];
                A[kk * AS + ii] = v;
            }
            for (int idx = tid; idx < CONV_TILE * (BS - 1); idx += CONV_THREADS) {
                const int kk = idx / (BS - 1), ii = idx % (BS - 1), i = i0 + tl0 + ii;
                double v = 0.0;                                    // a partner past the series' end contributes 0
                if (kb + kk < a.n_open && i < h) v = a.x[((size_t)a.open[kb + kk] * M + j) * h + i];
                B[kk * BS + ii] = v;
            }
            __syncthreads();
            const double* Ar = A + lane * AS;
            const double* Br = B + lane * BS + lo;
            double win[CONV_LT];
#pragma unroll
            for (int l = 0; l < CONV_LT; ++l) win[l] = Br[l];
#pragma unroll
            for (int ii = 0; ii < CONV_ROWS; ++ii) {       // acc[l] += x_i x_{i + tl0 + lo + l}, i ascending
                const double xi = Ar[ii];
#pragma unroll
                for (int l = 0; l < CONV_LT; ++l) acc[l] = fma(xi, win[l], acc[l]);
#pragma unroll
                for (int l = 0; l < CONV_LT - 1; ++l) win[l] = win[l + 1];
                if (ii + 1 < CONV_ROWS) win[CONV_LT - 1] = Br[ii + CONV_LT];
            }
            __syncthreads();
        }
    }
    if (need) {
        double* dst = a.chain + ((size_t)kl * a.C + c) * nl + (tl0 - a.t0 + lo);    // 16 consecutive doubles per lane
#pragma unroll
        for (int l = 0; l < CONV_LT; ++l) dst[l] = acc[l];
    }
}

// one lag of a sequence: rho_t fed to the pair loop (the monotone edit folded in as each pair is committed)
__device__ void conv_commit(ConvSeq& s) {
    double P = s.even + s.odd;                  // rho[t-1] + rho[t] of the pair being committed
    if (s.npairs > 0 && P > s.prevP) P = s.prevP;       // both entries become (previous pair) / 2: their sum is the previous sum
    s.sum += P;
    s.prevP = P;
    ++s.npairs;
}

__device__ void conv_feed(ConvSeq& s, int lag, double rho, int h) {
    if (lag == 0) return;
    if (lag == 1) {
        s.odd = rho;                            // rho[0] = 1 (even), rho[1]; t = 1
    } else if (lag == s.t + 1) {
        s.pend = rho;
        return;
    } else {                                    // lag t + 2: one iteration of the pair loop; the pair before it is inside rho[0 .. max_t]
        conv_commit(s);
        s.even = s.pend;
        s.odd = rho;
        s.t += 2;
    }
    if (!(s.t < h - 3 && s.even + s.odd > 0.0)) { s.open = 0; s.max_t = s.t - 2; }
}

struct ConvStep {
    const double* chain;        // [n_open][C][nl]
    const int* open;            // [n_open]
    int n_open, C, h, NS, t0, nl, n_lags, Q, q0;
    ConvSeq* seq;               // [nq][NS]
    int* full;                  // [nq] in: this block's combined sums were computed; out: the next block's are needed
    int* chain_open;            // [nq][C] out, or null
    int* any_open;              // [nq] out: the quantity needs another block
    double* rho_out;            // [n_lags][Q] raw combined rho_t, or null
};

__global__ void __launch_bounds__(WAVE) conv_step_kernel(const ConvStep a) {
    __shared__ double comb[CONV_MAX_LAGS];
    __shared__ int any;
    const int kl = blockIdx.x, q = a.open[kl], lane = threadIdx.x;
    const bool full = a.full[q];
    const double* ch = a.chain + (size_t)kl * a.C * a.nl;
    // the combined sums: the chains' in chain order (lanes over the lags, each lag's chain sums contiguous in c-major rows)
    if (full)
        for (int tl = lane; tl < a.nl; tl += WAVE) {
            double S = 0.0;
            for (int c = 0; c < a.C; ++c) S += ch[(size_t)c * a.nl + tl];
            comb[tl] = S;
        }
    if (lane == 0) any = 0;
    __syncthreads();
    const int M = 2 * a.C;
    for (int s = lane; s < a.NS; s += WAVE) {
        ConvSeq st = a.seq[(size_t)q * a.NS + s];
        const bool is_comb = s == 0;
        if (is_comb ? full : st.open) {
            const double norm = is_comb ? (double)M * a.h : 2.0 * a.h;
            for (int tl = 0; tl < a.nl; ++tl) {
                const int t = a.t0 + tl;
                if (t >= a.h || (!st.open && !(is_comb && t < a.n_lags))) break;
                const double S = is_comb ? comb[tl] : ch[(size_t)(s - 1) * a.nl + tl];
                const double rho = 1.0 - (st.W - S / norm) / st.vplus;
                if (is_comb && a.rho_out && t < a.n_lags) a.rho_out[(size_t)t * a.Q + a.q0 + q] = rho;
                if (st.open) conv_feed(st, t, rho, a.h);
            }
            a.seq[(size_t)q * a.NS + s] = st;
        }
        const int next = a.t0 + a.nl;
        if (is_comb) {
            const int f = st.open || (next < a.n_lags && next < a.h);
            a.full[q] = f;
            if (f) any = 1;
        } else {
            a.chain_open[(size_t)q * a.C + (s - 1)] = st.open;
            if (st.open) any = 1;
        }
    }
    __syncthreads();
    if (lane == 0) a.any_open[q] = any;
}

struct ConvFinish {
    const ConvSeq* seq;         // [nq][NS]
    const double *pmean, *pvar;
    int nq, NS, C, h, Q, q0;
    double *mean, *var, *r_hat, *ess, *ess_chain;       // [Q] (ess_chain [C][Q]); any may be null
    int* trunc_lag;
};

__global__ void __launch_bounds__(CONV_THREADS) conv_finish_kernel(const ConvFinish a) {
    const long long g = (long long)blockIdx.x * CONV_THREADS + threadIdx.x;
    if (g >= (long long)a.nq * a.NS) return;
    const int k = (int)(g / a.NS), s = (int)(g % a.NS), Qg = a.q0 + k;
    const ConvSeq st = a.seq[g];
    const int M = s == 0 ? 2 * a.C : 2;
    const double Mh = (double)M * a.h;
    // rho[max_t + 1]: the last iteration's even, where the loop wrote it (even + odd >= 0) or the tail rule sets it (even > 0)
    const double tail = (st.even > 0.0 || st.even + st.odd >= 0.0) ? st.even : 0.0;
    double tau = -1.0 + 2.0 * st.sum + tail;
    const double floor_ = 1.0 / log10(Mh);
    if (floor_ > tau) tau = floor_;
    double ess = Mh / tau;
    if (!(st.vplus != 0.0)) ess = __builtin_nan("");
    if (s == 0) {
        if (a.ess) a.ess[Qg] = ess;
        if (a.trunc_lag) a.trunc_lag[Qg] = st.max_t;
        if (a.r_hat) a.r_hat[Qg] = st.vplus == 0.0 ? __builtin_nan("") : (st.W == 0.0 ? __builtin_inf() : sqrt(st.vplus / st.W));
        if (a.mean) a.mean[Qg] = a.pmean[k];
        if (a.var) a.var[Qg] = a.pvar[k];
    } else if (a.ess_chain) {
        a.ess_chain[(size_t)(s - 1) * a.Q + Qg] = ess;
    }
}
