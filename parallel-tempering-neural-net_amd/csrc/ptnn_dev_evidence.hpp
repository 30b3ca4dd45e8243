// ptnn_dev_evidence.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// the log evidence log Z of the sampled ladder (ptnn_evidence, include/ptnn.h):
// per-rung statistics of the full-data log-likelihood U(w) over each rung's draws, and the same over draws of the prior, which
// the host turns into thermodynamic-integration and stepping-stone estimates.
//   a. sample_runs_kernel (reg = 0: U needs w only) + predict_scan_kernel: the selected rows collapse into distinct vectors.
//   b. the per-shape predict_forward_kernel of ptnn_dev_predict.hpp, unchanged, on the training rows.
//   c. evid_rows_kernel: one lane per distinct vector adds its rows' terms in row order into a double -- log p_y (classification)
//      or (y - f)^2 (regression, the SSE) -- carried across row blocks, so any block size gives the same bits;
//      evid_finish_kernel turns the sum into U (and b = -log SSE for a regression).
//   d. evid_expand_kernel writes every draw's U (expanding multiplicities, chain-major), evid_rung_kernel reduces each rung:
//      mean and variance of U, log-mean-exp of d_k U with its exact maximum and the relative variance of the exp-terms; the
//      rung's ESS comes from the convergence kernels (ptnn_dev_convergence.hpp) on the same draws, laid out by evid_conv_kernel.
//   e. prior draws: evid_prior_kernel writes w = sigma z, z from Philox stream STREAM_PRIOR (counter (k / 4, draw, 0, 5)), into
//      blocks of vectors that stages b and c evaluate; evid_prior_reduce_kernel reduces over all draws per exponent a_j.
// Every reduction runs over a fixed index order with a fixed tree, so the results depend on the draws and their order only.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int EVID_THREADS = 256;          // 4 waves
constexpr int EVID_MAX_A = 4;              // prior exponents per call (include/ptnn.h: PTNN_EVIDENCE_MAX_A)
constexpr uint32_t STREAM_PRIOR = 5;       // prior draws of ptnn_evidence (counter: k / 4, draw, 0)

// stage c: per distinct vector u, the terms of rows [row0, row0 + nr) added to acc[u] in row order
struct EvidRows {
    const float* fx;            // [nr * O][U] network outputs of the block (predict_forward_kernel layout)
    const float* y;             // target of block row r at y[r * ys]
    int ys, nr, O, U, reg;
    double* acc;                // [U] running sums (zeroed before the first block)
};

__global__ void __launch_bounds__(EVID_THREADS) evid_rows_kernel(const EvidRows a) {
    const int u = blockIdx.x * EVID_THREADS + threadIdx.x;
    if (u >= a.U) return;
    double s = a.acc[u];
    for (int r = 0; r < a.nr; ++r) {
        const double yv = (double)a.y[(size_t)r * a.ys];
        if (a.reg) {
            const double d = yv - (double)a.fx[(size_t)r * a.U + u];
            s += d * d;
        } else {
            s += log((double)a.fx[((size_t)r * a.O + (int)yv) * a.U + u]);      // CLS:209-222: log p_y, as ptnn_elpd
        }
    }
    a.acc[u] = s;
}

// U and b of every distinct vector: classification U = sum log p_y, b = 0; regression U = -(N / 2) log SSE, b = -log SSE
__global__ void __launch_bounds__(EVID_THREADS) evid_finish_kernel(int U, int reg, int N, const double* acc, double* u_out,
                                                                   double* b_out, int* zero_sse) {
    const int u = blockIdx.x * EVID_THREADS + threadIdx.x;
    if (u >= U) return;
    const double s = acc[u];
    if (!reg) { u_out[u] = s; if (b_out) b_out[u] = 0.0; return; }
    if (!(s > 0.0)) atomicAdd(zero_sse, 1);
    const double l = log(s);
    u_out[u] = -0.5 * (double)N * l;
    if (b_out) b_out[u] = -l;
}

// draw j (expanded, chain-major) gets the U of its item's distinct vector; item_of = null: draw j is item j; item_run = null:
// every item is its own entry of u_dist (host U)
__global__ void __launch_bounds__(EVID_THREADS) evid_expand_kernel(long long n_draws, const int* item_of, const int* item_run,
                                                                   const double* u_dist, double* u_draw) {
    const long long j = (long long)blockIdx.x * EVID_THREADS + threadIdx.x;
    if (j >= n_draws) return;
    const long long i = item_of ? item_of[j] : j;
    u_draw[j] = u_dist[item_run ? (long long)item_run[i] : i];
}

// the convergence kernels' host-draw layout [1][n][K] in fp32 for rungs of n draws each (rung k's draws at u_draw + off[k])
__global__ void __launch_bounds__(EVID_THREADS) evid_conv_kernel(int K, int n, const long long* off, const int* rung,
                                                                 const double* u_draw, float* draws) {
    const long long j = (long long)blockIdx.x * EVID_THREADS + threadIdx.x;
    if (j >= (long long)K * n) return;
    const int i = (int)(j / K), q = (int)(j % K);
    draws[j] = (float)u_draw[off[rung[q]] + i];
}

// stage d: one work-group per rung k over its draws u_draw[off[k] .. off[k + 1])
struct EvidRung {
    const double* u_draw;
    const long long* off;       // [K + 1]
    const double* d;            // [K] stone exponents (null: no stones)
    double *mean, *var, *log_stone, *relvar;    // [K] each
};

__global__ void __launch_bounds__(EVID_THREADS) evid_rung_kernel(const EvidRung a) {
    __shared__ double red[EVID_THREADS];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* x = a.u_draw + a.off[k];
    const long long n = a.off[k + 1] - a.off[k];
    double s = 0.0;
    for (long long i = tid; i < n; i += EVID_THREADS) s += x[i];
    const double mean = wg_sum<EVID_THREADS>(red, s) / (double)n;
    double q = 0.0;
    for (long long i = tid; i < n; i += EVID_THREADS) { const double c = x[i] - mean; q += c * c; }
    const double var = wg_sum<EVID_THREADS>(red, q) / (double)(n - 1);
    if (tid == 0) { a.mean[k] = mean; a.var[k] = var; }
    if (!a.d) return;
    const double dk = a.d[k];
    double mx = -INFINITY;
    for (long long i = tid; i < n; i += EVID_THREADS) mx = fmax(mx, dk * x[i]);
    mx = wg_max<EVID_THREADS>(red, mx);
    double e = 0.0;
    for (long long i = tid; i < n; i += EVID_THREADS) e += exp(dk * x[i] - mx);
    const double me = wg_sum<EVID_THREADS>(red, e) / (double)n;
    double ve = 0.0;
    for (long long i = tid; i < n; i += EVID_THREADS) { const double c = exp(dk * x[i] - mx) - me; ve += c * c; }
    ve = wg_sum<EVID_THREADS>(red, ve) / (double)(n - 1);
    if (tid == 0) { a.log_stone[k] = mx + log(me); a.relvar[k] = ve / (me * me); }
}

// the four standard normals of components 4 q .. 4 q + 3 of prior draw `draw`
__device__ __forceinline__ void prior_normals(int q, long long draw, uint32_t slo, uint32_t shi, float (&z)[4]) {
    uint32_t x[4];
    philox4x32_10((uint32_t)q, (uint32_t)draw, 0u, STREAM_PRIOR, slo, shi, x);
    box_muller(x[0], x[1], z[0], z[1]);
    box_muller(x[2], x[3], z[2], z[3]);
}

// stage e: the vectors of prior draws [d0, d0 + nb): w[b][k] = sigma * normals(P, d0 + b, 0, STREAM_PRIOR, seed)[k] (philox.py)
__global__ void __launch_bounds__(EVID_THREADS) evid_prior_kernel(long long d0, int nb, int P, float sigma, uint32_t slo, uint32_t shi,
                                                                  float* w, long long* run_off) {
    const int nq = (P + 3) >> 2;
    const long long j = (long long)blockIdx.x * EVID_THREADS + threadIdx.x;
    if (j >= (long long)nb * nq) return;
    const int b = (int)(j / nq), q = (int)(j % nq);
    float z[4];
    prior_normals(q, d0 + b, slo, shi, z);
    float* dst = w + (size_t)b * P;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (4 * q + c < P) dst[4 * q + c] = sigma * z[c];
    if (q == 0) run_off[b] = (long long)b * P;
}

// stage e: per exponent a_j (one work-group each) over all n prior draws with weights e^{b + a_j U}:
// log mean e^{b + a_j U} (exact max), Kish ESS (sum w)^2 / sum w^2, the weighted mean and variance of U
struct EvidPriorRed {
    const double* u;            // [n]
    const double* b;            // [n]
    long long n;
    const double* a;            // [n_a]
    double *lme, *kish, *umean, *uvar;   // [n_a] each
};

__global__ void __launch_bounds__(EVID_THREADS) evid_prior_reduce_kernel(const EvidPriorRed r) {
    __shared__ double red[EVID_THREADS];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double aj = r.a[j];
    double mx = -INFINITY;
    for (long long i = tid; i < r.n; i += EVID_THREADS) mx = fmax(mx, r.b[i] + aj * r.u[i]);
    mx = wg_max<EVID_THREADS>(red, mx);
    double s0 = 0.0, s1 = 0.0, su = 0.0;
    for (long long i = tid; i < r.n; i += EVID_THREADS) {
        const double w = exp(r.b[i] + aj * r.u[i] - mx);
        s0 += w; s1 += w * w; su += w * r.u[i];
    }
    s0 = wg_sum<EVID_THREADS>(red, s0);
    s1 = wg_sum<EVID_THREADS>(red, s1);
    const double mu = wg_sum<EVID_THREADS>(red, su) / s0;
    double sv = 0.0;
    for (long long i = tid; i < r.n; i += EVID_THREADS) {
        const double w = exp(r.b[i] + aj * r.u[i] - mx), c = r.u[i] - mu;
        sv += w * c * c;
    }
    sv = wg_sum<EVID_THREADS>(red, sv);
    if (tid == 0) {
        r.lme[j] = mx + log(s0 / (double)r.n);
        r.kish[j] = s0 * s0 / s1;
        r.umean[j] = mu;
        r.uvar[j] = sv / s0;
    }
}
