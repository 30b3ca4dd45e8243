// ptnn_dev_lfo.hpp -- part of ptnn_analysis.hip (textually included there after ptnn_dev_elpd.hpp, inside namespace ptnn; not a
// stand-alone header): leave-future-out cross-validation of ordered data rows (ptnn_lfo, include/ptnn.h).
// The samples are conditioned on rows [0, n_fit); an origin i scores rows [i, i + block) from the rows [0, i) by Pareto-smoothed
// importance weights with the log ratio lr = C[i] - C[n_fit], where C[j] = the sum of a sample's pointwise ll over rows < j.
//   a, b. the stages of ptnn_elpd, unchanged (shared selection, elpd_run_eta_kernel, the per-shape predict_forward_kernel).
//   c. lfo_accum_kernel: one lane per distinct sample folds the ll of a row block (elpd_ll, the same function ptnn_elpd reduces)
//      into its running sum, rows ascending, the carry kept across blocks, and keeps C at the columns the origins need.
//   d. lfo_reduce_kernel: one work-group per origin; (lr, t) read from the sums, then psis_reduce of ptnn_dev_elpd.hpp.
// A sum C[j] is one double accumulated in row order per sample, so it does not depend on the row blocks or on which columns are
// kept; psis_reduce depends on the multiset of (lr, t) only.  Hence the invariance of section 13 carries over bitwise: trace,
// host vectors, expanded or (distinct, multiplicity) input, any scratch budget, any split of the origins into launches.

struct LfoAcc {
    ElpdRed a;                  // the block as ptnn_elpd describes it: mode, fx / ll, eta, y, ys, U, O, row0
    int nrows;                  // rows of the block
    const int* slot_of;         // [n_rows + 1] the column of C that keeps the sum over rows < j, or -1
    double* carry;              // [U] the sum over the rows before the block; after it, over the rows through it
    double* C;                  // [n_slots][U]
};

__global__ void __launch_bounds__(ELPD_THREADS) lfo_accum_kernel(const LfoAcc p) {
    const int u = blockIdx.x * ELPD_THREADS + threadIdx.x;
    if (u >= p.a.U) return;
    double c = p.carry[u];
    for (int r = 0; r < p.nrows; ++r) {
        const int n = p.a.row0 + r;
        const double y = p.a.mode == ELPD_HOST ? 0.0 : (double)p.a.y[(size_t)n * p.a.ys];
        c += elpd_ll(p.a, r, u, y);
        const int slot = p.slot_of[n + 1];
        if (slot >= 0) p.C[(size_t)slot * p.a.U + u] = c;
    }
    p.carry[u] = c;
}

struct LfoRed {
    const double* C;            // [n_slots][U]
    const int* cnt;             // [U] multiplicities (0 = absent)
    const int* org_slot;        // [n_origins][2] the columns of C[i] and C[i + block] of the launch's origins
    int fit_slot;               // the column of C[n_fit]
    int U, M;                   // M: tail length bound, <= ELPD_TAIL_CAP
    long long S;                // expanded sample count
    double* elpd_lfo;           // [n_origins] each, at blockIdx.x
    double* khat;
    long long* tail_len;
};

// an origin's entries: lr = C[i] - C[n_fit] (lw = lr - max lr), t = C[i + block] - C[i]; the tail keeps (key(lw), key(t))
struct LfoSrc {
    const double *ci, *cf, *ce;
    const int* cnt;
    double lrmax;
    static constexpr bool PAIR = true;
    static constexpr bool EMIT = false;
    __device__ __forceinline__ int count(int u) const { return cnt[u]; }
    __device__ __forceinline__ double lr(int u) const { return ci[u] - cf[u]; }
    __device__ __forceinline__ void get(int u, double& lw, double& t) const {
        const double c = ci[u];
        lw = (c - cf[u]) - lrmax; t = ce[u] - c;
    }
    __device__ __forceinline__ unsigned long long key(double lw, double) const { return elpd_key(lw); }
    __device__ __forceinline__ unsigned long long second(double t) const { return elpd_key(t); }
    __device__ __forceinline__ void decode(unsigned long long k, unsigned long long v, double& lw, double& t) const {
        lw = elpd_unkey(k); t = elpd_unkey(v);
    }
};

constexpr size_t LFO_TVAL_OFFSET = (sizeof(ElpdShared) + 15) / 16 * 16;
constexpr size_t LFO_LDS_BYTES = LFO_TVAL_OFFSET + sizeof(unsigned long long) * ELPD_TAIL_CAP;   // dynamic: above the static 64 KB

__global__ void __launch_bounds__(ELPD_THREADS) lfo_reduce_kernel(const LfoRed a) {
    extern __shared__ __align__(16) unsigned char lfo_lds[];
    ElpdShared& sh = *reinterpret_cast<ElpdShared*>(lfo_lds);
    unsigned long long* tval = reinterpret_cast<unsigned long long*>(lfo_lds + LFO_TVAL_OFFSET);
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const size_t U = (size_t)a.U;
    LfoSrc src{a.C + (size_t)a.org_slot[2 * k] * U, a.C + (size_t)a.fit_slot * U, a.C + (size_t)a.org_slot[2 * k + 1] * U, a.cnt, 0.0};
    // the largest log ratio (an origin at the fit: every lr is 0, the tail empty, the weights uniform)
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double mn = INF, mx = -INF;
    for (int u = tid; u < a.U; u += ELPD_THREADS) {
        if (a.cnt[u] == 0) continue;
        const double v = src.lr(u);
        mn = fmin(mn, v); mx = fmax(mx, v);
    }
    block_min_max(sh, mn, mx);
    src.lrmax = mx;
    double elpd, khat;
    long long T;
    psis_reduce(sh, tval, src, a.U, a.S, a.M, &elpd, &khat, &T);
    if (tid == 0) {
        a.elpd_lfo[k] = elpd;
        a.khat[k] = khat;
        a.tail_len[k] = T;
    }
}
