// ptnn_dev_select.hpp -- the shape-independent kernels of the posterior predictive (textually included by ptnn_analysis.hip,
// inside namespace ptnn, after ptnn_shapes.hpp; not a stand-alone header): stages a and c of ptnn_dev_predict.hpp --
// sample_runs_kernel + predict_scan_kernel, the sample selection every analysis call shares, and predict_reduce_kernel.  The
// object that includes this file holds them.

// Where trace row `step` of local replica `rep` keeps its vector: the float offset in d_pos_w [Rl][cap][PW] -- its own ring slot,
// or with compact traces the row its TR_SRC names (a rejected step wrote no vector).  *src_out = the step whose row that is; a
// TR_SRC outside [0, step] is counted in *error and the step's own slot used, which keeps the address inside the ring.  Shared by
// sample_runs_kernel and conv_gather_kernel.
__device__ __forceinline__ long long trace_vector_offset(const float* scal, long long rep, int cap, int PW, int step, int compact,
                                                         int* error, int* src_out) {
    const int slot = step % cap;
    if (!compact) { *src_out = step; return (rep * cap + slot) * (long long)PW; }
    int src = __float_as_int(scal[(rep * cap + slot) * TR_COUNT + TR_SRC]);
    if (src < 0 || src > step) { atomicAdd(error, 1); src = step; }   // keeps the address inside the ring
    *src_out = src;
    return (rep * cap + src % cap) * (long long)PW;
}

// stage a, part 1: per selected item, where its vector is, whether it starts a run; with reg also its eta, compared with the
// previous item's and checked for validity.  Shared by every analysis call that reads weight vectors (ptnn_analysis.hip: distinct_samples).
struct SampleSel {
    // trace source (items = n_chains x m selected rows, chain-major)
    const float* pos_w;         // d_pos_w [Rl][cap][PW]
    const float* scal;          // d_scal [Rl][cap][TR_COUNT] (compact traces: TR_SRC; reg: TR_ACC_TR, TR_ACCEPT)
    const int* replicas;        // [n_chains] local replica indices
    const int* st_i;            // d_st_i [Rl][SI_COUNT]: SI_NACC = accepted steps so far (the last row's successor; reg only)
    int cap, PW, step0, thin, m, compact, cur;   // cur: MH steps done = the last trace row
    // host source (items = uploaded vectors [n][P], dense, and with reg their eta [n])
    int host;
    const float* host_eta;
    int reg, P;                 // reg: a sample is (w, eta), a regression's eta = log tau^2
    long long n_items;
    long long* item_off;        // out: float offset of the item's vector
    float* item_eta;            // out: the item's eta (0 without reg), or null: not stored
    int* flag;                  // out: 1 = the item starts a run
    int* error;                 // out: [0] unresolved compact rows (internal error); reg: [1] rows without eta, [2] first such chain
};

__global__ void __launch_bounds__(PRED_THREADS) sample_runs_kernel(const SampleSel s) {
    const long long i = (long long)blockIdx.x * PRED_THREADS + threadIdx.x;
    if (i >= s.n_items) return;
    if (s.host) {
        const float* w = s.pos_w + i * s.P;
        int differs = i == 0;
        for (int k = 0; k < s.P && !differs; ++k) differs = __float_as_uint(w[k]) != __float_as_uint(w[k - s.P]);
        const float eta = s.reg ? s.host_eta[i] : 0.0f;
        if (s.reg && !differs) differs = __float_as_uint(eta) != __float_as_uint(s.host_eta[i - 1]);
        s.item_off[i] = i * s.P;
        if (s.item_eta) s.item_eta[i] = eta;
        s.flag[i] = differs;
        return;
    }
    const int c = (int)(i / s.m), j = (int)(i % s.m);
    const long long rep = s.replicas[c];
    auto eta_of = [&](int src) -> float {
        return s.reg ? s.scal[(rep * s.cap + src % s.cap) * TR_COUNT + TR_ACC_TR] : 0.0f;
    };
    const int step = s.step0 + j * s.thin;
    int src = 0, src_prev = 0;
    const long long off = trace_vector_offset(s.scal, rep, s.cap, s.PW, step, s.compact, s.error, &src);
    const float eta = eta_of(src);
    int differs = j == 0;
    if (!differs) {
        const long long off_prev = trace_vector_offset(s.scal, rep, s.cap, s.PW, step - s.thin, s.compact, s.error, &src_prev);
        if (s.compact) differs = src != src_prev;
        else {
            const float* a = s.pos_w + off;
            const float* b = s.pos_w + off_prev;
            for (int k = 0; k < s.P && !differs; ++k) differs = __float_as_uint(a[k]) != __float_as_uint(b[k]);
        }
        if (s.reg && !differs) differs = __float_as_uint(eta) != __float_as_uint(eta_of(src_prev));
    }
    if (s.reg) {
        // row r (after MH step r - 1) holds a recorded eta once some step <= r - 1 was accepted: the count AFTER step r - 1 is the
        // TR_ACCEPT of row r + 1 (written before step r's decision, REG:380), or the chain's counter when r is the last row
        auto accepted_before = [&](int row) -> int {
            return __float_as_int(s.scal[(rep * s.cap + row % s.cap) * TR_COUNT + TR_ACCEPT]);
        };
        const int after = step < s.cur ? accepted_before(step + 1) : s.st_i[rep * SI_COUNT + SI_NACC];
        if (after < 1) { atomicAdd(&s.error[1], 1); atomicMin(&s.error[2], c); }
    }
    s.item_off[i] = off;
    if (s.item_eta) s.item_eta[i] = eta;
    s.flag[i] = differs;
}

// stage a, part 2 (one work-group): run index of every item, the offset and multiplicity of every run, the number of runs
struct PredictScan {
    long long n_items;
    const int* flag;
    const long long* item_off;
    const int* weight;          // [n_items] multiplicity of the item, or null (1 each)
    int* item_run;              // out: run index of the item
    long long* run_off;         // out: [U] vector offset of the run
    int* run_cnt;               // out: [U] multiplicity (zeroed by the caller)
    int* n_runs;                // out: U
};

__global__ void __launch_bounds__(PRED_SCAN_THREADS) predict_scan_kernel(const PredictScan s) {
    __shared__ long long part[PRED_SCAN_THREADS];
    const int tid = threadIdx.x;
    const long long per = (s.n_items + PRED_SCAN_THREADS - 1) / PRED_SCAN_THREADS;
    const long long lo = min(s.n_items, per * tid), hi = min(s.n_items, lo + per);
    long long c = 0;
    for (long long i = lo; i < hi; ++i) c += s.flag[i];
    part[tid] = c;
    __syncthreads();
    wg_incl_scan<PRED_SCAN_THREADS>(part, tid);            // inclusive scan of the per-thread run starts
    long long r = part[tid] - c - 1;                        // index of the run in progress before this thread's first item
    for (long long i = lo; i < hi; ++i) {
        if (s.flag[i]) { ++r; s.run_off[r] = s.item_off[i]; }
        s.item_run[i] = (int)r;
        atomicAdd(&s.run_cnt[r], s.weight ? s.weight[i] : 1);
    }
    if (tid == PRED_SCAN_THREADS - 1) *s.n_runs = (int)part[tid];
}

// stage c: one work-group per output column of a block
struct PredictRed {
    const float* fx;            // [ncols][U]
    const int* cnt;             // [U]
    int U, O, col0;             // col0: global index of the block's first column
    int ncols_total;            // columns of the whole request (n_rows * O)
    long long M;                // selected rows, repeats included
    int n_ranks;
    const long long* ranks;     // [n_ranks] 0-based ranks in the expanded multiset
    double* mean;               // [ncols_total]
    float* ostat;               // [n_ranks][ncols_total]
    long long* votes;           // [ncols_total] samples whose argmax is this column's class, or null (regression)
};

__device__ __forceinline__ unsigned pred_key(float f) {         // order-preserving uint32 key of an fp32 value
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pred_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(PRED_THREADS) predict_reduce_kernel(const PredictRed r) {
    __shared__ double dsum[PRED_THREADS];
    __shared__ long long vsum[PRED_THREADS];
    __shared__ unsigned hist[PRED_MAX_RANKS][256];
    __shared__ unsigned prefix[PRED_MAX_RANKS];
    __shared__ long long krem[PRED_MAX_RANKS];
    const int tid = threadIdx.x, col = blockIdx.x;
    const float* f = r.fx + (size_t)col * r.U;
    // weighted mean in double, a fixed summation order for a given U
    double s = 0.0;
    long long votes = 0;
    const int o = col % r.O;
    const float* row_base = r.fx + (size_t)(col - o) * r.U;  // column of class 0 of the same row
    for (int u = tid; u < r.U; u += PRED_THREADS) {
        const int c = r.cnt[u];
        s += (double)c * (double)f[u];
        if (r.votes) {
            int best = 0;
            float bv = row_base[u];
            for (int q = 1; q < r.O; ++q) {
                const float v = row_base[(size_t)q * r.U + u];
                if (v > bv) { bv = v; best = q; }                   // first index wins a tie (np.argmax)
            }
            if (best == o) votes += c;
        }
    }
    dsum[tid] = s;
    vsum[tid] = votes;
    if (tid < r.n_ranks) { prefix[tid] = 0u; krem[tid] = r.ranks[tid]; }
    __syncthreads();
    wg_tree<PRED_THREADS>([&](int i, int j) { dsum[i] += dsum[j]; vsum[i] += vsum[j]; });
    if (tid == 0) {
        r.mean[r.col0 + col] = dsum[0] / (double)r.M;
        if (r.votes) r.votes[r.col0 + col] = vsum[0];
    }
    // exact order statistics: 4 passes of 8 bits over the keys, one LDS histogram of multiplicities per target rank
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int k = tid; k < r.n_ranks * 256; k += PRED_THREADS) hist[k >> 8][k & 255] = 0u;
        __syncthreads();
        for (int u = tid; u < r.U; u += PRED_THREADS) {
            const unsigned key = pred_key(f[u]);
            const unsigned c = (unsigned)r.cnt[u];
            for (int t = 0; t < r.n_ranks; ++t)
                if (pass == 0 || (key >> (shift + 8)) == (prefix[t] >> (shift + 8))) atomicAdd(&hist[t][(key >> shift) & 255u], c);
        }
        __syncthreads();
        if (tid < r.n_ranks) {
            long long k = krem[tid], cum = 0;
            for (int b = 0; b < 256; ++b) {
                const long long hcount = hist[tid][b];
                if (k < cum + hcount) { prefix[tid] |= (unsigned)b << shift; krem[tid] = k - cum; break; }
                cum += hcount;
            }
        }
        __syncthreads();
    }
    if (tid < r.n_ranks) r.ostat[(size_t)tid * r.ncols_total + r.col0 + col] = pred_unkey(prefix[tid]);
}
