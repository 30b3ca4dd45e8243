// ptnn_dev_elpd.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// predictive accuracy of the sampled chains (ptnn_elpd, include/ptnn.h): per data row
// the log pointwise predictive density, the WAIC penalty and the PSIS-LOO estimate with its Pareto shape k-hat.
//   a. sample_runs_kernel (ptnn_dev_select.hpp, with reg) + predict_scan_kernel + elpd_run_eta_kernel: the selected rows
//      collapse into distinct (w, eta) samples with multiplicities; a regression's eta comes from the TR_ACC_TR slot of the row
//      that holds the vector, and rows before their chain's first accepted step (no eta recorded yet) are counted so that the
//      host can refuse them.
//   b. the per-shape predict_forward_kernel of ptnn_dev_predict.hpp, unchanged (all n_out columns of a row are computed).
//   c. elpd_reduce_kernel: one work-group per data row; ll is formed on the fly from the fp32 outputs, everything after is double.
//      Its Pareto smoothing is psis_reduce, which lfo_reduce_kernel (ptnn_dev_lfo.hpp) shares.
// Every sum over samples is a 128-bit fixed-point sum of terms scaled by the row's exact maximum (integer addition: the result
// depends on the multiset of samples only, not on their order or on how repeats are grouped), and the tail is sorted by its ll
// key and merged before the Pareto fit.  So the trace, host vectors, expanded or (distinct, multiplicity) input and any block
// size give bitwise-identical results.  Nothing here writes chain state, tapes, counters or trace rows.

constexpr int ELPD_THREADS = 256;         // 4 waves
constexpr int ELPD_TAIL_CAP = 4096;       // distinct tail entries in LDS (include/ptnn.h: PTNN_ELPD_TAIL_CAP)
constexpr int ELPD_MAX_GRID = 30 + 64;    // m = 30 + floor(sqrt(T)), T <= ELPD_TAIL_CAP
constexpr int ELPD_PER_THREAD = ELPD_TAIL_CAP / ELPD_THREADS;
enum { ELPD_REG = 0, ELPD_CLS = 1, ELPD_HOST = 2 };

// stage a, part 3: the eta of every run (after predict_scan_kernel)
__global__ void __launch_bounds__(ELPD_THREADS) elpd_run_eta_kernel(long long n_items, const int* flag, const int* item_run,
                                                                    const float* item_eta, float* run_eta) {
    const long long i = (long long)blockIdx.x * ELPD_THREADS + threadIdx.x;
    if (i < n_items && flag[i]) run_eta[item_run[i]] = item_eta[i];
}

// stage c: one work-group per data row of a block
struct ElpdRed {
    int mode;                   // ELPD_REG / ELPD_CLS: ll from fx; ELPD_HOST: ll given
    const float* fx;            // [nrows * O][U] network outputs of the block (predict_forward_kernel layout)
    const float* eta;           // [U] eta of distinct sample u (regression)
    const float* y;             // target of global row n at y[n * ys]
    int ys;
    const double* ll;           // host: ll of sample u on global row n at ll[u * ll_stride + n]
    long long ll_stride;
    const int* cnt;             // [U] multiplicities (0 = absent)
    int U, O, row0;             // row0: global index of the block's first row
    long long S;                // expanded sample count (>= 2)
    int M;                      // tail length bound, <= ELPD_TAIL_CAP
    double* lppd;               // [n_rows] each, at row0 + blockIdx.x
    double* p_waic;
    double* elpd_loo;
    double* khat;
    long long* tail_len;
    double* ll_out;             // [nrows][U] or null: elpd_loglik_kernel only
};

constexpr double ELPD_LOG_2PI = 1.8378770664093454836;

__device__ __forceinline__ double elpd_ll(const ElpdRed& a, int r, int u, double y) {
    if (a.mode == ELPD_HOST) return a.ll[(size_t)u * a.ll_stride + a.row0 + r];
    if (a.mode == ELPD_REG) {                                  // REG:200-204, untempered, tau^2 = exp(eta)
        const double f = (double)a.fx[(size_t)r * a.U + u];
        const double eta = (double)a.eta[u];
        const double d = y - f;
        return -0.5 * (ELPD_LOG_2PI + eta) - 0.5 * (d * d) * exp(-eta);
    }
    return log((double)a.fx[((size_t)r * a.O + (int)y) * a.U + u]);   // CLS:209-222: log p_y
}

__device__ __forceinline__ unsigned long long elpd_key(double v) {      // order-preserving uint64 key of a double
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double elpd_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
}

// 128-bit fixed-point accumulator (Fix128, ptnn_dev_wg.hpp): a term t in [0, 1] counts floor(t * 2^62) units, c times -- exact integer sums
__device__ __forceinline__ void fix_add(Fix128& a, double t, unsigned c) {
    t = t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0;
    const unsigned long long v = (unsigned long long)(t * 0x1p62);
    const unsigned long long plo = v * (unsigned long long)c, phi = __umul64hi(v, (unsigned long long)c);
    a.lo += plo;
    a.hi += phi + (a.lo < plo ? 1ull : 0ull);
}

__device__ __forceinline__ double gpinv(double p, double k, double sigma) {
    if (!(sigma > 0.0)) return __longlong_as_double(0x7ff8000000000000ll);
    if (fabs(k) < 2.220446049250313e-16) return -sigma * log1p(-p);
    return sigma * expm1(-k * log1p(-p)) / k;
}

struct ElpdShared {
    unsigned long long tkey[ELPD_TAIL_CAP];    // tail: ~key(ll) (ascending = lw ascending), merged in place into distinct keys
    int tpos[ELPD_TAIL_CAP + 1];               // tail: counts, then each distinct key's first expanded position (tpos[G] = T)
    unsigned long long r0[ELPD_THREADS], r1[ELPD_THREADS];   // block reductions (two 64-bit words per thread)
    unsigned hist[256];
    int scan0[ELPD_THREADS], scan1[ELPD_THREADS];
    double gb[ELPD_MAX_GRID], gk[ELPD_MAX_GRID], gw[ELPD_MAX_GRID];
    double bc[8];                              // broadcast values
    long long bl[4];
    int n_ent, n_grp;
};

// the extremes over the work-group through r0, r1 (every thread gets them; a barrier before and after)
__device__ void block_min_max(ElpdShared& sh, double& mn, double& mx) {
    wg_min_max<ELPD_THREADS>(reinterpret_cast<double*>(sh.r0), reinterpret_cast<double*>(sh.r1), mn, mx);
}
// exclusive scan of one int per thread in thread order; *total = the sum
__device__ int block_excl_scan(int* buf, int v, int* total) {
    const int tid = threadIdx.x;
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
    wg_incl_scan<ELPD_THREADS>(buf, tid);
    const int incl = buf[tid];
    *total = buf[ELPD_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// The Pareto smoothing of stage c over U entries with multiplicities, shared by elpd_reduce_kernel and lfo_reduce_kernel
// (ptnn_dev_lfo.hpp): the cut by radix select, the tail compacted into LDS, sorted and merged, gpdfit, and the two sums
// *elpd = logsumexp(lw + t) - logsumexp(lw) over body samples and smoothed tail positions.  `Src` gives every entry:
//   int count(u)                      multiplicity (0 = absent)
//   void get(u, lw, t)                lw = lr - max(lr) <= 0 and the target t
//   PAIR                              false: one stored word gives both (ptnn_elpd: lw = min(ll) - ll, t = ll); true: (lw, t)
//                                     pairs, t kept in tval [ELPD_TAIL_CAP], entries ordered by lw, then t
//   key(lw, t), second(t)             the stored words, ascending key = ascending lw
//   decode(key, second, lw, t)        their values back
//   EMIT                              true (ptnn_powerscale): emit_body(u, lw) for every body entry and emit_tail(j, t, lw) for
//                                     every smoothed tail position j receive the final log weights; false: nothing is compiled in
// Every thread of the work-group calls it and gets the three results.
template <class Src>
__device__ void psis_reduce(ElpdShared& sh, unsigned long long* tval, const Src& src, int U, long long S_, int M, double* elpd,
                            double* khat_out, long long* tail_out) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    // the cutoff: the value of lw at ascending expanded rank S - M - 1, by 8 passes of 8 bits
    const long long rank = S_ - M - 1;
    const double LOG_DBL_MIN = -708.39641853226408;             // log(DBL_MIN)
    double cut = LOG_DBL_MIN;
    if (rank >= 0) {
        unsigned long long prefix = 0;
        long long krem = rank;
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            for (int k = tid; k < 256; k += ELPD_THREADS) sh.hist[k] = 0u;
            __syncthreads();
            for (int u = tid; u < U; u += ELPD_THREADS) {
                const unsigned c = (unsigned)src.count(u);
                if (c == 0) continue;
                double lw, t;
                src.get(u, lw, t);
                const unsigned long long key = elpd_key(lw);
                if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(key >> shift) & 255u], c);
            }
            __syncthreads();
            if (tid == 0) {
                long long cum = 0;
                for (int b = 0; b < 256; ++b) {
                    const long long hc = sh.hist[b];
                    if (krem < cum + hc) { prefix |= (unsigned long long)b << shift; krem -= cum; break; }
                    cum += hc;
                }
                sh.bl[0] = (long long)prefix; sh.bl[1] = krem;
            }
            __syncthreads();
            prefix = (unsigned long long)sh.bl[0]; krem = sh.bl[1];
            __syncthreads();
        }
        cut = fmax(elpd_unkey(prefix), LOG_DBL_MIN);
    }
    // the tail: samples with lw > cut, compacted as (stored words, count) into LDS; T = their expanded count
    if (tid == 0) sh.n_ent = 0;
    __syncthreads();
    long long t_part = 0;
    for (int u = tid; u < U; u += ELPD_THREADS) {
        const int c = src.count(u);
        if (c == 0) continue;
        double lw, t;
        src.get(u, lw, t);
        if (lw > cut) {
            t_part += c;
            const int slot = atomicAdd(&sh.n_ent, 1);
            if (slot < ELPD_TAIL_CAP) {
                sh.tkey[slot] = src.key(lw, t); sh.tpos[slot] = c;
                if constexpr (Src::PAIR) tval[slot] = src.second(t);
            }
        }
    }
    const long long T = wg_sum<ELPD_THREADS>(reinterpret_cast<long long*>(sh.r0), t_part);   // (barriers inside: n_ent is final)
    const int n_ent = min(sh.n_ent, ELPD_TAIL_CAP);              // the host keeps T <= M <= ELPD_TAIL_CAP
    double khat = INF, sigma = 0.0;
    bool smooth = false;
    const double ecut = exp(cut);
    if (T > 4) {
        // bitonic sort of the entries (padded to a power of two with the largest words), ascending = ascending lw
        int npow = 1;
        while (npow < n_ent) npow <<= 1;
        for (int k = n_ent + tid; k < npow; k += ELPD_THREADS) {
            sh.tkey[k] = ~0ull; sh.tpos[k] = 0;
            if constexpr (Src::PAIR) tval[k] = ~0ull;
        }
        __syncthreads();
        for (int size = 2; size <= npow; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < npow / 2; t += ELPD_THREADS) {
                    const int i = 2 * t - (t & (stride - 1));
                    const int j = i + stride;
                    const bool up = (i & size) == 0;
                    const unsigned long long ki = sh.tkey[i], kj = sh.tkey[j];
                    bool above = ki > kj;
                    if constexpr (Src::PAIR) above = above || (ki == kj && tval[i] > tval[j]);
                    if (above == up) {
                        sh.tkey[i] = kj; sh.tkey[j] = ki;
                        const int ci = sh.tpos[i]; sh.tpos[i] = sh.tpos[j]; sh.tpos[j] = ci;
                        if constexpr (Src::PAIR) { const unsigned long long vi = tval[i]; tval[i] = tval[j]; tval[j] = vi; }
                    }
                }
                __syncthreads();
            }
        }
        // merge equal entries: thread tid owns entries [tid * per, (tid + 1) * per) of the sorted list
        const int per = (npow + ELPD_THREADS - 1) / ELPD_THREADS;
        unsigned long long kk[ELPD_PER_THREAD], vv[Src::PAIR ? ELPD_PER_THREAD : 1];
        int cc[ELPD_PER_THREAD], hh[ELPD_PER_THREAD];
        int csum = 0, hsum = 0;
#pragma unroll
        for (int q = 0; q < ELPD_PER_THREAD; ++q) {
            const int i = tid * per + q;
            const bool live = q < per && i < n_ent;
            kk[q] = live ? sh.tkey[i] : 0ull;
            cc[q] = live ? sh.tpos[i] : 0;
            bool head = live && (i == 0 || sh.tkey[i - 1] != kk[q]);
            if constexpr (Src::PAIR) {
                vv[q] = live ? tval[i] : 0ull;
                head = head || (live && tval[i - 1] != vv[q]);     // (i > 0 here: i == 0 is a head already)
            }
            hh[q] = head ? 1 : 0;
            csum += cc[q]; hsum += hh[q];
        }
        int tot_c = 0, tot_h = 0;
        int pos = block_excl_scan(sh.scan0, csum, &tot_c);
        int grp = block_excl_scan(sh.scan1, hsum, &tot_h);      // (barriers inside: every entry has been read)
#pragma unroll
        for (int q = 0; q < ELPD_PER_THREAD; ++q) {
            if (hh[q]) {
                sh.tkey[grp] = kk[q]; sh.tpos[grp] = pos;
                if constexpr (Src::PAIR) tval[grp] = vv[q];
                ++grp;
            }
            pos += cc[q];
        }
        if (tid == 0) { sh.tpos[tot_h] = tot_c; sh.n_grp = tot_h; }
        __syncthreads();
        const int G = sh.n_grp;
        const double n = (double)T;
        auto x_of = [&](int g) -> double {
            double lw, t;
            src.decode(sh.tkey[g], Src::PAIR ? tval[g] : 0ull, lw, t);
            return exp(lw) - ecut;
        };
        auto group_at = [&](long long p) -> int {                    // the distinct entry holding expanded position p
            int lo = 0, hi = G - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (sh.tpos[mid] <= p) lo = mid; else hi = mid - 1; }
            return lo;
        };
        // gpdfit (Zhang & Stephens 2009, with the weakly informative prior of Vehtari et al.)
        const int m = 30 + (int)floor(sqrt(n));
        const double q1 = x_of(group_at((long long)floor(n / 4.0 + 0.5) - 1));
        const double xmax = x_of(G - 1);
        for (int i = tid; i < m; i += ELPD_THREADS)
            sh.gb[i] = (1.0 - sqrt((double)m / ((double)i + 0.5))) / (3.0 * q1) + 1.0 / xmax;
        __syncthreads();
        for (int i = wave; i < m; i += ELPD_THREADS / WAVE) {          // one wave per grid point, lanes over the distinct entries
            const double b = sh.gb[i];
            double s = 0.0;
            for (int g = lane; g < G; g += WAVE) s += (double)(sh.tpos[g + 1] - sh.tpos[g]) * log1p(-b * x_of(g));
            s = wave_sum(s);
            if (lane == 0) {
                const double k = s / n;
                sh.gk[i] = n * (log(-b / k) - k - 1.0);               // the profile log-likelihood L[i]
            }
        }
        __syncthreads();
        if (wave == 0) {
            for (int i = lane; i < m; i += WAVE) {
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += exp(sh.gk[j] - sh.gk[i]);
                sh.gw[i] = 1.0 / s;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double wsum = 0.0;
            for (int i = 0; i < m; ++i) if (!(sh.gw[i] < 10.0 * 2.220446049250313e-16)) wsum += sh.gw[i];
            double bpost = 0.0;
            for (int i = 0; i < m; ++i) if (!(sh.gw[i] < 10.0 * 2.220446049250313e-16)) bpost += sh.gb[i] * (sh.gw[i] / wsum);
            sh.bc[0] = bpost;
        }
        __syncthreads();
        const double bpost = sh.bc[0];
        double s = 0.0;
        for (int g = tid; g < G; g += ELPD_THREADS) s += (double)(sh.tpos[g + 1] - sh.tpos[g]) * log1p(-bpost * x_of(g));
        s = wave_sum(s);
        __syncthreads();
        if (lane == 0) reinterpret_cast<double*>(sh.r0)[wave] = s;
        __syncthreads();
        const double* ws = reinterpret_cast<double*>(sh.r0);
        const double kpost = (((ws[0] + ws[1]) + ws[2]) + ws[3]) / n;
        sigma = -kpost / bpost;
        khat = (n * kpost + 10.0 * 0.5) / (n + 10.0);
        smooth = isfinite(khat);
        __syncthreads();
    }
    // the smoothed log weight of tail position j (of the distinct entry g)
    const double Tn = (double)T;
    auto lw_smooth = [&](long long j) -> double {
        double v = log(gpinv(((double)j + 0.5) / Tn, khat, sigma) + ecut);
        return v > 0.0 ? 0.0 : v;
    };
    const int G = smooth ? sh.n_grp : 0;
    auto t_at = [&](long long j) -> double {                        // the target of tail position j
        int lo = 0, hi = G - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (sh.tpos[mid] <= j) lo = mid; else hi = mid - 1; }
        double lw, t;
        src.decode(sh.tkey[lo], Src::PAIR ? tval[lo] : 0ull, lw, t);
        return t;
    };
    // the largest lw and lw + t, body samples and smoothed tail positions
    double a1 = -INF, a2 = -INF;
    for (int u = tid; u < U; u += ELPD_THREADS) {
        if (src.count(u) == 0) continue;
        double lw, l;
        src.get(u, lw, l);
        if (smooth && lw > cut) continue;
        a1 = fmax(a1, lw); a2 = fmax(a2, lw + l);
    }
    for (long long j = tid; j < (smooth ? T : 0); j += ELPD_THREADS) {
        const double l = t_at(j), lw = lw_smooth(j);
        a1 = fmax(a1, lw); a2 = fmax(a2, lw + l);
    }
    double na1 = -a1;
    block_min_max(sh, na1, a2);                                  // min of -a1 = -max of a1; max of a2
    a1 = -na1;
    const double b2 = a2;
    // sum c exp(lw - a1) and sum c exp(lw + t - b2)
    Fix128 fz{0, 0}, fl{0, 0};
    for (int u = tid; u < U; u += ELPD_THREADS) {
        const unsigned c = (unsigned)src.count(u);
        if (c == 0) continue;
        double lw, l;
        src.get(u, lw, l);
        if (smooth && lw > cut) continue;
        if constexpr (Src::EMIT) src.emit_body(u, lw);
        fix_add(fz, exp(lw - a1), c);
        fix_add(fl, exp(lw + l - b2), c);
    }
    for (long long j = tid; j < (smooth ? T : 0); j += ELPD_THREADS) {
        const double l = t_at(j), lw = lw_smooth(j);
        if constexpr (Src::EMIT) src.emit_tail(j, l, lw);
        fix_add(fz, exp(lw - a1), 1u);
        fix_add(fl, exp(lw + l - b2), 1u);
    }
    const double z = wg_fix_sum<ELPD_THREADS>(sh.r0, sh.r1, fz);
    const double e = wg_fix_sum<ELPD_THREADS>(sh.r0, sh.r1, fl);
    *elpd = (b2 + log(e)) - (a1 + log(z));
    *khat_out = khat;
    *tail_out = T;
}

// ptnn_elpd's entries: the samples of one data row, lr = -ll and the target ll; the tail keeps ~key(ll)
struct ElpdLooSrc {
    const ElpdRed& a;
    int r;
    double y, mn;               // mn = min(ll) = -max(lr)
    static constexpr bool PAIR = false;
    static constexpr bool EMIT = false;
    __device__ __forceinline__ int count(int u) const { return a.cnt[u]; }
    __device__ __forceinline__ void get(int u, double& lw, double& t) const { t = elpd_ll(a, r, u, y); lw = mn - t; }
    __device__ __forceinline__ unsigned long long key(double, double t) const { return ~elpd_key(t); }
    __device__ __forceinline__ unsigned long long second(double) const { return 0ull; }
    __device__ __forceinline__ void decode(unsigned long long k, unsigned long long, double& lw, double& t) const {
        t = elpd_unkey(~k); lw = mn - t;
    }
};

__global__ void __launch_bounds__(ELPD_THREADS) elpd_reduce_kernel(const ElpdRed a) {
    __shared__ ElpdShared sh;
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const double y = a.mode == ELPD_HOST ? 0.0 : (double)a.y[(size_t)(a.row0 + r) * a.ys];
    const double S = (double)a.S;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);

    // pass 1: the extremes of ll
    double mn = INF, mx = -INF;
    for (int u = tid; u < a.U; u += ELPD_THREADS) {
        if (a.cnt[u] == 0) continue;
        const double l = elpd_ll(a, r, u, y);
        mn = fmin(mn, l); mx = fmax(mx, l);
    }
    block_min_max(sh, mn, mx);
    const double R = mx - mn;
    // pass 2: sum c exp(ll - max) and sum c (ll - min) / R
    Fix128 fe{0, 0}, fm{0, 0};
    for (int u = tid; u < a.U; u += ELPD_THREADS) {
        const unsigned c = (unsigned)a.cnt[u];
        if (c == 0) continue;
        const double l = elpd_ll(a, r, u, y);
        fix_add(fe, exp(l - mx), c);
        if (R > 0.0) fix_add(fm, (l - mn) / R, c);
    }
    const double se = wg_fix_sum<ELPD_THREADS>(sh.r0, sh.r1, fe);
    const double sm = wg_fix_sum<ELPD_THREADS>(sh.r0, sh.r1, fm);
    const double lppd = mx + log(se / S);
    double mean = R > 0.0 ? mn + R * (sm / S) : mn;
    mean = fmin(fmax(mean, mn), mx);
    // pass 3: sum c (ll - mean)^2, each term scaled by the largest one
    const double D = fmax((mx - mean) * (mx - mean), (mean - mn) * (mean - mn));
    Fix128 fv{0, 0};
    if (D > 0.0) {
        for (int u = tid; u < a.U; u += ELPD_THREADS) {
            const unsigned c = (unsigned)a.cnt[u];
            if (c == 0) continue;
            const double d = elpd_ll(a, r, u, y) - mean;
            fix_add(fv, (d * d) / D, c);
        }
    }
    const double p_waic = D > 0.0 ? D * wg_fix_sum<ELPD_THREADS>(sh.r0, sh.r1, fv) / (S - 1.0) : 0.0;

    // the Pareto smoothing of lr = -ll (lw = lr - max(lr) = min(ll) - ll) with the target ll
    const ElpdLooSrc src{a, r, y, mn};
    double elpd_loo, khat;
    long long T;
    psis_reduce(sh, nullptr, src, a.U, a.S, a.M, &elpd_loo, &khat, &T);
    if (tid == 0) {
        const int n = a.row0 + r;
        if (a.lppd) a.lppd[n] = lppd;
        if (a.p_waic) a.p_waic[n] = p_waic;
        if (a.elpd_loo) a.elpd_loo[n] = elpd_loo;
        if (a.khat) a.khat[n] = khat;
        if (a.tail_len) a.tail_len[n] = T;
    }
}

// the pointwise log-likelihood of a block as the reduction forms it: ll_out[r][u] (for ptnn_elpd_spec.loglik_out)
__global__ void __launch_bounds__(ELPD_THREADS) elpd_loglik_kernel(const ElpdRed a, int nrows) {
    const long long i = (long long)blockIdx.x * ELPD_THREADS + threadIdx.x;
    if (i >= (long long)nrows * a.U) return;
    const int r = (int)(i / a.U), u = (int)(i % a.U);
    const double y = a.mode == ELPD_HOST ? 0.0 : (double)a.y[(size_t)(a.row0 + r) * a.ys];
    a.ll_out[i] = elpd_ll(a, r, u, y);
}
