// ptnn_dev_rank.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn, after ptnn_dev_convergence.hpp
// and ptnn_dev_powerscale.hpp; not a stand-alone header): the front half of the rank-normalised convergence diagnostics
// (ptnn_rank_convergence, include/ptnn.h; Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021).
// A segment is what is ranked together: the L = 2 C h kept draws of a quantity (each chain's first and last h = n / 2 draws), or,
// for the per-chain figures, the 2 h kept draws of one chain of it.  Per block of quantities, the host loop in ptnn_analysis.hip:
//   1. rank_gather_kernel: one work-group per (chain, tile of 64 quantities) reads the chain's rows as conv_gather_kernel does
//      (conv_load: trace rows through trace_vector_offset, or host draws) and writes, through an LDS transpose, the sort word
//      (pred_key(value) << 32 | position in the segment) of every kept draw; -0 is keyed as +0; a non-finite draw flags its quantity.
//   2. the segmented bitonic sort of ptnn_dev_powerscale.hpp orders every segment's words (the padding, ~0, sorts last).
//   3. rank_series_kernel: a thread per sorted position.  Equal keys are equal values, so a run of ties is a run of equal keys:
//      its first and last position are the thread's own where a neighbour differs and a binary search otherwise, and a draw with
//      `less` draws below it and `leq` at or below it has twice the average rank r2 = less + leq + 1 (an integer).  One of
//        RANK_BULK       z = ppnd16((r2 / 2 - 3/8) / (L + 1/4)), and the histogram bin ((r2 - 2) B) / (2 L) of its chain counted
//                        with integer atomics (LDS, then one 64-bit add per non-empty bin);
//        RANK_FOLD       med = (x_(L/2-1) + x_(L/2)) / 2 and f = |x - med| in double; f falls, weakly, over the sorted positions
//                        below L / 2 and rises over the others, so `less` and `leq` of f are four binary searches over the two sides
//                        (the merge of the two sides, without a second sort); ties of f rank equal whichever side they lie on;
//        RANK_INDICATOR  I = [x <= x_(lo)]: the position lies before the end of the run that holds position lo
//      is written, in double, to the draw's own place of the series [position][column].
//   4. conv_gather_kernel<true> and stages 2-4 of ptnn_dev_convergence.hpp take the series as they take draws.
// No floating-point atomics; every result is a function of the words alone.  Nothing here writes chain state, tapes, counters or
// trace rows.

constexpr int RANK_THREADS = 256;          // 4 waves
constexpr int RANK_TILE = 64;              // quantities per work-group of rank_gather_kernel (a lane each)
constexpr int RANK_HIST_LDS = 8192;        // histogram counters a work-group keeps in dynamic LDS (C * B above that: global atomics)
enum { RANK_BULK = 0, RANK_FOLD = 1, RANK_INDICATOR = 2 };

// Wichura's AS241, PPND16: the normal quantile of p in (0, 1), about 1e-16 relative
__device__ double ppnd16(double p) {
    const double q = p - 0.5;
    double r, num, den;
    if (fabs(q) <= 0.425) {
        r = 0.180625 - q * q;
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r
                 + 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r
                 + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r
                 + 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r
                 + 4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r
                 + 1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r
                 + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r
                 + 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r
                 + 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r
                 + 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r
                 + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r
                 + 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r
                 + 5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// 1. the sort words of a block of quantities
struct RankGather {
    ConvGather src;             // the source fields, qcol, nq, C, n, h and error, as conv_gather_kernel reads them
    int per_chain;              // segments: 0 a quantity's 2 C h kept draws, 1 each chain's 2 h
    int npow;                   // words per segment (a power of two; the host has filled the padding)
    unsigned long long* keys;   // [nq][npow], or [nq][C][npow]
    int* bad;                   // [nq] set where a draw of the quantity is not finite
};
__global__ void __launch_bounds__(RANK_THREADS) rank_gather_kernel(const RankGather a) {
    constexpr int NW = RANK_THREADS / WAVE;
    __shared__ float stage[RANK_TILE][RANK_TILE + 1];       // [quantity][draw] of a chunk of 64 draws
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int c = blockIdx.x, k0 = blockIdx.y * RANK_TILE, k = k0 + lane;
    const bool live = k < a.src.nq;
    const int col = a.src.qcol[live ? k : k0];
    const int n = a.src.n, h = a.src.h, C = a.src.C;
    bool nonfinite = false;
    for (int i0 = 0; i0 < n; i0 += RANK_TILE) {
        for (int r = wave; r < RANK_TILE && i0 + r < n; r += NW) {
            const float v = conv_load(a.src, c, i0 + r, col, a.src.error);
            nonfinite |= !isfinite(v);
            stage[lane][r] = v == 0.0f ? 0.0f : v;           // compare by value: -0 is +0
        }
        __syncthreads();
        for (int idx = tid; idx < RANK_TILE * RANK_TILE; idx += RANK_THREADS) {
            const int kk = idx / RANK_TILE, r = idx % RANK_TILE, i = i0 + r;
            if (k0 + kk >= a.src.nq || i >= n || (i >= h && i < n - h)) continue;     // the middle draw of an odd n is dropped
            const int li = i < h ? i : h + i - (n - h);                                // place among the chain's 2 h kept draws
            const unsigned pos = a.per_chain ? (unsigned)li : (unsigned)(c * 2 * h + li);
            const size_t seg = a.per_chain ? (size_t)(k0 + kk) * C + c : (size_t)(k0 + kk);
            a.keys[seg * a.npow + pos] = ((unsigned long long)pred_key(stage[kk][r]) << 32) | pos;
        }
        __syncthreads();
    }
    if (live && nonfinite) atomicOr(&a.bad[k], 1);
}

// 3. one series of every segment of the block, from its sorted words
struct RankSeries {
    const unsigned long long* keys;     // [segments][npow] sorted
    const int* bad;                     // [nq]
    int mode;                           // RANK_BULK, RANK_FOLD, RANK_INDICATOR
    int lo;                             // RANK_INDICATOR: the order statistic floor((L - 1) p)
    int L, npow;                        // draws and words per segment
    int nq, C, per_chain;               // segments: nq, or nq * C
    double* ser;                        // [L][nq], or [L][C][nq]
    unsigned long long* hist;           // RANK_BULK of whole quantities: [C][B][Q] counts, or null
    int B, Q, q0;
};
// the first j in [lo, hi) with pred(j), or hi: pred is false up to some j and true from it on
template <class P> __device__ __forceinline__ int rank_first(int lo, int hi, P pred) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__global__ void __launch_bounds__(RANK_THREADS) rank_series_kernel(const RankSeries a) {
    extern __shared__ int lh[];         // C * B counters where the launch counts in LDS (the host sizes it), else none
    const int tid = threadIdx.x, seg = blockIdx.y, s = blockIdx.x * RANK_THREADS + tid;
    const int k = a.per_chain ? seg / a.C : seg, L = a.L;
    const int ncol = a.per_chain ? a.nq * a.C : a.nq, col = a.per_chain ? (seg % a.C) * a.nq + k : k;
    const unsigned long long* w = a.keys + (size_t)seg * a.npow;
    const bool bad = a.bad[k] != 0;
    const int CB = a.C * a.B;
    const bool count = a.mode == RANK_BULK && a.hist && !bad, in_lds = CB <= RANK_HIST_LDS;      // uniform over the work-group
    if (count && in_lds) {
        for (int i = tid; i < CB; i += RANK_THREADS) lh[i] = 0;
        __syncthreads();
    }
    if (s < L) {
        const unsigned long long word = w[s];
        const unsigned pos = (unsigned)word, key = (unsigned)(word >> 32);
        auto hi = [&](int j) { return (unsigned)(w[j] >> 32); };
        double out;
        if (a.mode == RANK_INDICATOR) {
            const unsigned kl = hi(a.lo);
            const int cut = rank_first(a.lo + 1, L, [&](int j) { return hi(j) > kl; });         // the end of x_(lo)'s run of ties
            out = s < cut ? 1.0 : 0.0;
        } else {
            int less, leq;
            if (a.mode == RANK_BULK) {
                less = (s == 0 || hi(s - 1) != key) ? s : rank_first(0, s, [&](int j) { return hi(j) >= key; });
                leq = (s == L - 1 || hi(s + 1) != key) ? s + 1 : rank_first(s + 1, L, [&](int j) { return hi(j) > key; });
            } else {
                const int half = L / 2;
                const double med = ((double)pred_unkey(hi(half - 1)) + (double)pred_unkey(hi(half))) / 2.0;
                auto f = [&](int j) { return fabs((double)pred_unkey(hi(j)) - med); };
                const double fs = fabs((double)pred_unkey(key) - med);
                // below the median f falls with the position, above it f rises: counts of f_j < fs and f_j <= fs on either side
                const int l_less = half - rank_first(0, half, [&](int j) { return f(j) < fs; });
                const int l_leq = half - rank_first(0, half, [&](int j) { return f(j) <= fs; });
                const int r_less = rank_first(half, L, [&](int j) { return f(j) >= fs; }) - half;
                const int r_leq = rank_first(half, L, [&](int j) { return f(j) > fs; }) - half;
                less = l_less + r_less;
                leq = l_leq + r_leq;
            }
            const long long r2 = (long long)less + leq + 1;                                      // twice the average rank
            out = bad ? __builtin_nan("") : ppnd16((0.5 * (double)r2 - 0.375) / ((double)L + 0.25));
            if (count) {
                const int bin = (int)(((r2 - 2) * a.B) / (2LL * L));
                const int cb = (int)(pos / (unsigned)(L / a.C)) * a.B + bin;                     // the chain's 2 h kept draws are consecutive positions
                if (in_lds) atomicAdd(&lh[cb], 1);
                else atomicAdd(&a.hist[(size_t)cb * a.Q + a.q0 + k], 1ull);
            }
        }
        a.ser[(size_t)pos * ncol + col] = out;
    }
    if (count && in_lds) {
        __syncthreads();
        for (int i = tid; i < CB; i += RANK_THREADS)
            if (lh[i]) atomicAdd(&a.hist[(size_t)i * a.Q + a.q0 + k], (unsigned long long)lh[i]);
    }
}
