// ptnn_dev_compress.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// posterior compression, kernel herding with the energy-distance kernel ("support points") on the all-pairs function-space distance
// that ptnn_dev_modes.hpp forms (ptnn_compress, include/ptnn.h).  Shape-independent kernels only: no per-shape
// code object includes this file.
//   a. compress_mean_kernel: one work-group per row u: mu_u = (sum_v c_v sqrt(sq[u, v])) / M, thread t adding v = t, t + 256, ... in
//      ascending order, the 256 partials down wg_sum<256>; the row's count of non-finite elements; the work-group that finishes last
//      adds c_u mu_u in row order and divides by M: D0.
//   b. compress_herd_kernel: ONE work-group of 1024 threads walks the m picks.  Thread t owns the candidates c = t + 1024 k, k < 12
//      (U <= 11585 < 12 x 1024) and keeps their r_c, mu_c and a live bit (present, not yet chosen) in registers.  Per pick: the
//      thread's smallest (order-preserving bits of score_c, c), wg_min_pair<1024>, the owner of the winner x publishes r_x and mu_x
//      through LDS, thread 0 carries musum and pair and writes picks, energy and pick_score, and every thread adds sqrt(sq[x, c]) to
//      its live r_c: the matrix is symmetric bit for bit, so column x is the contiguous row x.  No grid barrier, no relaunch.
//   c. compress_subset_kernel: one work-group per subset: strided partials of sum_k mu and of sum over the m_b^2 ordered pairs
//      p -> (p / m_b, p % m_b) of d, ascending p, down wg_sum<256>.
// Rounding: every double operation here is rounded once and none is contracted with its neighbour: each kernel body opens with
// `#pragma clang fp contract(off)` (this compiler's __dmul_rn / __dadd_rn are plain operators, which the default contraction would
// still fuse, so the pragma is what holds), the square root is __dsqrt_rn and `/` is the correctly rounded division (the library is
// built without fast-math).  A numpy float64 replay in the same order reproduces every bit (tests/compress_ref.py).
// Registers of b (gfx950, from the compiler's resource-usage remark): the 12-candidate layout holds 24 doubles of state per thread;
// the kernel takes 108 VGPRs, 0 AGPRs and no scratch (0 spilled) -- under the 128 that 16 waves per work-group leave a thread -- and
// 16 KiB + 16 B of LDS.
// No value passes through an atomic: the one atomic is the ticket that elects the finishing work-group of a.  Nothing here writes
// chain state, tapes, counters or trace rows.

constexpr int COMPRESS_THREADS = 256;
constexpr int COMPRESS_HERD_THREADS = 1024;
constexpr int COMPRESS_HERD_OWN = 12;       // candidates per thread: 12 x 1024 > 11585 = the largest U under PTNN_MODES_MAX_ELEMENTS
static_assert((long long)COMPRESS_HERD_OWN * COMPRESS_HERD_THREADS * COMPRESS_HERD_OWN * COMPRESS_HERD_THREADS > (1ll << 27), "herd layout covers the cap");

// signed double -> unsigned word of the same order (scores can be negative), and back
__device__ __forceinline__ unsigned long long compress_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double compress_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}
// 2 a / n - b / n^2 - d0, each operation rounded once (n^2 is exact: n < 2^26)
__device__ __forceinline__ double compress_energy(double musum, double pair, double n, double d0) {
#pragma clang fp contract(off)
    const double t1 = (2.0 * musum) / n;
    const double t2 = pair / (n * n);
    const double t3 = t1 - t2;
    return t3 - d0;
}

struct CompressMean {
    const double* sq;           // [U][U]
    const int* cnt;             // [U] multiplicities (0 = absent)
    int U;
    double m;                   // M as a double
    double* mu;                 // [U] (absent: 0)
    double* row_part;           // [U] c_u mu_u
    long long* row_bad;         // [U] non-finite elements among the present v; + 2^40 when sq[u, u] is one of them
    unsigned int* ticket;       // 0 before the launch
    double* d0;                 // [1]
    long long* bad;             // [2] as ModesDensity::bad
};

__global__ void __launch_bounds__(COMPRESS_THREADS) compress_mean_kernel(const CompressMean a) {
#pragma clang fp contract(off)
    __shared__ double rd[COMPRESS_THREADS];
    __shared__ long long rl[COMPRESS_THREADS];
    __shared__ unsigned int last;
    const int tid = threadIdx.x, u = (int)blockIdx.x;
    const double* row = a.sq + (size_t)u * a.U;
    const int cu = a.cnt[u];
    long long nbad = 0;
    double part = 0.0;
    if (cu != 0)
        for (int v = tid; v < a.U; v += COMPRESS_THREADS) {
            const int c = a.cnt[v];
            if (c == 0) continue;
            const double s = row[v];
            if (!(fabs(s) <= 1.7976931348623157e308)) { ++nbad; continue; }
            const double term = (double)c * __dsqrt_rn(s);
            part = part + term;
        }
    nbad = wg_sum<COMPRESS_THREADS>(rl, nbad);
    part = wg_sum<COMPRESS_THREADS>(rd, part);
    if (tid == 0) {
        const bool diag = cu != 0 && !(fabs(row[u]) <= 1.7976931348623157e308);
        const double mu = part / a.m;
        a.mu[u] = mu;
        a.row_part[u] = (double)cu * mu;
        a.row_bad[u] = nbad + (diag ? (1ll << 40) : 0);
        __threadfence();
        last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;                          // `last` is shared: the whole work-group leaves or stays
    __threadfence();
    // the finishing work-group, as modes_density_kernel's: 256 rows at a time into LDS, added by one thread in row order
    const volatile double* part_v = a.row_part;
    const volatile long long* bad_v = a.row_bad;
    double s = 0.0;
    long long bad = 0, first_diag = -1, first_row = -1;
    for (int r0 = 0; r0 < a.U; r0 += COMPRESS_THREADS) {
        const int r = r0 + tid, nr = min(COMPRESS_THREADS, a.U - r0);
        if (tid < nr) { rd[tid] = part_v[r]; rl[tid] = bad_v[r]; }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < nr; ++k) {
                s = s + rd[k];
                const long long b = rl[k];
                if (b != 0 && first_row < 0) first_row = r0 + k;
                if (b >= (1ll << 40) && first_diag < 0) first_diag = r0 + k;
                bad += b & ((1ll << 40) - 1);
            }
        __syncthreads();
    }
    if (tid != 0) return;
    a.d0[0] = s / a.m;
    a.bad[0] = bad;
    a.bad[1] = first_diag >= 0 ? first_diag : first_row;
}

struct CompressHerd {
    const double* sq;           // [U][U]
    const int* cnt;             // [U]
    const double* mu;           // [U]
    const double* d0;           // [1]
    int U, m;                   // m <= the present samples
    int* picks;                 // [m]
    double* energy;             // [m]
    double* score;              // [m] the winning score of every pick
};

__global__ void __launch_bounds__(COMPRESS_HERD_THREADS) compress_herd_kernel(const CompressHerd a) {
#pragma clang fp contract(off)
    __shared__ unsigned long long ka[COMPRESS_HERD_THREADS], kb[COMPRESS_HERD_THREADS];
    __shared__ double pub[2];
    const int tid = threadIdx.x;
    double r[COMPRESS_HERD_OWN], mu[COMPRESS_HERD_OWN];
    unsigned int live = 0;
#pragma unroll
    for (int k = 0; k < COMPRESS_HERD_OWN; ++k) {
        const int c = tid + COMPRESS_HERD_THREADS * k;
        r[k] = 0.0;
        mu[k] = c < a.U ? a.mu[c] : 0.0;
        if (c < a.U && a.cnt[c] != 0) live |= 1u << k;
    }
    const double d0 = a.d0[0];
    double musum = 0.0, pair = 0.0;             // thread 0's
    for (int j = 0; j < a.m; ++j) {
        const double nj = (double)(j + 1);
        unsigned long long key = ~0ull, idx = ~0ull;
#pragma unroll
        for (int k = 0; k < COMPRESS_HERD_OWN; ++k)
            if ((live >> k) & 1u) {
                const double q = r[k] / nj;
                const unsigned long long kk = compress_key(mu[k] - q);
                if (kk < key) { key = kk; idx = (unsigned long long)(tid + COMPRESS_HERD_THREADS * k); }   // ascending c: the first of equals stays
            }
        wg_min_pair<COMPRESS_HERD_THREADS>(ka, kb, key, idx);
        if (idx == ~0ull) return;               // no candidate left (the host refuses m > present): the same on every thread
        const int x = (int)idx;
        if (tid == x % COMPRESS_HERD_THREADS) {
            const int kx = x / COMPRESS_HERD_THREADS;
#pragma unroll
            for (int k = 0; k < COMPRESS_HERD_OWN; ++k)
                if (k == kx) { pub[0] = r[k]; pub[1] = mu[k]; live &= ~(1u << k); }
        }
        __syncthreads();
        if (tid == 0) {                         // pub is written again only behind the barriers of the next wg_min_pair
            musum = musum + pub[1];
            pair = pair + 2.0 * pub[0];
            a.picks[j] = x;
            a.energy[j] = compress_energy(musum, pair, nj, d0);
            a.score[j] = compress_unkey(key);
        }
        const double* row = a.sq + (size_t)x * a.U;
#pragma unroll
        for (int k = 0; k < COMPRESS_HERD_OWN; ++k)
            if ((live >> k) & 1u) r[k] = r[k] + __dsqrt_rn(row[tid + COMPRESS_HERD_THREADS * k]);
    }
}

struct CompressSubset {
    const double* sq;           // [U][U]
    const double* mu;           // [U]
    const double* d0;           // [1]
    const int* item_sample;     // [n_items], or null: item k is sample k
    const int* items;           // [B][mb] item indices, checked by the host (in range, no absent sample)
    int U, mb;
    double* energy;             // [B]
};

__global__ void __launch_bounds__(COMPRESS_THREADS) compress_subset_kernel(const CompressSubset a) {
#pragma clang fp contract(off)
    __shared__ double rd[COMPRESS_THREADS];
    const int tid = threadIdx.x;
    const int* it = a.items + (size_t)blockIdx.x * a.mb;
    const auto sample = [&](long long k) { const int i = it[k]; return a.item_sample ? a.item_sample[i] : i; };
    double smu = 0.0, sd = 0.0;
    for (int k = tid; k < a.mb; k += COMPRESS_THREADS) smu = smu + a.mu[sample(k)];
    const long long pairs = (long long)a.mb * a.mb;
    for (long long p = tid; p < pairs; p += COMPRESS_THREADS)
        sd = sd + __dsqrt_rn(a.sq[(size_t)sample(p / a.mb) * a.U + sample(p % a.mb)]);
    smu = wg_sum<COMPRESS_THREADS>(rd, smu);
    sd = wg_sum<COMPRESS_THREADS>(rd, sd);
    if (tid == 0) a.energy[blockIdx.x] = compress_energy(smu, sd, (double)a.mb, a.d0[0]);
}
