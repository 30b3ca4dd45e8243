// ptnn_dev_influence.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// case influence, the covariance over the samples of every target column with every case's log-likelihood (ptnn_influence,
// include/ptnn.h).  Shape-independent kernels only: no per-shape code object includes this file.
//   a. + b. as ptnn_elpd: distinct_samples (with the eta compare), the per-shape predict_forward_kernel; the case columns
//      B [n_b][U] are elpd_loglik_kernel's (ptnn_dev_elpd.hpp: elpd_ll, unchanged), the target columns A [n_a][U] the fp32
//      outputs widened (influence_widen_kernel) or elpd_loglik_kernel's on the target rows.
//   c. influence_moments_kernel: one work-group per column; the smallest value, the weighted mean and the weighted sum of squared
//      deviations from it, each sum a strided partial per thread and the LDS tree of wg_sum: the order depends on U only.
//   d. influence_cov_kernel: C = sum_u cnt_u (A - mean_a)(B - mean_b), a tiled "NT" GEMM in FP64 FMA with both operands
//      contiguous in u; one work-group per (64 x 64 output tile, chunk of INFL_KCHUNK samples), the partial tile to scratch;
//      influence_finish_kernel adds the partials of a tile in chunk order and divides by M - 1.
// Every element is the sum, in ascending u within a chunk and ascending chunk, of its own products: its bits depend on its two
// columns, cnt and U -- not on the tile it falls in, the row blocks, the grid or the scratch budget.  No atomics; fp64 throughout.
// Nothing here writes chain state, tapes, counters or trace rows.

constexpr int INFL_THREADS = 256;         // 4 waves: a 16 x 16 grid of threads, a 4 x 4 patch of the output tile each
constexpr int INFL_TILE = 64;             // output tile edge
constexpr int INFL_KT = 32;               // samples staged in LDS per step
constexpr int INFL_KCHUNK = 512;          // samples per partial (a multiple of INFL_KT): fixed, so that a sum's order depends on U only
constexpr int INFL_LD = INFL_TILE + 2;    // LDS row pitch in doubles: 528 bytes, rows stay 16-byte aligned for the 128-bit reads
constexpr int INFL_PATCH = INFL_TILE / 16;
static_assert(INFL_KCHUNK % INFL_KT == 0 && INFL_THREADS % INFL_KT == 0 && INFL_PATCH == 4, "influence tile geometry");

// fp32 network outputs [n] -> double
__global__ void __launch_bounds__(INFL_THREADS) influence_widen_kernel(const float* src, double* dst, long long n) {
    const long long i = (long long)blockIdx.x * INFL_THREADS + threadIdx.x;
    if (i < n) dst[i] = (double)src[i];
}

struct InflMoments {
    const double* v;            // [ncols][U] the columns of a block
    const int* cnt;             // [U] multiplicities (0 = absent)
    int U;
    long long M;                // expanded sample count (>= 2)
    double* mean;               // [ncols] at blockIdx.x
    double* ssd;                // [ncols] sum cnt (v - mean)^2
};

// Sums are taken of v - min: a constant column has the mean of its value and deviations of exactly 0, and integer columns whose
// sums stay below 2^53 are summed exactly.
__global__ void __launch_bounds__(INFL_THREADS) influence_moments_kernel(const InflMoments a) {
    __shared__ double r0[INFL_THREADS], r1[INFL_THREADS];
    const int tid = threadIdx.x;
    const double* v = a.v + (size_t)blockIdx.x * a.U;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double mn = INF, mx = -INF;
    for (int u = tid; u < a.U; u += INFL_THREADS)
        if (a.cnt[u] != 0) { mn = fmin(mn, v[u]); mx = fmax(mx, v[u]); }
    wg_min_max<INFL_THREADS>(r0, r1, mn, mx);
    double s = 0.0;
    for (int u = tid; u < a.U; u += INFL_THREADS) {
        const int c = a.cnt[u];
        if (c != 0) s += (double)c * (v[u] - mn);
    }
    s = wg_sum<INFL_THREADS>(r0, s);
    const double mean = fmin(fmax(mn + s / (double)a.M, mn), mx);
    double q = 0.0;
    for (int u = tid; u < a.U; u += INFL_THREADS) {
        const int c = a.cnt[u];
        if (c != 0) { const double d = v[u] - mean; q += (double)c * (d * d); }
    }
    q = wg_sum<INFL_THREADS>(r0, q);
    if (tid == 0) { a.mean[blockIdx.x] = mean; a.ssd[blockIdx.x] = q; }
}

struct InflCov {
    const double *A, *B;        // [na][U], [nb][U]: the columns of the two blocks
    const double *mean_a, *mean_b;   // [na], [nb] their means
    const int* cnt;             // [U]
    int na, nb, U;
    int tiles_b;                // tiles along b: tile t covers rows 64 (t / tiles_b) of A and 64 (t % tiles_b) of B
    int tile0;                  // the first tile of this launch (blockIdx.x counts from it)
    int nchunks;                // ceil(U / INFL_KCHUNK) = gridDim.y
    double* part;               // [gridDim.x][nchunks][64 * 64] partial tiles
};

// grid (tiles of the launch, chunks).  Staging: thread t loads sample t % 32 of rows t / 32 + 8 p of either operand (32 lanes read
// 256 contiguous bytes of a column), centres it, gives A's the cnt factor and stores it transposed, [sample][row]; rows past the
// block, samples past the chunk and absent samples are staged as 0 and add nothing.  Product: thread (ty, tx) reads its four A
// rows and four B rows of a sample as two 128-bit LDS reads each and issues 16 FMAs.
__global__ void __launch_bounds__(INFL_THREADS) influence_cov_kernel(const InflCov a) {
    __shared__ __align__(16) double As[INFL_KT][INFL_LD];
    __shared__ __align__(16) double Bs[INFL_KT][INFL_LD];
    constexpr int RPP = INFL_THREADS / INFL_KT, PASSES = INFL_TILE / RPP;       // 8 rows per pass, 8 passes
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int sk = tid % INFL_KT, sr = tid / INFL_KT;
    const int tile = a.tile0 + (int)blockIdx.x, chunk = (int)blockIdx.y;
    const int a0 = (tile / a.tiles_b) * INFL_TILE, b0 = (tile % a.tiles_b) * INFL_TILE;
    const int u_begin = chunk * INFL_KCHUNK, u_end = min(a.U, u_begin + INFL_KCHUNK);
    double ma[PASSES], mb[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int ra = a0 + sr + RPP * p, rb = b0 + sr + RPP * p;
        ma[p] = ra < a.na ? a.mean_a[ra] : 0.0;
        mb[p] = rb < a.nb ? a.mean_b[rb] : 0.0;
    }
    double acc[INFL_PATCH][INFL_PATCH];
#pragma unroll
    for (int i = 0; i < INFL_PATCH; ++i)
#pragma unroll
        for (int j = 0; j < INFL_PATCH; ++j) acc[i][j] = 0.0;

    for (int u0 = u_begin; u0 < u_end; u0 += INFL_KT) {
        const int u = u0 + sk;
        const int c = u < u_end ? a.cnt[u] : 0;
        const double cd = (double)c;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int r = sr + RPP * p, ra = a0 + r, rb = b0 + r;
            As[sk][r] = (c != 0 && ra < a.na) ? cd * (a.A[(size_t)ra * a.U + u] - ma[p]) : 0.0;
            Bs[sk][r] = (c != 0 && rb < a.nb) ? a.B[(size_t)rb * a.U + u] - mb[p] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < INFL_KT; ++k) {
            const double2* pa = reinterpret_cast<const double2*>(&As[k][ty * INFL_PATCH]);
            const double2* pb = reinterpret_cast<const double2*>(&Bs[k][tx * INFL_PATCH]);
            const double2 a01 = pa[0], a23 = pa[1], b01 = pb[0], b23 = pb[1];
            const double av[INFL_PATCH] = {a01.x, a01.y, a23.x, a23.y}, bv[INFL_PATCH] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int i = 0; i < INFL_PATCH; ++i)
#pragma unroll
                for (int j = 0; j < INFL_PATCH; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    double* out = a.part + ((size_t)blockIdx.x * a.nchunks + chunk) * (INFL_TILE * INFL_TILE);
#pragma unroll
    for (int i = 0; i < INFL_PATCH; ++i) {
        double2* row = reinterpret_cast<double2*>(out + (ty * INFL_PATCH + i) * INFL_TILE + tx * INFL_PATCH);
        row[0] = make_double2(acc[i][0], acc[i][1]);
        row[1] = make_double2(acc[i][2], acc[i][3]);
    }
}

struct InflFinish {
    const double* part;         // influence_cov_kernel's
    int nchunks, tiles_b, tile0, na, nb;
    long long ldc;              // row pitch of C
    double denom;               // M - 1
    double* C;                  // the block's corner: element (i, j) of the block at C[i * ldc + j]
};

// grid (tiles of the launch, 16): one thread per element of the tile, the partials added in chunk order
__global__ void __launch_bounds__(INFL_THREADS) influence_finish_kernel(const InflFinish a) {
    const int e = (int)blockIdx.y * INFL_THREADS + threadIdx.x;
    const int tile = a.tile0 + (int)blockIdx.x;
    const int i = (tile / a.tiles_b) * INFL_TILE + e / INFL_TILE, j = (tile % a.tiles_b) * INFL_TILE + e % INFL_TILE;
    if (i >= a.na || j >= a.nb) return;
    const double* p = a.part + (size_t)blockIdx.x * a.nchunks * (INFL_TILE * INFL_TILE) + e;
    double s = p[0];
    for (int c = 1; c < a.nchunks; ++c) s += p[(size_t)c * (INFL_TILE * INFL_TILE)];
    a.C[(size_t)i * a.ldc + j] = s / a.denom;
}
