// ptnn_dev_modes.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn; not a stand-alone header):
// posterior modes, the all-pairs function-space distance of the sampled nets and the density-peaks stage on it (ptnn_modes,
// include/ptnn.h).  Shape-independent kernels only: no per-shape code object includes this file.
//   a. + b. as ptnn_predict: distinct_samples, the per-shape predict_forward_kernel -> fx [col][U] fp32, a block of columns at a
//      time; a host matrix is staged in the same layout.
//   c. modes_dist_kernel: sq[u, v] += sum over the block's columns of (F[u, j] - F[v, j])^2, both values widened to double, every
//      term one fma(d, d, acc); one accumulator per element, carried in the matrix across the column blocks, columns ascending.
//      One work-group per 64 x 64 tile with tile row <= tile column; the mirror tile is written from the same registers.
//   d. modes_density_kernel: one work-group per row: rho_u = sum_v c_v [sq <= near_sq], the row's largest sq, its count of
//      non-finite elements and its share of sum_u sum_v c_u c_v sq; the work-group that finishes last adds the shares in row order.
//   e. modes_parent_kernel: one work-group per row: the lexicographic minimum of (bits of sq[u, v], v) over the v that precede u.
// An element of sq is the sum, in ascending column order, of its own terms: its bits depend on the two output vectors and the
// number of columns -- not on the tile, the column blocks, the grid or the scratch budget.  No value passes through an atomic: the
// one atomic is the ticket that elects the finishing work-group of d.  Nothing here writes chain state, tapes, counters or trace
// rows.

constexpr int MODES_THREADS = 256;        // 4 waves: a 16 x 16 grid of threads, a 4 x 4 patch of the tile each
constexpr int MODES_TILE = 64;            // tile edge
constexpr int MODES_KT = 32;              // columns staged in LDS per step
constexpr int MODES_LD = MODES_TILE + 2;  // LDS row pitch in doubles: 528 bytes, rows stay 16-byte aligned for the 128-bit reads
constexpr int MODES_PATCH = MODES_TILE / 16;
static_assert(MODES_THREADS % MODES_TILE == 0 && MODES_KT % (MODES_THREADS / MODES_TILE) == 0 && MODES_PATCH == 4, "modes tile geometry");

// fx [nc][U] of one block -> out [U][n] at columns [c0, c0 + nc): the outputs of every distinct sample, row-major
__global__ void __launch_bounds__(MODES_THREADS) modes_outputs_kernel(const float* fx, long long n, long long c0, int nc, int U, float* out) {
    const long long i = (long long)blockIdx.x * MODES_THREADS + threadIdx.x;
    if (i >= (long long)nc * U) return;
    const long long c = i / U, u = i % U;
    out[u * n + c0 + c] = fx[i];
}

struct ModesDist {
    const float* fx;            // [nc][U] the block's columns, each contiguous in u
    int nc, U;
    int T;                      // tiles per edge, ceil(U / 64); the grid is the T (T + 1) / 2 tiles with row <= column
    int first;                  // the first column block: the accumulators start at 0, else at the matrix's contents
    double* sq;                 // [U][U]
};

// Staging: thread t loads sample t % 64 of columns t / 64 + 4 p of either operand (64 lanes read 256 contiguous bytes of a
// column), widens it and stores it [column][sample]; samples past U and columns past the block are staged as 0 on both sides: their
// difference is 0 and fma(0, 0, acc) = acc.  Product: thread (ty, tx) reads its four rows and four columns of a staged column as
// two 128-bit LDS reads each and issues 16 subtractions and 16 FMAs.
__global__ void __launch_bounds__(MODES_THREADS) modes_dist_kernel(const ModesDist a) {
    __shared__ __align__(16) double As[MODES_KT][MODES_LD];
    __shared__ __align__(16) double Bs[MODES_KT][MODES_LD];
    constexpr int CPP = MODES_THREADS / MODES_TILE, PASSES = MODES_KT / CPP;    // 4 columns per pass, 8 passes
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int sr = tid % MODES_TILE, sk = tid / MODES_TILE;
    int ti = 0, rem = (int)blockIdx.x;
    while (rem >= a.T - ti) { rem -= a.T - ti; ++ti; }
    const int tj = ti + rem;
    const int i0 = ti * MODES_TILE, j0 = tj * MODES_TILE;
    double acc[MODES_PATCH][MODES_PATCH];
#pragma unroll
    for (int i = 0; i < MODES_PATCH; ++i)
#pragma unroll
        for (int j = 0; j < MODES_PATCH; ++j) {
            const int u = i0 + ty * MODES_PATCH + i, v = j0 + tx * MODES_PATCH + j;
            acc[i][j] = (!a.first && u < a.U && v < a.U) ? a.sq[(size_t)u * a.U + v] : 0.0;
        }
    const bool in_a = i0 + sr < a.U, in_b = j0 + sr < a.U;
    for (int c0 = 0; c0 < a.nc; c0 += MODES_KT) {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int k = sk + CPP * p, c = c0 + k;
            const float* col = a.fx + (size_t)c * a.U;
            As[k][sr] = (c < a.nc && in_a) ? (double)col[i0 + sr] : 0.0;
            Bs[k][sr] = (c < a.nc && in_b) ? (double)col[j0 + sr] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < MODES_KT; ++k) {
            const double2* pa = reinterpret_cast<const double2*>(&As[k][ty * MODES_PATCH]);
            const double2* pb = reinterpret_cast<const double2*>(&Bs[k][tx * MODES_PATCH]);
            const double2 a01 = pa[0], a23 = pa[1], b01 = pb[0], b23 = pb[1];
            const double av[MODES_PATCH] = {a01.x, a01.y, a23.x, a23.y}, bv[MODES_PATCH] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int i = 0; i < MODES_PATCH; ++i)
#pragma unroll
                for (int j = 0; j < MODES_PATCH; ++j) {
                    const double d = av[i] - bv[j];
                    acc[i][j] = fma(d, d, acc[i][j]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MODES_PATCH; ++i)
#pragma unroll
        for (int j = 0; j < MODES_PATCH; ++j) {
            const int u = i0 + ty * MODES_PATCH + i, v = j0 + tx * MODES_PATCH + j;
            if (u < a.U && v < a.U) {
                a.sq[(size_t)u * a.U + v] = acc[i][j];
                if (ti != tj) a.sq[(size_t)v * a.U + u] = acc[i][j];     // (a - b)^2 = (b - a)^2; a diagonal tile holds both halves
            }
        }
}

struct ModesDensity {
    const double* sq;           // [U][U]
    const int* cnt;             // [U] multiplicities (0 = absent)
    int U;
    double near_sq;             // radius^2 n
    double mm;                  // M^2 as a double
    long long* rho;             // [U]
    double* row_max;            // [U] the largest sq[u, v] over the present v
    double* row_part;           // [U] c_u sum_v c_v sq[u, v]
    long long* row_bad;         // [U] non-finite elements among the present v; + 2^40 when sq[u, u] is one of them
    unsigned int* ticket;       // 0 before the launch
    double* spread_sq;          // [1]
    long long* bad;             // [2] non-finite elements, and the first sample with a non-finite sq[u, u] (else the first such row, else -1)
};

__global__ void __launch_bounds__(MODES_THREADS) modes_density_kernel(const ModesDensity a) {
    __shared__ double rd[MODES_THREADS];
    __shared__ long long rl[MODES_THREADS];
    __shared__ unsigned int last;
    const int tid = threadIdx.x, u = (int)blockIdx.x;
    const double* row = a.sq + (size_t)u * a.U;
    const int cu = a.cnt[u];
    long long rho = 0, nbad = 0;
    double part = 0.0, mx = 0.0;
    if (cu != 0)
        for (int v = tid; v < a.U; v += MODES_THREADS) {
            const int c = a.cnt[v];
            if (c == 0) continue;
            const double s = row[v];
            if (!(fabs(s) <= 1.7976931348623157e308)) { ++nbad; continue; }
            if (s <= a.near_sq) rho += c;
            part += (double)c * s;
            mx = fmax(mx, s);
        }
    rho = wg_sum<MODES_THREADS>(rl, rho);
    nbad = wg_sum<MODES_THREADS>(rl, nbad);
    part = wg_sum<MODES_THREADS>(rd, part);
    mx = wg_max<MODES_THREADS>(rd, mx);
    if (tid == 0) {
        const bool diag = cu != 0 && !(fabs(row[u]) <= 1.7976931348623157e308);
        a.rho[u] = rho;
        a.row_max[u] = mx;
        a.row_part[u] = (double)cu * part;
        a.row_bad[u] = nbad + (diag ? (1ll << 40) : 0);
        __threadfence();
        last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;                          // `last` is shared: the whole work-group leaves or stays
    __threadfence();
    // The finishing work-group: 256 rows at a time are fetched by all threads into LDS and added by one, in row order, so that the
    // sum's bits depend on the matrix and the counts only
    const volatile double* part_v = a.row_part;
    const volatile long long* bad_v = a.row_bad;
    double s = 0.0;
    long long bad = 0, first_diag = -1, first_row = -1;
    for (int r0 = 0; r0 < a.U; r0 += MODES_THREADS) {
        const int r = r0 + tid, nr = min(MODES_THREADS, a.U - r0);
        if (tid < nr) { rd[tid] = part_v[r]; rl[tid] = bad_v[r]; }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < nr; ++k) {
                s += rd[k];
                const long long b = rl[k];
                if (b != 0 && first_row < 0) first_row = r0 + k;
                if (b >= (1ll << 40) && first_diag < 0) first_diag = r0 + k;
                bad += b & ((1ll << 40) - 1);
            }
        __syncthreads();
    }
    if (tid != 0) return;
    a.spread_sq[0] = s / a.mm;
    a.bad[0] = bad;
    a.bad[1] = first_diag >= 0 ? first_diag : first_row;
}

struct ModesParent {
    const double* sq;           // [U][U]
    const int* cnt;             // [U]
    const long long* rho;       // [U]
    const double* row_max;      // [U]
    int U;
    int* parent;                // [U]
    double* delta_sq;           // [U]
};

// v precedes u iff rho_v > rho_u, or rho_v = rho_u and v < u (present samples only).  The bits of a non-negative double order as the
// values do, so the lexicographic minimum of (bits, v) is the smallest sq and, among equals, the lowest v.
__global__ void __launch_bounds__(MODES_THREADS) modes_parent_kernel(const ModesParent a) {
    __shared__ unsigned long long r0[MODES_THREADS], r1[MODES_THREADS];
    const int tid = threadIdx.x, u = (int)blockIdx.x;
    if (a.cnt[u] == 0) {
        if (tid == 0) { a.parent[u] = -1; a.delta_sq[u] = 0.0; }
        return;
    }
    const double* row = a.sq + (size_t)u * a.U;
    const long long ru = a.rho[u];
    unsigned long long key = ~0ull, idx = ~0ull;
    for (int v = tid; v < a.U; v += MODES_THREADS) {
        if (a.cnt[v] == 0) continue;
        const long long rv = a.rho[v];
        if (!(rv > ru || (rv == ru && v < u))) continue;
        const unsigned long long k = (unsigned long long)__double_as_longlong(row[v]);
        if (k < key) { key = k; idx = (unsigned long long)v; }      // ascending v: the first of equals stays
    }
    wg_min_pair<MODES_THREADS>(r0, r1, key, idx);
    if (tid == 0) {
        const bool none = idx == ~0ull;
        a.parent[u] = none ? -1 : (int)idx;
        a.delta_sq[u] = none ? a.row_max[u] : __longlong_as_double((long long)key);
    }
}
