// ptnn_dev_wg.hpp -- the work-group and wave reductions and scans of the analysis kernels (textually included inside namespace ptnn).
// One fixed order each, so that a result depends on the values and N only: an LDS tree over N = the work-group's thread count
// (a power of two) values, a Hillis-Steele scan, the 64-lane butterfly.  An operator updates its first argument in place.
#pragma once

// the tree alone: step(i, i + d) on threads i < d for d = N / 2 ... 1, a barrier after every level.  The caller has stored its
// values and synchronised; several arrays may go down one tree.
template <int N, class Step>
__device__ __forceinline__ void wg_tree(Step step) {
    const int tid = threadIdx.x;
    for (int d = N / 2; d > 0; d >>= 1) {
        if (tid < d) step(tid, tid + d);
        __syncthreads();
    }
}

// one value per thread through buf [N]; every thread gets the result; a barrier before and after
template <int N, class T, class Op>
__device__ T wg_reduce(T* buf, T v, Op op) {
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    wg_tree<N>([&](int i, int j) { op(buf[i], buf[j]); });
    v = buf[0];
    __syncthreads();
    return v;
}
template <int N, class T> __device__ T wg_sum(T* buf, T v) { return wg_reduce<N>(buf, v, [](T& a, T b) { a += b; }); }
template <int N> __device__ double wg_max(double* buf, double v) { return wg_reduce<N>(buf, v, [](double& a, double b) { a = fmax(a, b); }); }

// the two-word forms.  Fix128: a 128-bit fixed-point sum in units of 2^-62 (ptnn_dev_elpd.hpp: fix_add)
struct Fix128 { unsigned long long lo, hi; };
template <int N>
__device__ __forceinline__ void wg_fix_tree(unsigned long long* r0, unsigned long long* r1) {      // r1:r0 [i] += r1:r0 [j], with the carry
    wg_tree<N>([&](int i, int j) {
        const unsigned long long lo = r0[i] + r0[j];
        r1[i] += r1[j] + (lo < r0[i] ? 1ull : 0ull);
        r0[i] = lo;
    });
}
template <int N>
__device__ double wg_fix_sum(unsigned long long* r0, unsigned long long* r1, Fix128 a) {
    const int tid = threadIdx.x;
    __syncthreads();
    r0[tid] = a.lo; r1[tid] = a.hi;
    __syncthreads();
    wg_fix_tree<N>(r0, r1);
    const double v = ((double)r1[0] * 0x1p64 + (double)r0[0]) * 0x1p-62;
    __syncthreads();
    return v;
}
template <int N>
__device__ void wg_min_max(double* a, double* b, double& mn, double& mx) {      // mn = the smallest mn, mx = the largest mx
    const int tid = threadIdx.x;
    __syncthreads();
    a[tid] = mn; b[tid] = mx;
    __syncthreads();
    wg_tree<N>([&](int i, int j) { a[i] = fmin(a[i], a[j]); b[i] = fmax(b[i], b[j]); });
    mn = a[0]; mx = b[0];
    __syncthreads();
}
// the lexicographically smallest pair (key, idx) of the work-group, as one 128-bit unsigned compare; every thread gets it
template <int N>
__device__ void wg_min_pair(unsigned long long* a, unsigned long long* b, unsigned long long& key, unsigned long long& idx) {
    const int tid = threadIdx.x;
    __syncthreads();
    a[tid] = key; b[tid] = idx;
    __syncthreads();
    wg_tree<N>([&](int i, int j) {
        if (a[j] < a[i] || (a[j] == a[i] && b[j] < b[i])) { a[i] = a[j]; b[i] = b[j]; }
    });
    key = a[0]; idx = b[0];
    __syncthreads();
}

// inclusive scan in thread order of a [N] (and b [N] beside it), stored and synchronised by the caller: log2 N steps
template <int N, class T>
__device__ __forceinline__ void wg_incl_scan(T* a, int tid) {
    for (int d = 1; d < N; d <<= 1) {
        const T add = tid >= d ? a[tid - d] : T(0);
        __syncthreads();
        a[tid] += add;
        __syncthreads();
    }
}
template <int N, class T>
__device__ __forceinline__ void wg_incl_scan(T* a, T* b, int tid) {
    for (int d = 1; d < N; d <<= 1) {
        const T add_a = tid >= d ? a[tid - d] : T(0), add_b = tid >= d ? b[tid - d] : T(0);
        __syncthreads();
        a[tid] += add_a; b[tid] += add_b;
        __syncthreads();
    }
}

// the butterfly over the 64 lanes of a wave (xor 32 ... 1): every lane ends with the same bits (a + b and b + a are the same)
template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) op(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return wave_all(v, [](double& a, double b) { a += b; }); }
__device__ __forceinline__ long long wave_sum(long long v) { return wave_all(v, [](long long& a, long long b) { a += b; }); }
__device__ __forceinline__ double wave_min(double v) { return wave_all(v, [](double& a, double b) { a = fmin(a, b); }); }
__device__ __forceinline__ double wave_max(double v) { return wave_all(v, [](double& a, double b) { a = fmax(a, b); }); }
