// Ladder adaptation during burn-in (swap_rule 1; ptnn_set_ladder_adaptation).  Included by
// ptnn_dev_wide.hpp inside its fp-contract(off) section, right above swap_block, its only caller.
//
// Round t (< A) of the even/odd exchange moves the log-gaps s_k = log(T_k+1 - T_k) by kappa(t) (a_k(t) - mean a), with a_k(t) the
// Rao-Blackwellised acceptance of EVERY adjacent pair under the ladder the round's own test used, and rescales the gaps so that
// the ladder runs from 1 to the fixed T_max.  Every block of the round recomputes the update from the same inputs in the same
// order (the order depends on R only: wave 0, lane-strided partial sums, a fixed shuffle tree, fixed 64-lane chunks for the
// prefix sum), so every block -- of one launch, of a persistent body, of another handle holding another block of the ladder --
// arrives at the same ladder bit for bit.  Block 0 records it.
//
// Ownership of the buffers (no round ever writes what another block of the same round reads):
//   lad_hist [A+1][R]  ladders; round t reads row min(t, A) (the host and persistent_loop point temps_global at it), writes t+1
//   lad_s    [2][R-1]  log-gaps in double; round t reads row t & 1, block 0 writes row (t + 1) & 1
//   lad_acc  [cap][R-1] a_k(t) of every round, adapted or not (block 0)
//   lad_out  [R]       the newest ladder (the handle's d_temps_global, which nothing reads while adaptation is on)

// a_k(t) of every adjacent pair into sA[0 .. R-2], recorded by block 0.  When round < A: the new ladder into sT[0 .. R-1], the
// new log-gaps and ladder row by block 0, and true.  Every thread of the block calls it (it synchronises).  Not inlined, and
// handed scalars and pointers rather than the SwapParams: inlined into the persistent bodies it cost them 10 - 22 vector
// registers (and the packed kernel a spill), with a reference to the SwapParams it put a copy of them on the stack.
__device__ __noinline__ bool ladder_round(const int R, const int round, const int b, const int label_mode, const int* __restrict__ slot_cur,
                                          const float* __restrict__ temps, const float* __restrict__ L_raw, const int L_stride,
                                          const int A, const int acc_cap, const double kappa0, const double t0, float* __restrict__ hist,
                                          double* __restrict__ lad_s, float* __restrict__ lad_acc, float* __restrict__ lad_out,
                                          float* sA, float* sT) {
    const int n = R - 1;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        // exactly the exchange test's pr (cascade_lds), for both parities
        const int s0 = label_mode ? slot_cur[k] : k, s1 = label_mode ? slot_cur[k + 1] : k + 1;
        const float d = (1.0f / temps[k] - 1.0f / temps[k + 1]) * (L_raw[(size_t)s1 * L_stride] - L_raw[(size_t)s0 * L_stride]);
        const float a = (d != d) ? 1.0f : fminf(1.0f, expf_fast(fminf(d, 80.0f)));
        sA[k] = a;
        if (b == 0 && round < acc_cap) lad_acc[(size_t)round * n + k] = a;
    }
    __syncthreads();
    if (round >= A) return false;
    if (threadIdx.x < WAVE) {
        const int lane = threadIdx.x;
        double part = 0.0;
        for (int k = lane; k < n; k += WAVE) part += (double)sA[k];
        part = wave_sum(part);                                                  // a + b == b + a: every lane holds the same sum
        const double abar = part / (double)n;
        const double kap = kappa0 * t0 / ((double)round + t0);
        const double* s_old = lad_s + (size_t)(round & 1) * n;
        double* s_new = lad_s + (size_t)((round + 1) & 1) * n;
        // lane l owns the pairs [l c, (l + 1) c): chunk sums, an inclusive scan over the lanes, then the prefix within the chunk
        const int c = (n + WAVE - 1) / WAVE;
        const int k0 = min(n, lane * c), k1 = min(n, k0 + c);
        double g = 0.0;
        for (int k = k0; k < k1; ++k) g += exp(s_old[k] + kap * ((double)sA[k] - abar));
        double incl = g;
        for (int o = 1; o < WAVE; o <<= 1) {
            const double v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        const double total = __shfl(incl, WAVE - 1);
        const double up = __shfl_up(incl, 1);
        double acc = lane == 0 ? 0.0 : up;
        const float tmax = temps[n];
        const double scale = ((double)tmax - 1.0) / total;
        for (int k = k0; k < k1; ++k) {
            const double sk = s_old[k] + kap * ((double)sA[k] - abar);
            acc += exp(sk);
            if (b == 0) s_new[k] = sk;
            sT[k + 1] = (k + 1 == n) ? tmax : (float)(1.0 + scale * acc);
        }
        if (lane == 0) sT[0] = 1.0f;
    }
    __syncthreads();
    if (b == 0)
        for (int k = threadIdx.x; k < R; k += blockDim.x) {
            hist[(size_t)(round + 1) * R + k] = sT[k];
            lad_out[k] = sT[k];
        }
    return true;
}
