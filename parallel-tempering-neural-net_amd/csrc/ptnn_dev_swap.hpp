// ptnn_dev_swap.hpp -- the non-template kernels of the sampler (textually included by ptnn.hip, inside namespace ptnn, after
// ptnn_shapes.hpp; not a stand-alone header): xchg_pack_kernel, chain_reset_kernel, swap_kernel.  The object that includes this
// file holds them.

// mode bit 0: apply the local moves; bit 1: count the round and log it
// exchange row of every local replica: state, cached gradient, its valid flag and the posted scalar, ready for the all-gather
__global__ void xchg_pack_kernel(const SwapParams sp) {
    const int b = blockIdx.x;
    float* row = sp.xchg + (size_t)(sp.first_global + b) * sp.XS;
    const float* from = sp.cur + (size_t)b * sp.PS;
    const float* gfrom = sp.gd_cur + (size_t)b * sp.PS;
    for (int j = threadIdx.x; j < sp.PS; j += blockDim.x) { row[j] = from[j]; row[sp.PS + j] = gfrom[j]; }
    if (threadIdx.x == 0) {
        row[2 * sp.PS] = sp.gd_valid_cur[b] ? 1.0f : 0.0f;
        row[2 * sp.PS + 1] = sp.L[sp.first_global + b];
        if (sp.rule == 1) {
            row[2 * sp.PS + 2] = sp.L_raw[sp.first_global + b];
            row[2 * sp.PS + 3] = sp.prior_post[sp.first_global + b];
        }
    }
}

// Restart of the chains (ptnn_set_state), one block per local replica, everything a run starts from in ONE kernel on the handle's
// stream: the initial weights into both state buffers (REG:649), the recorded row = ones and row 0 of every trace (Q7: pos_w =
// ones, REG:240; likeh = -100, REG:292-293; the rest zero), the cached-gradient rows and flags, the per-chain scalars and
// counters, the temperatures, the error flag, the swap counters and the identity slot <-> temperature maps.  (It was some twenty
// blocking copies and fills on the null stream, two of them hipMemcpy2D calls with the trace ring's pitch -- 74 MB for Ionosphere,
// where a restart cost 25 ms: a fifth of a whole 256-replica run, profiles/r03a_gap_probe_before.json.)
struct ResetParams {
    int R, Rl, P, PS, PW;
    size_t cap;
    const float* w0;          // [Rl][P]  staged initial weights
    const float* temps_in;    // [Rl]
    float *state0, *state1, *rec_w, *gd0, *gd1, *st_f, *temps, *pos_w, *scal;
    int *gd_valid0, *gd_valid1, *st_i, *error, *label0, *label1, *slot0, *slot1;
    long long* counters;
};
__global__ void chain_reset_kernel(const ResetParams q) {
    const int r = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const size_t row = (size_t)r * q.PS;
    for (int j = tid; j < q.PS; j += nthr) {
        const float v = (j < q.P) ? q.w0[(size_t)r * q.P + j] : 0.0f;
        q.state0[row + j] = v; q.state1[row + j] = v;
        q.rec_w[row + j] = 1.0f;
        q.gd0[row + j] = 0.0f; q.gd1[row + j] = 0.0f;
    }
    float* prow = q.pos_w + (size_t)r * q.cap * q.PW;
    for (int j = tid; j < q.PW; j += nthr) prow[j] = (j < q.P) ? 1.0f : 0.0f;
    if (tid == 0) {
        store_trace_row(q.scal + (size_t)r * q.cap * TR_COUNT, -100.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0.0f);
        q.gd_valid0[r] = 0; q.gd_valid1[r] = 0;
        q.temps[r] = q.temps_in[r];
    }
    if (tid < SF_COUNT) q.st_f[(size_t)r * SF_COUNT + tid] = 0.0f;
    if (tid < SI_COUNT) q.st_i[(size_t)r * SI_COUNT + tid] = 0;
    if (r == 0) {
        if (tid == 0) { q.counters[0] = 0; q.counters[1] = 0; *q.error = 0; }
        for (int k = tid; k < q.R; k += nthr) { q.label0[k] = k; q.label1[k] = k; q.slot0[k] = k; q.slot1[k] = k; }
    }
}

__global__ void swap_kernel(const SwapParams sp, const int round, const int mode) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    swap_block(sp, round, mode, blockIdx.x, smem);
}

