// ptnn_dev_shapley.hpp -- part of ptnn_analysis_device.hpp (textually included there, inside namespace ptnn; not a stand-alone header):
// coalition values of the sampled nets and linear functionals of them (ptnn_coalition_values, include/ptnn.h; DESIGN.md section 29;
// Shapley 1953, Strumbelj & Kononenko 2014, Lundberg & Lee 2017: the interventional value function).  Nothing of the kind is in
// the reference.
//
//   h(x, b, S)_i   = x_i if bit i of S is set, else b_i         the hybrid row: exact fp32 values, a select, nothing rebuilt by arithmetic
//   v_s[n, S, o]   = (1/B) sum_b f_o(w_s; h(x_n, b, S))         f in fp32 as ptnn_predict returns it; the sum over b in double
//   out_s[n, o, t] = sum_c coef[c, t] v_s[n, S_c, o]            c = 0 .. C-1 in table order, in double, stored as fp32 once
//
// The device does not know what a Shapley value is: it gets a table of C coalitions (masks [C], coef [C][T]) and evaluates T linear
// functionals of the game v.  The host builds the table (effects.py: shapley_table).
//
// The three stages of ptnn_dev_predict.hpp, with another stage b:
//   b. shapley_forward_kernel<TASK, I, O> (per shape, AnalysisShape::shap_fwd): fx[col][u] = out of distinct vector
//      u, column col = (row * O + o) * T + t of a block of explained rows -- the layout of PredictFwd::fx, so stage c
//      (predict_reduce_kernel, with O = 1 and no votes) takes the columns as it takes the outputs.
//   then per block of rows sensitivity_sign_kernel (out > 0, out < 0 per column) and sensitivity_rows_kernel (|out| summed over the
//   rows per vector and (o, t), in double, carried across the blocks), and at the end sensitivity_mean_kernel: the reductions of
//   ptnn_dev_sensitivity.hpp as they are, with (o, t) where they have (o, i).
// Nothing here writes chain state, tapes, counters or trace rows, and nothing here uses an atomic.
//
// The invariants:
//   - a value f_o(w; h(x, b, S)) is a function of (vector, row, background row, mask) alone: one whole pass over the hidden units in
//     ascending order, z_h summed over the inputs in ascending order, in one lane.  It does not depend on NV, on the rows of a
//     work-group, on the block of rows, on the wave or on the position of the coalition in the table.
//   - v sums the background rows of a chunk of 64 by the fixed butterfly (wave_sum; a lane past the last row adds 0.0) and the
//     chunks in ascending order, so v depends on the background's order and on nothing else; out adds the coalitions in table
//     order, one fma per coalition, so out depends on the table's order and the background's order and on nothing else.
//   - the reductions over the samples depend on the multiset of samples only, as in every other analysis call.
//
// (No ptnn_dev_shapley_reduce.hpp beside this file: the predict and sensitivity reductions provide every reduction this call makes.)

constexpr int SHAP_THREADS = 256;            // 4 waves
constexpr int SHAP_MAX_NV = 8;               // distinct vectors per forward work-group
constexpr int SHAP_ROWS = 4;                 // explained rows per forward work-group
constexpr int SHAP_MAX_COALITIONS = 4096;    // PTNN_SHAP_MAX_COALITIONS
constexpr int SHAP_MAX_BACKGROUND = 256;     // PTNN_SHAP_MAX_BACKGROUND
constexpr int SHAP_MAX_TERMS = 64;           // PTNN_SHAP_MAX_TERMS
constexpr int SHAP_MAX_ACC = 256;            // n_terms * n_out: four accumulators a lane

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: ShapPlan)
struct ShapFwd {
    FwdCommon c;                        // x: the explained rows
    const float* bg;                    // [B][I] background rows
    int B, C, T;                        // background rows, coalitions, terms
    const unsigned long long* masks;    // [C] bit i set: input i from the explained row
    const double* coef;                 // [C][T]
    float* fx;                          // [nrows * O * T][U] column-major
};

// One wave per (distinct vector, explained row) pair, the lanes over the background rows in chunks of 64.  NV vectors staged in
// LDS, every weight read wave-uniform (an LDS broadcast); the explained row and the mask are uniform, the lane's background row
// sits in I registers, the hybrid input is a select.  A work-group takes NV vectors and SHAP_ROWS rows; wave w takes the pairs w,
// w + 4, ...  Per coalition and chunk: one pass over ALL hidden units in ascending order, the output head of ptnn_dev_net.hpp
// (the saturating sigmoids), the O outputs summed over the lanes in double by the butterfly.  The T * O <= 256 accumulators are
// spread over the lanes: lane l owns q = l, l + 64, ... with q = o * T + t, and adds coef[c, t] * v[o] with one fma.
template <int TASK, int I, int O>
__global__ void __launch_bounds__(SHAP_THREADS) shapley_forward_kernel(const ShapFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NWAVE = SHAP_THREADS / WAVE, NACC = SHAP_MAX_ACC / WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FwdCommon& cm = a.c;
    const int NV = cm.NV, PV = cm.PV, H = cm.H, B = a.B, C = a.C, T = a.T, OT = O * T;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, cm.U - u0);
    const int r0 = blockIdx.y * SHAP_ROWS;
    const int nr = min(SHAP_ROWS, cm.nrows - r0);
    float* sv = smem;                                   // [NV][PV] the staged vectors
    stage_vectors<SHAP_THREADS>(sv, cm, u0, nv, tid);
    __syncthreads();
    const int nch = (B + WAVE - 1) / WAVE;              // chunks of background rows
    const double nb = (double)B;
    // the accumulators of this lane: q = lane + 64 k = o * T + t
    int qo[NACC], qt[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const int q = min(lane + WAVE * k, OT - 1);     // past the last accumulator: the last again, not stored
        qo[k] = q / T;
        qt[k] = q - qo[k] * T;
    }
    for (int p = wave; p < nv * nr; p += NWAVE) {
        const int v = p / nr, r = r0 + p % nr;          // wave-uniform
        const NetView n = net_view<I, O>(sv + v * PV, H);
        const float* xr = cm.x + (size_t)(cm.row0 + r) * cm.xs;     // the explained row: wave-uniform, not load_row's row per lane
        float x[I], bg[I];
#pragma unroll
        for (int i = 0; i < I; ++i) x[i] = xr[i];
        if (nch == 1) {                                 // a lane past the last background row computes the last and adds 0.0
            const float* br = a.bg + (size_t)min(lane, B - 1) * I;
#pragma unroll
            for (int i = 0; i < I; ++i) bg[i] = br[i];
        }
        double acc[NACC];
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
        for (int c = 0; c < C; ++c) {
            const unsigned long long mask = a.masks[c];
            double vs[O];
#pragma unroll
            for (int o = 0; o < O; ++o) vs[o] = 0.0;
            for (int ch = 0; ch < nch; ++ch) {
                const int b = ch * WAVE + lane;
                if (nch > 1) {
                    const float* br = a.bg + (size_t)min(b, B - 1) * I;
#pragma unroll
                    for (int i = 0; i < I; ++i) bg[i] = br[i];
                }
                float hx[I], f[O];
#pragma unroll
                for (int i = 0; i < I; ++i) hx[i] = ((mask >> i) & 1ull) ? x[i] : bg[i];
#pragma unroll
                for (int o = 0; o < O; ++o) f[o] = 0.0f;
                for (int h = 0; h < H; ++h) {
                    const float hid = sigmoid_sat(hidden_preact<I>(hx, n.W1, H, h) - n.B1[h]);      // Q1
#pragma unroll
                    for (int o = 0; o < O; ++o) f[o] = fmaf(hid, n.W2[h * O + o], f[o]);
                }
                output_head<TASK, O>(f, n.B2);
#pragma unroll
                for (int o = 0; o < O; ++o) vs[o] += wave_sum(b < B ? (double)f[o] : 0.0);
            }
#pragma unroll
            for (int o = 0; o < O; ++o) vs[o] = vs[o] / nb;
            // every lane holds the same v[o]; its accumulators take theirs by a select (a run-time index would go to memory)
#pragma unroll
            for (int k = 0; k < NACC; ++k) {
                if (WAVE * k < OT) {
                    double vq = vs[0];
#pragma unroll
                    for (int o = 1; o < O; ++o) vq = qo[k] == o ? vs[o] : vq;
                    acc[k] = fma(a.coef[(size_t)c * T + qt[k]], vq, acc[k]);
                }
            }
        }
        // column (r * O + o) * T + t = r * OT + q of the block, vector u0 + v
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            const int q = lane + WAVE * k;
            if (q < OT) a.fx[((size_t)r * OT + q) * cm.U + u0 + v] = (float)acc[k];
        }
    }
}
