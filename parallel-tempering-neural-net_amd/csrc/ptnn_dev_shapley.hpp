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
    const float* base;                  // vectors: d_pos_w rows or the uploaded host vectors
    const long long* run_off;           // [U] float offset of distinct vector u in base
    const float* x;                     // explained rows, x_0 .. x_{I-1} at x + row * xs
    int xs;                             // row stride of x (floats)
    int row0, nrows;                    // rows [row0, row0 + nrows) of x form this block of columns
    int H, P, PV;                       // hidden units, parameters, LDS stride of a staged vector (P rounded up to 4)
    int U, NV;                          // distinct vectors, vectors staged per work-group
    const float* bg;                    // [B][I] background rows
    int B, C, T;                        // background rows, coalitions, terms
    const unsigned long long* masks;    // [C] bit i set: input i from the explained row
    const double* coef;                 // [C][T]
    float* fx;                          // [nrows * O * T][U] column-major
};

// One wave per (distinct vector, explained row) pair, the lanes over the background rows in chunks of 64.  NV vectors staged in
// LDS, every weight read wave-uniform (an LDS broadcast); the explained row and the mask are uniform, the lane's background row
// sits in I registers, the hybrid input is a select.  A work-group takes NV vectors and SHAP_ROWS rows; wave w takes the pairs w,
// w + 4, ...  Per coalition and chunk: one pass over ALL hidden units in ascending order, the output sigmoids as pd_forward_kernel
// forms them, the O outputs summed over the lanes in double by the butterfly.  The T * O <= 256 accumulators are spread over the
// lanes: lane l owns q = l, l + 64, ... with q = o * T + t, and adds coef[c, t] * v[o] with one fma.
template <int TASK, int I, int O>
__global__ void __launch_bounds__(SHAP_THREADS) shapley_forward_kernel(const ShapFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NWAVE = SHAP_THREADS / WAVE, NACC = SHAP_MAX_ACC / WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NV = a.NV, PV = a.PV, H = a.H, B = a.B, C = a.C, T = a.T, OT = O * T;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, a.U - u0);
    const int r0 = blockIdx.y * SHAP_ROWS;
    const int nr = min(SHAP_ROWS, a.nrows - r0);
    float* sv = smem;                                   // [NV][PV] the staged vectors
    for (int v = 0; v < nv; ++v) {
        const float* src = a.base + a.run_off[u0 + v];
        for (int k = tid; k < a.P; k += SHAP_THREADS) sv[v * PV + k] = src[k];
    }
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
        const float* W1 = sv + v * PV;                  // [I][H]  (decode: w = W1, W2, B1, B2)
        const float* W2 = W1 + I * H;                   // [H][O]
        const float* B1 = W2 + H * O;
        const float* B2 = B1 + H;
        const float* xr = a.x + (size_t)(a.row0 + r) * a.xs;
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
                float hx[I], s[O];
#pragma unroll
                for (int i = 0; i < I; ++i) hx[i] = ((mask >> i) & 1ull) ? x[i] : bg[i];
#pragma unroll
                for (int o = 0; o < O; ++o) s[o] = 0.0f;
                for (int h = 0; h < H; ++h) {
                    float z = 0.0f;
#pragma unroll
                    for (int i = 0; i < I; ++i) z = fmaf(hx[i], W1[i * H + h], z);
                    z -= B1[h];                                                 // bias subtracted (Q1)
                    const float e = expf(-fabsf(z));                            // as sigmoid_and_slope forms it: e <= 1
                    const float hid = (z >= 0.0f ? 1.0f : e) / (1.0f + e);
#pragma unroll
                    for (int o = 0; o < O; ++o) s[o] = fmaf(hid, W2[h * O + o], s[o]);
                }
                // the output sigmoid (Q2); classification: p = softmax(s) (CLS:108-110)
                float f[O];
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    const float zo = s[o] - B2[o];
                    const float e = expf(-fabsf(zo));
                    f[o] = (zo >= 0.0f ? 1.0f : e) / (1.0f + e);
                }
                if (TASK == TASK_CLS) {
                    float sum = 0.0f;
#pragma unroll
                    for (int o = 0; o < O; ++o) { f[o] = expf(f[o]); sum += f[o]; }
#pragma unroll
                    for (int o = 0; o < O; ++o) f[o] = f[o] / sum;
                }
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
            if (q < OT) a.fx[((size_t)r * OT + q) * a.U + u0 + v] = (float)acc[k];
        }
    }
}
