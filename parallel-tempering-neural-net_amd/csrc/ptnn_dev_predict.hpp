// ptnn_dev_predict.hpp -- part of ptnn_analysis_device.hpp (textually included there, inside namespace ptnn; not a stand-alone header):
// posterior predictive over sampled weight vectors (ptnn_predict, include/ptnn.h).
//
// The reference's drafts take the network outputs of every post-burn-in sample on the train and test rows and reduce them to
// a mean and 5 / 95 % percentile bands (multicore-pt-classification/Misc_code/ldpt_classifier_multi.py:788-794); its
// run_chains() stopped producing those outputs "to save memory" (REG:244-245, 410-419, 785-837).  Three stages:
//   a. sample_runs_kernel + predict_scan_kernel (ptnn_dev_select.hpp): the selected rows (trace rows of a list of chains, or uploaded vectors) are
//      collapsed into DISTINCT vectors with integer multiplicities -- a rejected MH step repeats the previous vector (REG:417),
//      so most selected rows repeat the one before; the output depends on w only, so one evaluation per run is exact.
//   b. predict_forward_kernel<TASK, I, O> (per shape, AnalysisShape::predict_fwd): fx[col][u] = ForwardPass of distinct vector u on
//      output column col = row * O + o of a block of input rows (REG:51-55 / CLS:49-55; CLS: softmax of it, CLS:108-110).
//   c. predict_reduce_kernel (ptnn_dev_select.hpp): one work-group per column -- weighted mean (double), exact weighted order statistics (radix select
//      on the order-preserving key of the fp32 value), and for classification the class-vote counts.
// Nothing here writes chain state, tapes, counters or trace rows.  This file holds the constants, PredictFwd and stage b, which
// ptnn_analysis_shape.hip instantiates per shape.

constexpr int PRED_THREADS = 256;        // forward and reduce kernels: 4 waves
constexpr int PRED_SCAN_THREADS = 1024;  // the scan: one work-group
constexpr int PRED_MAX_RANKS = 16;
constexpr int PRED_MAX_NV = 16;          // distinct vectors per forward work-group

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: ptnn_predict)
struct PredictFwd {
    const float* base;          // vectors: d_pos_w rows or the uploaded host vectors
    const long long* run_off;   // [U] float offset of distinct vector u in base
    const float* x;             // input rows, x_0 .. x_{I-1} at x + row * xs
    int xs;                     // row stride of x (floats)
    int row0, nrows;            // rows [row0, row0 + nrows) of x form this block of columns
    int H, P, PV;               // hidden units, parameters, LDS stride of a staged vector (P rounded up to 4)
    int U, NV;                  // distinct vectors, vectors staged per work-group
    float* fx;                  // [nrows * O][U] column-major
};

template <int TASK, int I, int O>
__global__ void __launch_bounds__(PRED_THREADS) predict_forward_kernel(const PredictFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NWAVE = PRED_THREADS / WAVE;
    const int NV = a.NV, PV = a.PV, H = a.H;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, a.U - u0);
    const int r0 = blockIdx.y * WAVE;
    float* sv = smem;                                   // [NV][PV] the staged vectors
    float* red = sv + (size_t)NV * PV;                  // [NWAVE][NV][O][64] partial output sums, one per wave's hidden slice
    float* fin = red + (size_t)NWAVE * NV * O * WAVE;   // [64 * O][NV] finished outputs, the tile transposed for the store
    for (int v = 0; v < nv; ++v) {
        const float* src = a.base + a.run_off[u0 + v];
        for (int k = tid; k < a.P; k += PRED_THREADS) sv[v * PV + k] = src[k];
    }
    // one lane per input row, the row's inputs in registers (a lane past the last row computes row 0 and stores nothing)
    const int row = r0 + lane;
    const bool live = row < a.nrows;
    const float* xr = a.x + (size_t)(a.row0 + (live ? row : 0)) * a.xs;
    float x[I];
#pragma unroll
    for (int i = 0; i < I; ++i) x[i] = xr[i];
    __syncthreads();
    // wave `wave` takes the hidden units h = wave, wave + 4, ...: every weight read is wave-uniform (an LDS broadcast)
    for (int v = 0; v < nv; ++v) {
        const float* W1 = sv + v * PV;                  // [I][H]  (decode: w = W1, W2, B1, B2)
        const float* W2 = W1 + I * H;                   // [H][O]
        const float* B1 = W2 + H * O;
        float acc[O];
#pragma unroll
        for (int o = 0; o < O; ++o) acc[o] = 0.0f;
        for (int h = wave; h < H; h += NWAVE) {
            float z = 0.0f;
#pragma unroll
            for (int i = 0; i < I; ++i) z = fmaf(x[i], W1[i * H + h], z);
            const float hid = 1.0f / (1.0f + expf(-(z - B1[h])));        // bias subtracted (Q1)
#pragma unroll
            for (int o = 0; o < O; ++o) acc[o] = fmaf(hid, W2[h * O + o], acc[o]);
        }
#pragma unroll
        for (int o = 0; o < O; ++o) red[(((size_t)wave * NV + v) * O + o) * WAVE + lane] = acc[o];
    }
    __syncthreads();
    // the four partial sums in a fixed order, the output sigmoid (Q2), classification: softmax (CLS:108-110)
    for (int idx = tid; idx < nv * WAVE; idx += PRED_THREADS) {
        const int v = idx / WAVE, l = idx % WAVE;
        const float* B2 = sv + v * PV + I * a.H + a.H * O + a.H;
        float out[O];
#pragma unroll
        for (int o = 0; o < O; ++o) {
            float s = red[(((size_t)0 * NV + v) * O + o) * WAVE + l];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) s += red[(((size_t)w * NV + v) * O + o) * WAVE + l];
            out[o] = 1.0f / (1.0f + expf(-(s - B2[o])));
        }
        if (TASK == TASK_CLS) {
            float e[O], sum = 0.0f;
#pragma unroll
            for (int o = 0; o < O; ++o) { e[o] = expf(out[o]); sum += e[o]; }
#pragma unroll
            for (int o = 0; o < O; ++o) out[o] = e[o] / sum;
        }
#pragma unroll
        for (int o = 0; o < O; ++o) fin[(size_t)(l * O + o) * NV + v] = out[o];
    }
    __syncthreads();
    // column-major store: column r0 * O + c of the block gets NV consecutive floats
    for (int idx = tid; idx < WAVE * O * NV; idx += PRED_THREADS) {
        const int c = idx / NV, v = idx % NV;
        if (v < nv && r0 + c / O < a.nrows) a.fx[(size_t)(r0 * O + c) * a.U + u0 + v] = fin[idx];
    }
}
