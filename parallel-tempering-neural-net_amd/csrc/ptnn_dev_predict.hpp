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

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: ForwardPlan)
struct PredictFwd {
    FwdCommon c;
    float* fx;                  // [nrows * O][U] column-major
};

template <int TASK, int I, int O>
__global__ void __launch_bounds__(PRED_THREADS) predict_forward_kernel(const PredictFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NWAVE = PRED_THREADS / WAVE;
    const FwdCommon& cm = a.c;
    const int NV = cm.NV, PV = cm.PV, H = cm.H;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, cm.U - u0);
    const int r0 = blockIdx.y * WAVE;
    float* sv = smem;                                   // [NV][PV] the staged vectors
    float* red = sv + (size_t)NV * PV;                  // [NWAVE][NV][O][64] partial output sums, one per wave's hidden slice
    float* fin = red + (size_t)NWAVE * NV * O * WAVE;   // [64 * O][NV] finished outputs, the tile transposed for the store
    stage_vectors<PRED_THREADS>(sv, cm, u0, nv, tid);
    float x[I];
    load_row<I>(cm, r0 + lane, x);
    __syncthreads();
    // wave `wave` takes the hidden units h = wave, wave + 4, ...: every weight read is wave-uniform (an LDS broadcast)
    for (int v = 0; v < nv; ++v) {
        const NetView n = net_view<I, O>(sv + v * PV, H);
        float acc[O];
#pragma unroll
        for (int o = 0; o < O; ++o) acc[o] = 0.0f;
        for (int h = wave; h < H; h += NWAVE) {
            const float hid = sigmoid_plain(hidden_preact<I>(x, n.W1, H, h) - n.B1[h]);      // Q1
#pragma unroll
            for (int o = 0; o < O; ++o) acc[o] = fmaf(hid, n.W2[h * O + o], acc[o]);
        }
#pragma unroll
        for (int o = 0; o < O; ++o) red[(((size_t)wave * NV + v) * O + o) * WAVE + lane] = acc[o];
    }
    __syncthreads();
    // the four partial sums in a fixed order, the plain output sigmoid (Q2), the softmax
    for (int idx = tid; idx < nv * WAVE; idx += PRED_THREADS) {
        const int v = idx / WAVE, l = idx % WAVE;
        const float* B2 = net_view<I, O>(sv + v * PV, H).B2;
        float out[O];
#pragma unroll
        for (int o = 0; o < O; ++o) {
            float s = red[(((size_t)0 * NV + v) * O + o) * WAVE + l];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) s += red[(((size_t)w * NV + v) * O + o) * WAVE + l];
            out[o] = sigmoid_plain(s - B2[o]);
        }
        softmax_head<TASK, O>(out);
#pragma unroll
        for (int o = 0; o < O; ++o) fin[(size_t)(l * O + o) * NV + v] = out[o];
    }
    __syncthreads();
    // column-major store: column r0 * O + c of the block gets NV consecutive floats
    for (int idx = tid; idx < WAVE * O * NV; idx += PRED_THREADS) {
        const int c = idx / NV, v = idx % NV;
        if (v < nv && r0 + c / O < cm.nrows) a.fx[(size_t)(r0 * O + c) * cm.U + u0 + v] = fin[idx];
    }
}
