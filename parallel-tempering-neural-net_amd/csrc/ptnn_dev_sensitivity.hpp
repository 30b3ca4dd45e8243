// ptnn_dev_sensitivity.hpp -- part of ptnn_analysis_device.hpp (textually included there, inside namespace ptnn; not a stand-alone header):
// input sensitivity of the sampled nets (ptnn_sensitivity, include/ptnn.h) -- the Jacobian of the network
// output with respect to the inputs, per distinct weight vector and data row.  Nothing of the kind is in the reference.
//
//   z_h = sum_i x_i W1[i,h] - B1[h]     hid_h = sigmoid(z_h)     d_h  = hid_h (1 - hid_h)
//   a_o = sum_h hid_h W2[h,o] - B2[o]   s_o   = sigmoid(a_o)     ds_o = s_o (1 - s_o)
//   J[o,i] = ds_o sum_h W2[h,o] d_h W1[i,h]                      regression: g = J
//   classification (p = softmax(s), CLS:108-110):                g[c,i] = p_c (J[c,i] - sum_o p_o J[o,i])
//
// The three stages of ptnn_dev_predict.hpp, with another stage b:
//   b. sensitivity_forward_kernel<TASK, I, O> (per shape, AnalysisShape::sens_fwd): gx[col][u] = g of distinct vector u, column
//      col = (row * O + o) * I + i of a block of input rows -- the layout of PredictFwd::fx, so stage c (predict_reduce_kernel) takes
//      the gradient columns as it takes the outputs.
//   then per block of rows sensitivity_sign_kernel (the weighted counts of g > 0 and g < 0 per column) and
//   sensitivity_rows_kernel (|g| and g^2 summed over the rows, per vector and (o, i), in double, carried across the blocks), and
//   at the end sensitivity_mean_kernel (the weighted means of those sums over the vectors).
// Nothing here writes chain state, tapes, counters or trace rows.
//
// This file holds the constants, SensFwd and stage b, which ptnn_analysis_shape.hip instantiates per shape; the shape-independent
// kernels are ptnn_dev_sensitivity_reduce.hpp, which ptnn_analysis.hip alone includes.
constexpr int SENS_THREADS = 256;        // 4 waves
constexpr int SENS_MAX_NV = 16;          // distinct vectors per forward work-group
constexpr int SENS_ACC = 40;             // gradient accumulators a lane holds in one pass over the hidden units

// The inputs are tiled: one pass over the hidden units carries S[o][i] for all O outputs and a chunk of IT inputs, at most SENS_ACC
// accumulators (pendigit's 16 x 10 = 160 at once would leave a SIMD one wave).  NT passes, balanced: 34 x 2 -> 2 x 17,
// 16 x 10 -> 4 x 4, 11 x 10 -> 4 + 4 + 3, 6 x 18 -> 3 x 2; every other compiled shape takes one pass.
template <int I, int O> struct SensTile {
    static constexpr int FIT = SENS_ACC / O < 1 ? 1 : (SENS_ACC / O < I ? SENS_ACC / O : I);
    static constexpr int NT = (I + FIT - 1) / FIT;
    static constexpr int IT = (I + NT - 1) / NT;
};

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: SensPlan)
struct SensFwd {
    FwdCommon c;
    int VS;                     // LDS stride of a vector's finished tile: O * I * 64 + a pad that spreads the vectors over the banks
    float* gx;                  // [nrows * O * I][U] column-major
};

// One lane per input row with the row's inputs in registers, NV vectors staged in LDS, every weight read wave-uniform (an LDS
// broadcast): the pieces of ptnn_dev_net.hpp.  The work of a group is the nv x NT (vector, input tile) pairs; wave w takes the pairs
// w, w + 4, ...  A pair is one pass over ALL hidden units in ascending order -- z_h and a_o are recomputed per tile, the sums are
// never split across waves -- so a value does not depend on NV, on the block of rows or on which wave computed it.
template <int TASK, int I, int O>
__global__ void __launch_bounds__(SENS_THREADS) sensitivity_forward_kernel(const SensFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int IT = SensTile<I, O>::IT, NT = SensTile<I, O>::NT, NWAVE = SENS_THREADS / WAVE, OI = O * I;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FwdCommon& cm = a.c;
    const int NV = cm.NV, PV = cm.PV, H = cm.H, VS = a.VS;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, cm.U - u0);
    const int r0 = blockIdx.y * WAVE;
    float* sv = smem;                                   // [NV][PV] the staged vectors
    float* fin = sv + (size_t)NV * PV;                  // [NV][VS] finished gradients: fin[v * VS + (o * I + i) * 64 + lane]
    stage_vectors<SENS_THREADS>(sv, cm, u0, nv, tid);
    float x[I];
    load_row<I>(cm, r0 + lane, x);
    __syncthreads();
    for (int p = wave; p < nv * NT; p += NWAVE) {
        const int v = p / NT, i0 = (p % NT) * IT;      // wave-uniform
        const NetView n = net_view<I, O>(sv + v * PV, H);
        const float *W1 = n.W1, *W2 = n.W2;
        int w1row[IT];                                  // W1 rows of this tile; past the last input (11 = 4 + 4 + 3): the last row again, not stored
#pragma unroll
        for (int k = 0; k < IT; ++k) w1row[k] = min(i0 + k, I - 1) * H;
        float S[O][IT], acc[O];
#pragma unroll
        for (int o = 0; o < O; ++o) {
            acc[o] = 0.0f;
#pragma unroll
            for (int k = 0; k < IT; ++k) S[o][k] = 0.0f;
        }
        for (int h = 0; h < H; ++h) {
            float hid, d;
            sigmoid_and_slope(hidden_preact<I>(x, W1, H, h) - n.B1[h], &hid, &d);       // Q1
            float dw[IT];
#pragma unroll
            for (int k = 0; k < IT; ++k) dw[k] = d * W1[w1row[k] + h];
#pragma unroll
            for (int o = 0; o < O; ++o) {
                const float w2 = W2[h * O + o];
                acc[o] = fmaf(hid, w2, acc[o]);
#pragma unroll
                for (int k = 0; k < IT; ++k) S[o][k] = fmaf(w2, dw[k], S[o][k]);
            }
        }
        // the output sigmoid (Q2) and its slope, the softmax
        float ds[O], pc[O];
#pragma unroll
        for (int o = 0; o < O; ++o) sigmoid_and_slope(acc[o] - n.B2[o], &pc[o], &ds[o]);
        softmax_head<TASK, O>(pc);
        float* out = fin + (size_t)v * VS + lane;
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            float J[O], m = 0.0f;
#pragma unroll
            for (int o = 0; o < O; ++o) {
                J[o] = ds[o] * S[o][k];
                m = fmaf(pc[o], J[o], m);
            }
            if (i0 + k < I) {
#pragma unroll
                for (int o = 0; o < O; ++o) out[(o * I + i0 + k) * WAVE] = TASK == TASK_CLS ? pc[o] * (J[o] - m) : J[o];
            }
        }
    }
    __syncthreads();
    // column-major store: column (r0 + l) * O * I + oi of the block gets NV consecutive floats
    for (int idx = tid; idx < OI * WAVE * NV; idx += SENS_THREADS) {
        const int v = idx % NV, c = idx / NV, l = c % WAVE, oi = c / WAVE;
        if (v < nv && r0 + l < cm.nrows) a.gx[((size_t)(r0 + l) * OI + oi) * cm.U + u0 + v] = fin[(size_t)v * VS + oi * WAVE + l];
    }
}
