// ptnn_dev_pd.hpp -- part of ptnn_analysis_device.hpp (textually included there, inside namespace ptnn; not a stand-alone header):
// partial dependence and individual conditional expectation curves of the sampled nets (ptnn_partial_dependence, include/ptnn.h;
// DESIGN.md section 25; Friedman 2001, Goldstein et al. 2015).  Nothing of the kind is in the reference.
//
//   ICE_s[n, a, k, o] = f_o(w_s; x_n with x_n[j] := v)      j = inputs[a], v = grid[a, k], f as ptnn_predict returns it
//   z_h  = sum_i x_i W1[i,h] - B1[h]                         the row as it is, once per hidden unit
//   zk_h = z_h + (v - x_j) W1[j,h]                           the substituted row is never rebuilt: one FMA per grid value
//   hid  = sigmoid(zk_h)   a_o = sum_h hid W2[h,o] - B2[o]   s_o = sigmoid(a_o)   classification: p = softmax(s) (CLS:108-110)
//
// The three stages of ptnn_dev_predict.hpp, with another stage b:
//   b. pd_forward_kernel<TASK, I, O> (per shape, AnalysisShape::pd_fwd): fx[col][u] = ICE of distinct vector u, column
//      col = ((row * A + a) * G + k) * O + o of a block of input rows -- the layout of PredictFwd::fx, so stage c
//      (predict_reduce_kernel, with O = 1 and no votes) takes the ICE columns as it takes the outputs.
//   then per block of rows pd_rows_kernel (ICE summed over the rows per vector and (a, k, o), in double, carried across the blocks;
//   after the last block PD32 = the row mean as fp32), and at the end pd_range_kernel (max_k - min_k of PD32 per vector and (a, o))
//   and pd_mean_kernel (the weighted means of the double row means over the vectors).
// Nothing here writes chain state, tapes, counters or trace rows, and nothing here uses an atomic.
//
// The invariant: a value of stage b is a function of (vector, row, input, grid value) alone.  It is one whole pass over the hidden
// units in ascending order into accumulators of its own, so it does not depend on NV, on how the grid is cut into chunks, on the
// tile slot the value falls in, on the block of rows or on the wave that computed it.
//
// This file holds the constants, PdFwd and stage b, which ptnn_analysis_shape.hip instantiates per shape; the shape-independent
// kernels are ptnn_dev_pd_reduce.hpp, which ptnn_analysis.hip alone includes.
constexpr int PD_THREADS = 256;          // 4 waves
constexpr int PD_MAX_NV = 16;            // distinct vectors per forward work-group
constexpr int PD_MAX_GRID = 64;          // grid values per input (PTNN_PD_MAX_GRID)
constexpr int PD_ACC = 40;               // output accumulators a lane holds in one pass over the hidden units
constexpr int PD_MAX_GT = 16;

// The grid values are tiled: one pass over the hidden units carries acc[o][k] for all O outputs and GT grid values, at most PD_ACC
// accumulators: O = 1, 2 -> 16, O = 3 -> 13, O = 10 -> 4, O = 18 -> 2.  The host plans with the same function.
constexpr int pd_grid_tile(int O) { return PD_ACC / O < 1 ? 1 : (PD_ACC / O < PD_MAX_GT ? PD_ACC / O : PD_MAX_GT); }

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: PdPlan)
struct PdFwd {
    FwdCommon c;
    int VS;                     // LDS stride of a vector's finished tile: GC * O * 64 + a pad that spreads the vectors over the banks
    int A, G;                   // selected inputs, grid values per input
    int GC, NCH;                // grid values per chunk, chunks per input: blockIdx.z = a * NCH + chunk
    const int* inputs;          // [A] input index j of slot a, in [0, I)
    const float* grid;          // [A][G]
    float* fx;                  // [nrows * A * G * O][U] column-major
};

// One lane per input row with the row's inputs in registers, NV vectors staged in LDS, every weight read wave-uniform (an LDS
// broadcast): the pieces of ptnn_dev_net.hpp.  A work-group takes 64 rows, NV vectors and one chunk: a selected input with a run
// of its grid values.  Its work is the nv x nt (vector, grid tile) pairs; wave w takes the pairs w, w + 4, ...  A pair is one pass
// over ALL hidden units in ascending order: z_h from the row as it is (I FMAs), then per grid value of the tile one FMA, one
// sigmoid and O FMAs.  A tile slot past the chunk's last grid value recomputes that value and stores nothing.
template <int TASK, int I, int O>
__global__ void __launch_bounds__(PD_THREADS) pd_forward_kernel(const PdFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int GT = pd_grid_tile(O), NWAVE = PD_THREADS / WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FwdCommon& cm = a.c;
    const int NV = cm.NV, PV = cm.PV, H = cm.H, VS = a.VS, G = a.G;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, cm.U - u0);
    const int r0 = blockIdx.y * WAVE;
    const int ai = blockIdx.z / a.NCH, k0 = (blockIdx.z % a.NCH) * a.GC;
    const int kc = min(a.GC, G - k0);                   // grid values of this chunk, >= 1
    const int nt = (kc + GT - 1) / GT;
    const int j = a.inputs[ai];
    const float* gv = a.grid + (size_t)ai * G + k0;
    float* sv = smem;                                   // [NV][PV] the staged vectors
    float* fin = sv + (size_t)NV * PV;                  // [NV][VS] finished values: fin[v * VS + (kk * O + o) * 64 + lane]
    stage_vectors<PD_THREADS>(sv, cm, u0, nv, tid);
    float x[I];
    const float xj = load_row<I>(cm, r0 + lane, x).xr[j];
    __syncthreads();
    for (int p = wave; p < nv * nt; p += NWAVE) {
        const int v = p / nt, t0 = (p % nt) * GT;       // wave-uniform
        const NetView n = net_view<I, O>(sv + v * PV, H);
        const float* W1j = n.W1 + j * H;
        float dv[GT], acc[O][GT];
#pragma unroll
        for (int k = 0; k < GT; ++k) {
            dv[k] = gv[min(t0 + k, kc - 1)] - xj;
#pragma unroll
            for (int o = 0; o < O; ++o) acc[o][k] = 0.0f;
        }
        for (int h = 0; h < H; ++h) {
            const float z = hidden_preact<I>(x, n.W1, H, h) - n.B1[h];      // Q1
            const float w1j = W1j[h];
            float w2[O];
#pragma unroll
            for (int o = 0; o < O; ++o) w2[o] = n.W2[h * O + o];
#pragma unroll
            for (int k = 0; k < GT; ++k) {
                const float hid = sigmoid_sat(fmaf(dv[k], w1j, z));
#pragma unroll
                for (int o = 0; o < O; ++o) acc[o][k] = fmaf(hid, w2[o], acc[o][k]);
            }
        }
        float* out = fin + (size_t)v * VS + lane;
#pragma unroll
        for (int k = 0; k < GT; ++k) {
            float f[O];
#pragma unroll
            for (int o = 0; o < O; ++o) f[o] = acc[o][k];
            output_head<TASK, O>(f, n.B2);
            if (t0 + k < kc) {
#pragma unroll
                for (int o = 0; o < O; ++o) out[((t0 + k) * O + o) * WAVE] = f[o];
            }
        }
    }
    __syncthreads();
    // column-major store: column ((r0 + l) * A + ai) * G * O + k0 * O + ko of the block gets NV consecutive floats
    const size_t GO = (size_t)G * O;
    for (int idx = tid; idx < kc * O * WAVE * NV; idx += PD_THREADS) {
        const int v = idx % NV, c = idx / NV, l = c % WAVE, ko = c / WAVE;
        if (v < nv && r0 + l < cm.nrows)
            a.fx[((((size_t)(r0 + l) * a.A + ai) * GO) + (size_t)k0 * O + ko) * cm.U + u0 + v] = fin[(size_t)v * VS + ko * WAVE + l];
    }
}
