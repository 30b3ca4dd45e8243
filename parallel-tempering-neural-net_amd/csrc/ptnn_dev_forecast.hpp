// ptnn_dev_forecast.hpp -- recursive multi-step forecasts of a one-step regression map (ptnn_forecast, include/ptnn.h;
// DESIGN.md section 14).  A trained REG net with n_out == 1 is the map x[t+1] = f_w(x[t-I+1 .. t]); step k = 1 .. h of a
// trajectory is y_k = f_w(window_{k-1}) (+ exp(eta / 2) z_k with noise on), window_k = (window_{k-1}[1:], y_k).
//   a. the selection: noise off -- sample_runs_kernel + predict_scan_kernel (distinct vectors with multiplicities, one
//      trajectory each); noise on -- sample_runs_kernel with the eta (every occurrence its own trajectory).  Both unchanged.
//   b. forecast_forward_kernel<TASK, I, O> (per shape, AnalysisShape::forecast_fwd): fx[col][u] = y of trajectory u at column
//      col = origin * hb + k of a block of origins and horizon steps; the windows are carried from one horizon block to the next.
//      With ForecastFwd::mu (ptnn_forecast_score) it also stores the output before the step's noise.
//   c. predict_reduce_kernel, unchanged.
// The forward pass is ptnn_predict's, operation for operation (the pieces of ptnn_dev_net.hpp where a line is the same operation;
// the lane layout's transposed vectors have a decode and a pre-activation of their own): four partial sums over h = wave (mod 4),
// each accumulated in ascending h, combined in the order 0, 1, 2, 3, then the output sigmoid -- so step 1 is bit-identical to ptnn_predict on the
// origin rows, whichever layout runs it.  Nothing here writes chain state, tapes, counters or trace rows.

constexpr int FC_THREADS = 256;          // 4 waves
enum { FC_LANE = 0, FC_SPLIT = 1 };      // layouts: one trajectory per lane / one vector per work-group, hidden units over waves
constexpr int FC_LANE_MAX_P = 96;        // the lane layout holds 4 waves x 64 vectors transposed: 4 * 96 * 64 * 4 B = 96 KiB

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: ptnn_forecast)
struct ForecastFwd {
    const float* base;          // vectors: d_pos_w rows or the uploaded host vectors
    const long long* run_off;   // [U] float offset of trajectory u's vector in base
    const float* eta;           // [U] eta of trajectory u (noise on), else null
    const float* x;             // origin windows, x_0 .. x_{I-1} at x + origin * xs
    int xs;                     // row stride of x (floats)
    int r0, nr;                 // origins [r0, r0 + nr) form this block
    int k0, hb, horizon;        // horizon steps [k0, k0 + hb) of `horizon`
    float* win;                 // [nr][U][I] windows carried between horizon blocks (null: one horizon block)
    int H, P, U;                // hidden units, parameters, trajectories
    int layout;                 // FC_LANE / FC_SPLIT
    int noise;
    uint32_t seed_lo, seed_hi;
    float* fx;                  // [nr * hb][U] column-major, column (r - r0) * hb + (k - k0)
    float* mu;                  // [nr * hb][U] as fx: the sigmoid output before the step's noise is added (ptnn_forecast_score), or null
};

// z_k of trajectory i at origin r: normals(k + 1, i, r, STREAM_FORECAST, seed)[k] of philox.py
__device__ __forceinline__ void forecast_normals(int k, int i, int r, uint32_t slo, uint32_t shi, float (&z)[4]) {
    uint32_t q[4];
    philox4x32_10((uint32_t)(k >> 2), (uint32_t)i, (uint32_t)r, STREAM_FORECAST, slo, shi, q);
    box_muller(q[0], q[1], z[0], z[1]);
    box_muller(q[2], q[3], z[2], z[3]);
}

__device__ __forceinline__ float forecast_pick(const float (&z)[4], int k) {     // z[k & 3] without a dynamic register index
    const int c = k & 3;
    return c == 0 ? z[0] : c == 1 ? z[1] : c == 2 ? z[2] : z[3];
}

template <int TASK, int I, int O>
__global__ void __launch_bounds__(FC_THREADS) forecast_forward_kernel(const ForecastFwd a) {
    if constexpr (TASK == TASK_REG && O == 1) {
        extern __shared__ __attribute__((aligned(16))) float smem[];
        const int tid = threadIdx.x, lane = tid & (WAVE - 1);
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        constexpr int NWAVE = FC_THREADS / WAVE;
        const int H = a.H, P = a.P, U = a.U;
        const bool carry = a.win != nullptr && a.k0 + a.hb < a.horizon;
        if (a.layout == FC_LANE) {
            // one trajectory per lane; the wave's 64 vectors staged transposed, sv[p][lane]: every weight read is conflict-free
            float* sv = smem + (size_t)wave * P * WAVE;
            const int ub = (blockIdx.x * NWAVE + wave) * WAVE;
            const int u = ub + lane;
            const bool live_u = u < U;
            for (int k = lane; k < P * WAVE; k += WAVE) {
                const int v = k / P, p = k - v * P;
                const float* src = a.base + a.run_off[min(ub + v, U - 1)];
                sv[p * WAVE + v] = src[p];
            }
            __syncthreads();
            const float* W1 = sv;                                // [I][H]  (decode: w = W1, W2, B1, B2)
            const float* W2 = W1 + I * H * WAVE;                 // [H]
            const float* B1 = W2 + H * WAVE;
            const float B2 = B1[H * WAVE + lane];
            const float sd = a.noise && live_u ? expf(0.5f * a.eta[u]) : 0.0f;
            // origins r0 + blockIdx.y, + gridDim.y, ...: the staged vectors serve every origin of the work-group
            for (int rl = blockIdx.y; rl < a.nr; rl += gridDim.y) {
                const int r = a.r0 + rl;
                float x[I];
                if (a.k0 == 0) {
                    const float* xr = a.x + (size_t)r * a.xs;
#pragma unroll
                    for (int i = 0; i < I; ++i) x[i] = xr[i];
                } else {
                    const float* wr = a.win + ((size_t)rl * U + (live_u ? u : 0)) * I;
#pragma unroll
                    for (int i = 0; i < I; ++i) x[i] = wr[i];
                }
                float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int k = a.k0; k < a.k0 + a.hb; ++k) {
                    float acc[NWAVE];
#pragma unroll
                    for (int w = 0; w < NWAVE; ++w) acc[w] = 0.0f;
                    for (int hb = 0; hb < H; hb += NWAVE) {
#pragma unroll
                        for (int w = 0; w < NWAVE; ++w) {
                            const int h = hb + w;
                            if (h < H) {
                                float zz = 0.0f;
#pragma unroll
                                for (int i = 0; i < I; ++i) zz = fmaf(x[i], W1[(i * H + h) * WAVE + lane], zz);
                                const float hid = sigmoid_plain(zz - B1[h * WAVE + lane]);      // Q1
                                acc[w] = fmaf(hid, W2[h * WAVE + lane], acc[w]);
                            }
                        }
                    }
                    float s = acc[0];
#pragma unroll
                    for (int w = 1; w < NWAVE; ++w) s += acc[w];
                    float y = sigmoid_plain(s - B2);                                  // Q2
                    if (a.mu && live_u) a.mu[((size_t)rl * a.hb + (k - a.k0)) * U + u] = y;
                    if (a.noise) {
                        if (k == a.k0 || (k & 3) == 0) forecast_normals(k, u, r, a.seed_lo, a.seed_hi, z);
                        y = y + sd * forecast_pick(z, k);
                    }
                    if (live_u) a.fx[((size_t)rl * a.hb + (k - a.k0)) * U + u] = y;
#pragma unroll
                    for (int i = 0; i + 1 < I; ++i) x[i] = x[i + 1];
                    x[I - 1] = y;
                }
                if (carry && live_u) {
                    float* wr = a.win + ((size_t)rl * U + u) * I;
#pragma unroll
                    for (int i = 0; i < I; ++i) wr[i] = x[i];
                }
            }
        } else {
            // one vector per work-group, one origin per lane, wave `wave` takes the hidden units h = wave, wave + 4, ... (the
            // predict_forward_kernel pattern); the partial sums meet in LDS (double-buffered: one barrier per step), and every
            // wave combines them alike, so each holds the new value without a second broadcast
            const int u = blockIdx.x;
            float* sv = smem;                                    // [P] the staged vector
            float* red = sv + ((P + 3) & ~3);                    // [2][NWAVE][64]
            const float* src = a.base + a.run_off[u];
            for (int k = tid; k < P; k += FC_THREADS) sv[k] = src[k];
            const int rl = blockIdx.y * WAVE + lane;
            const bool live = rl < a.nr;
            const int rc = live ? rl : 0;
            const int r = a.r0 + rc;
            float x[I];
            if (a.k0 == 0) {
                const float* xr = a.x + (size_t)r * a.xs;
#pragma unroll
                for (int i = 0; i < I; ++i) x[i] = xr[i];
            } else {
                const float* wr = a.win + ((size_t)rc * U + u) * I;
#pragma unroll
                for (int i = 0; i < I; ++i) x[i] = wr[i];
            }
            __syncthreads();
            const NetView n = net_view<I, O>(sv, H);
            const float B2 = n.B2[0];
            const float sd = a.noise ? expf(0.5f * a.eta[u]) : 0.0f;
            float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int buf = 0;
            for (int k = a.k0; k < a.k0 + a.hb; ++k) {
                float acc = 0.0f;
                for (int h = wave; h < H; h += NWAVE) {
                    const float hid = sigmoid_plain(hidden_preact<I>(x, n.W1, H, h) - n.B1[h]);
                    acc = fmaf(hid, n.W2[h], acc);
                }
                red[(buf * NWAVE + wave) * WAVE + lane] = acc;
                __syncthreads();
                float s = red[(buf * NWAVE + 0) * WAVE + lane];
#pragma unroll
                for (int w = 1; w < NWAVE; ++w) s += red[(buf * NWAVE + w) * WAVE + lane];
                buf ^= 1;
                float y = sigmoid_plain(s - B2);
                if (a.mu && wave == 0 && live) a.mu[((size_t)rl * a.hb + (k - a.k0)) * U + u] = y;
                if (a.noise) {
                    if (k == a.k0 || (k & 3) == 0) forecast_normals(k, u, r, a.seed_lo, a.seed_hi, z);
                    y = y + sd * forecast_pick(z, k);
                }
                if (wave == 0 && live) a.fx[((size_t)rl * a.hb + (k - a.k0)) * U + u] = y;
#pragma unroll
                for (int i = 0; i + 1 < I; ++i) x[i] = x[i + 1];
                x[I - 1] = y;
            }
            if (carry && wave == 0 && live) {
                float* wr = a.win + ((size_t)rl * U + u) * I;
#pragma unroll
                for (int i = 0; i < I; ++i) wr[i] = x[i];
            }
        }
    }
}
