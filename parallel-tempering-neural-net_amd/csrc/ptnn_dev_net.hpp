// ptnn_dev_net.hpp -- part of ptnn_analysis_device.hpp (textually included there, inside namespace ptnn; not a stand-alone header,
// and never a part of ptnn_device.hpp: the sampler's code objects see none of it): the ONE statement of the network for the
// per-shape analysis forward kernels (predict, forecast, sensitivity, pd, shapley, ale).  Each piece is the operations its callers
// wrote out by hand before, in the same order; the reference's quirks live here and nowhere else among those kernels:
//   Q1  the hidden bias is SUBTRACTED: z_h = sum_i x_i W1[i,h] - B1[h]    (REG:51-55 / CLS:49-55; the caller subtracts B1[h])
//   Q2  so is the output bias:          a_o = sum_h hid_h W2[h,o] - B2[o]
//   classification returns softmax(sigmoid(a)), not softmax(a)            (CLS:108-110)
// What is a kernel's own stays in the kernel: how the hidden units, inputs, grid values or slots are tiled over waves and passes,
// the accumulators and the `fin` layouts.

// The arguments every staged-vector forward kernel takes: the first member of PredictFwd, SensFwd, PdFwd, ShapFwd and AleFwd (56
// bytes, a multiple of 8, so the members after it sit where they sat when each struct listed these fields itself).  The host fills
// it in one place (ptnn_analysis.hip: StagedPlan::common).
struct FwdCommon {
    const float* base;          // vectors: d_pos_w rows or the uploaded host vectors
    const long long* run_off;   // [U] float offset of distinct vector u in base
    const float* x;             // input rows, x_0 .. x_{I-1} at x + row * xs
    int xs;                     // row stride of x (floats)
    int row0, nrows;            // rows [row0, row0 + nrows) of x form this block of columns
    int H, P, PV;               // hidden units, parameters, LDS stride of a staged vector (P rounded up to 4)
    int U, NV;                  // distinct vectors, vectors staged per work-group
};
static_assert(sizeof(FwdCommon) == 56, "FwdCommon: the kernel argument layout of the five *Fwd structs");

// the nv distinct vectors u0 .. u0 + nv - 1 into LDS, sv[v * PV + k], by all THREADS threads of the work-group (no barrier here)
template <int THREADS>
__device__ __forceinline__ void stage_vectors(float* sv, const FwdCommon& c, int u0, int nv, int tid) {
    for (int v = 0; v < nv; ++v) {
        const float* src = c.base + c.run_off[u0 + v];
        for (int k = tid; k < c.P; k += THREADS) sv[v * c.PV + k] = src[k];
    }
}

// One lane per input row, the row's inputs in registers: row `row` of the block into x[I].  A lane past the last row computes
// row 0 and stores nothing (live = false).  xr serves a run-time input index, which goes to memory and not to the register array.
struct RowRef {
    const float* xr;
    bool live;
};
template <int I>
__device__ __forceinline__ RowRef load_row(const FwdCommon& c, int row, float (&x)[I]) {
    RowRef r;
    r.live = row < c.nrows;
    r.xr = c.x + (size_t)(c.row0 + (r.live ? row : 0)) * c.xs;
#pragma unroll
    for (int i = 0; i < I; ++i) x[i] = r.xr[i];
    return r;
}

// decode: w = W1 [I][H], W2 [H][O], B1 [H], B2 [O]
struct NetView {
    const float *W1, *W2, *B1, *B2;
};
template <int I, int O>
__device__ __forceinline__ NetView net_view(const float* w, int H) {
    NetView n;
    n.W1 = w;
    n.W2 = n.W1 + I * H;
    n.B1 = n.W2 + H * O;
    n.B2 = n.B1 + H;
    return n;
}

// sum_i x_i W1[i,h]: the I FMAs in ascending i, from 0.0f
template <int I>
__device__ __forceinline__ float hidden_preact(const float (&x)[I], const float* W1, int H, int h) {
    float z = 0.0f;
#pragma unroll
    for (int i = 0; i < I; ++i) z = fmaf(x[i], W1[i * H + h], z);
    return z;
}

// Two sigmoids that do not round alike; a kernel keeps the one it has.  The plain one: predict and forecast (the sampler's form).
__device__ __forceinline__ float sigmoid_plain(float z) { return 1.0f / (1.0f + expf(-z)); }

// The saturating one: sensitivity, pd, shapley and ale.  sigmoid(z) and its derivative without the cancellation 1 - sigmoid(z) of
// a saturated unit: e = exp(-|z|) <= 1, sigmoid = (z >= 0 ? 1 : e) / (1 + e), derivative = e / (1 + e)^2 -- a few ulp at any saturation
__device__ __forceinline__ void sigmoid_and_slope(float z, float* s, float* d) {
    const float e = expf(-fabsf(z)), q = 1.0f + e;
    *s = (z >= 0.0f ? 1.0f : e) / q;
    *d = e / (q * q);
}
__device__ __forceinline__ float sigmoid_sat(float z) {
    float s, d;
    sigmoid_and_slope(z, &s, &d);
    return s;
}

// classification: f = softmax(f) of the O output sigmoids (CLS:108-110); regression: f as it is
template <int TASK, int O>
__device__ __forceinline__ void softmax_head(float (&f)[O]) {
    if constexpr (TASK == TASK_CLS) {
        float sum = 0.0f;
#pragma unroll
        for (int o = 0; o < O; ++o) { f[o] = expf(f[o]); sum += f[o]; }
#pragma unroll
        for (int o = 0; o < O; ++o) f[o] = f[o] / sum;
    }
}

// f in: the O sums over the hidden units; out: the network's outputs -- the saturating output sigmoid (Q2), then the softmax
template <int TASK, int O>
__device__ __forceinline__ void output_head(float (&f)[O], const float* B2) {
#pragma unroll
    for (int o = 0; o < O; ++o) f[o] = sigmoid_sat(f[o] - B2[o]);
    softmax_head<TASK, O>(f);
}
