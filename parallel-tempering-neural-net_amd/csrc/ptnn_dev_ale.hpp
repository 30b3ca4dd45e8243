// ptnn_dev_ale.hpp -- part of ptnn_analysis_device.hpp (textually included there, inside namespace ptnn; not a stand-alone header):
// accumulated local effects of the sampled nets, first order and the second order of input pairs (ptnn_accumulated_effects,
// include/ptnn.h; Apley & Zhu 2020).  Nothing of the kind is in the reference.
//
//   b(n)        = the bin of row n's x_j among the edges z_0 .. z_K: the smallest k >= 1 with x_j <= z_k, K* when there is none
//   d_s[n,a,o]  = f_o(w_s; x_n with x_j := z_b) - f_o(w_s; x_n with x_j := z_{b-1})            the row moved across its own bin only
//   D2_s[n,q,o] = [f(u_k, v_m) - f(u_{k-1}, v_m)] - [f(u_k, v_{m-1}) - f(u_{k-1}, v_{m-1})]    pair q = (j, l), cell (k, m) of the row
//   z_h  = sum_i x_i W1[i,h] - B1[h]             the row as it is, once per hidden unit, shared by EVERY slot of the pass
//   zb_h = z_h + (v - x_l) W1[l,h]               the pair's second input at the lane's own edge value (dl = 0 without l)
//   zk_h = zb_h + (z - x_j) W1[j,h]              hi (z = z_b) and lo (z = z_{b-1}): the lane's own edges, not a wave-uniform grid value
//                                                (a pair with j > l swaps the two roles: the input with the larger index always goes
//                                                first, so that (l, j) evaluates the very corners of (j, l))
//   hid  = sigmoid(zk_h)   a_o = sum_h hid W2[h,o] - B2[o]   s_o = sigmoid(a_o)   classification: p = softmax(s) (CLS:108-110)
//
// A slot is (j, optional l at one of its two edges): it gives the two values f(hi), f(lo).  A first-order term is one slot; a
// second-order term is two, l at v_m and l at v_{m-1}.  Stage b of the call, as pd_forward_kernel is of partial dependence:
//   ale_forward_kernel<TASK, I, O> (per shape, AnalysisShape::ale_fwd): fx[col][u] = the local effect of distinct vector u, column
//   col = ((row * T + t) * O + o) of a block of input rows, T = A + Q terms, first-order slots then pairs -- the layout of
//   PredictFwd::fx, so predict_reduce_kernel and scatter_samples take the columns untouched; and the bin (cell) of every
//   (row, term) in an int32 plane for the reduce stage (ptnn_dev_ale_reduce.hpp, which ptnn_analysis.hip alone includes).
// Nothing here writes chain state, tapes, counters or trace rows, and nothing here uses an atomic.
//
// The invariant: f(hi) and f(lo) of a slot are functions of (vector, row, slot) alone.  Each is one whole pass over the hidden
// units in ascending order into accumulators of its own, so it does not depend on NV, on the chunk, on the tile slot it falls in,
// on the block of rows or on the wave that computed it.
constexpr int ALE_THREADS = 256;         // 4 waves
constexpr int ALE_MAX_NV = 16;           // distinct vectors per forward work-group
constexpr int ALE_MAX_EDGES = 64;        // edges per input, first order (PTNN_ALE_MAX_EDGES)
constexpr int ALE_MAX_EDGES2 = 16;       // edges per input of a pair (PTNN_ALE_MAX_EDGES2)
constexpr int ALE_MAX_PAIRS = 16;        // pairs per call (PTNN_ALE_MAX_PAIRS)
constexpr int ALE_MAX_ST = 10;           // slots per pass: with each slot's three per-lane deltas and two offsets a lane stays near 130 VGPRs

// The slots are tiled: one pass over the hidden units carries acc[o][slot][hi / lo], at most PD_ACC accumulators: O = 1, 2 -> 10
// slots, O = 3 -> 6, O = 10 -> 2, O = 18 -> 1 (a pair is then two passes).  A chunk (blockIdx.z) holds whole terms:
// ale_chunk_slots(O) slots, an even number.  The host plans with the same functions.
constexpr int ale_slot_tile(int O) { return PD_ACC / (2 * O) < 1 ? 1 : (PD_ACC / (2 * O) < ALE_MAX_ST ? PD_ACC / (2 * O) : ALE_MAX_ST); }
constexpr int ale_chunk_slots(int O) { return ale_slot_tile(O) < 2 ? 2 : ale_slot_tile(O) / 2 * 2; }
// LDS of a work-group beside the staged vectors and their tiles: per slot of the chunk three deltas per lane and two offsets
constexpr int ale_slot_floats(int O) { return ale_chunk_slots(O) * (3 * 64 + 2); }

// what the forward kernel needs (the host fills it; ptnn_analysis.hip: AlePlan)
struct AleFwd {
    FwdCommon c;
    int VS;                     // LDS stride of a vector's finished tile: chunk slots * 2 * O * 64 + a pad
    int A, Q;                   // first-order terms, pairs
    int E, E2;                  // edges per first-order input, edges per input of a pair
    int NCH1;                   // chunks of first-order terms: blockIdx.z < NCH1, then the chunks of pairs
    const int* inputs;          // [A] input index j of term a, in [0, I)
    const float* edges;         // [A][E]
    const int* pairs;           // [Q][2] (j, l)
    const float* edges2;        // [Q][2][E2]: u (of j), then v (of l)
    float* fx;                  // [nrows * (A + Q) * O][U] column-major
    int* bins;                  // [all rows][A + Q]: the 0-based bin k - 1 of a first-order term, the cell (k - 1) * K2 + (m - 1) of a pair
};

// the bin of x among e[0 .. K]: 1 + the number of edges e[k] < e[K], 1 <= k < K, that x lies above (edges equal to the last one
// are padding or the last edge itself); every edge read is wave-uniform
__device__ __forceinline__ int ale_bin(const float* __restrict__ e, int K, float x) {
    const float last = e[K];
    int b = 1;
    for (int k = 1; k < K; ++k) b += (x > e[k] && e[k] < last) ? 1 : 0;
    return b;
}

// One lane per input row with the row's inputs in registers, NV vectors staged in LDS, every weight read wave-uniform (an LDS
// broadcast): the pieces of ptnn_dev_net.hpp.  A work-group takes 64 rows, NV vectors and one chunk of whole terms.  First the four
// waves share the chunk's slots: per slot the lane's bin from its own x_j (x_l), the deltas to the bin's edges, the offsets of the two
// W1 rows -- into LDS, since every (vector, tile) pair of the work-group reads them -- and, in the work-groups of the first vectors,
// the bin (cell) index of the row into the plane.  Then the work is the nv x nt (vector, slot tile) pairs; wave w takes the pairs
// w, w + 4, ...  A pair is one pass over ALL hidden units in ascending order: z_h from the row as it is (I FMAs, once for the whole
// tile), then per slot three FMAs, two sigmoids and 2 O FMAs.  A tile slot past the chunk's last slot recomputes that slot and
// stores nothing.
template <int TASK, int I, int O>
__global__ void __launch_bounds__(ALE_THREADS) ale_forward_kernel(const AleFwd a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ST = ale_slot_tile(O), CS = ale_chunk_slots(O), NWAVE = ALE_THREADS / WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FwdCommon& cm = a.c;
    const int NV = cm.NV, PV = cm.PV, H = cm.H, VS = a.VS, T = a.A + a.Q;
    const int u0 = blockIdx.x * NV;
    const int nv = min(NV, cm.U - u0);
    const int r0 = blockIdx.y * WAVE;
    const bool second = (int)blockIdx.z >= a.NCH1;      // a chunk of pairs
    const int term0 = second ? ((int)blockIdx.z - a.NCH1) * (CS / 2) : (int)blockIdx.z * CS;      // first term of the chunk, within its kind
    const int nterm = second ? min(CS / 2, a.Q - term0) : min(CS, a.A - term0);                    // >= 1
    const int ns = second ? 2 * nterm : nterm;          // slots of this chunk
    const int nt = (ns + ST - 1) / ST;
    float* sv = smem;                                   // [NV][PV] the staged vectors
    float* fin = sv + (size_t)NV * PV;                  // [NV][VS] finished values: fin[v * VS + ((slot * 2 + lo) * O + o) * 64 + lane]
    float* sd = fin + (size_t)NV * VS;                  // [CS][3][64] per slot and lane: z_b - x_j, z_{b-1} - x_j, v - x_l
    int* so = reinterpret_cast<int*>(sd + CS * 3 * WAVE);   // [CS][2] per slot: the offsets of W1[j,:] and W1[l,:]
    stage_vectors<ALE_THREADS>(sv, cm, u0, nv, tid);
    const int row = r0 + lane;
    float x[I];
    const RowRef rr = load_row<I>(cm, row, x);
    const float* xr = rr.xr;
    const bool plane = rr.live && blockIdx.x == 0;      // this work-group writes the rows' bins
    for (int s = wave; s < ns; s += NWAVE) {
        int j, l = 0, bin;
        float dhi, dlo, dl = 0.0f;                      // fmaf(0, w, z) = z: no second input
        if (second) {
            const int q = term0 + (s >> 1), K2 = a.E2 - 1;
            j = a.pairs[2 * q]; l = a.pairs[2 * q + 1];
            const float* eu = a.edges2 + (size_t)(2 * q) * a.E2;
            const float* ev = eu + a.E2;
            const float xj = xr[j], xl = xr[l];         // the run-time index goes to memory, not to the register array
            const int bk = ale_bin(eu, K2, xj), bm = ale_bin(ev, K2, xl);
            if (j < l) {                                // the input with the larger index is substituted first: (l, j) evaluates the
                dhi = eu[bk] - xj; dlo = eu[bk - 1] - xj;       // same four corners as (j, l), bit for bit
                dl = ev[bm - (s & 1)] - xl;             // the even slot at v_m, the odd one at v_{m-1}
            } else {                                    // the roles swapped: hi / lo over x_l, the even slot at u_k, the odd one at u_{k-1}
                dhi = ev[bm] - xl; dlo = ev[bm - 1] - xl;
                dl = eu[bk - (s & 1)] - xj;
                const int t = j; j = l; l = t;
            }
            bin = (bk - 1) * K2 + (bm - 1);
            if (plane && (s & 1) == 0) a.bins[(size_t)(cm.row0 + row) * T + a.A + q] = bin;
        } else {
            const int t = term0 + s;
            j = a.inputs[t];
            const float* e = a.edges + (size_t)t * a.E;
            const float xj = xr[j];
            bin = ale_bin(e, a.E - 1, xj);
            dhi = e[bin] - xj; dlo = e[bin - 1] - xj;
            if (plane) a.bins[(size_t)(cm.row0 + row) * T + t] = bin - 1;
        }
        sd[(s * 3) * WAVE + lane] = dhi;
        sd[(s * 3 + 1) * WAVE + lane] = dlo;
        sd[(s * 3 + 2) * WAVE + lane] = dl;
        if (lane == 0) { so[2 * s] = j * H; so[2 * s + 1] = l * H; }
    }
    __syncthreads();
    for (int p = wave; p < nv * nt; p += NWAVE) {
        const int v = p / nt, t0 = (p % nt) * ST;       // wave-uniform
        const NetView n = net_view<I, O>(sv + v * PV, H);
        const float* W1 = n.W1;
        int oj[ST], ol[ST];
        float dhi[ST], dlo[ST], dl[ST], acc[O][ST][2];
#pragma unroll
        for (int k = 0; k < ST; ++k) {
            const int s = min(t0 + k, ns - 1);          // slot of the chunk
            oj[k] = so[2 * s]; ol[k] = so[2 * s + 1];
            dhi[k] = sd[(s * 3) * WAVE + lane]; dlo[k] = sd[(s * 3 + 1) * WAVE + lane]; dl[k] = sd[(s * 3 + 2) * WAVE + lane];
#pragma unroll
            for (int o = 0; o < O; ++o) acc[o][k][0] = acc[o][k][1] = 0.0f;
        }
        for (int h = 0; h < H; ++h) {
            float z = 0.0f;
            if constexpr (I > 16 && I < 32) {
                // 20 inputs: hidden_preact's form keeps the I row offsets i * H in scalar registers and the compiler then spills 17
                // of them; a weight pointer it must hold in a vector register (the empty asm) costs one add per FMA here and no
                // spill.  The same FMAs in the same order.
                const float* wp = W1 + h;
#pragma unroll
                for (int i = 0; i < I; ++i) { z = fmaf(x[i], *wp, z); wp += H; asm volatile("" : "+v"(wp)); }
            } else {
                z = hidden_preact<I>(x, W1, H, h);
            }
            z -= n.B1[h];                                                   // Q1
            float w2[O];
#pragma unroll
            for (int o = 0; o < O; ++o) w2[o] = n.W2[h * O + o];
#pragma unroll
            for (int k = 0; k < ST; ++k) {
                const float w1j = W1[oj[k] + h];
                const float zb = fmaf(dl[k], W1[ol[k] + h], z);
                const float hh = sigmoid_sat(fmaf(dhi[k], w1j, zb)), hl = sigmoid_sat(fmaf(dlo[k], w1j, zb));
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    acc[o][k][0] = fmaf(hh, w2[o], acc[o][k][0]);
                    acc[o][k][1] = fmaf(hl, w2[o], acc[o][k][1]);
                }
            }
        }
        float* out = fin + (size_t)v * VS + lane;
#pragma unroll
        for (int k = 0; k < ST; ++k) {
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                float f[O];
#pragma unroll
                for (int o = 0; o < O; ++o) f[o] = acc[o][k][e2];
                output_head<TASK, O>(f, n.B2);
                if (t0 + k < ns) {
#pragma unroll
                    for (int o = 0; o < O; ++o) out[(((t0 + k) * 2 + e2) * O + o) * WAVE] = f[o];
                }
            }
        }
    }
    __syncthreads();
    // column-major store: column ((r0 + l) * T + term) * O + o of the block gets NV consecutive floats.  The differences are formed
    // in double from the fp32 values and rounded to fp32 once: hi - lo, and for a pair (hi - lo at v_m) - (hi - lo at v_{m-1}).
    const int tbase = second ? a.A + term0 : term0;
    for (int idx = tid; idx < nterm * O * WAVE * NV; idx += ALE_THREADS) {
        const int v = idx % NV, c = idx / NV, l = c % WAVE, to = c / WAVE, tt = to / O, o = to % O;
        if (v < nv && r0 + l < cm.nrows) {
            const float* fv = fin + (size_t)v * VS + l;
            const int s = second ? 2 * tt : tt;
            const double f0 = (double)fv[((s * 2) * O + o) * WAVE], f1 = (double)fv[((s * 2 + 1) * O + o) * WAVE];
            double d = f0 - f1;
            if (second) {
                const double f2 = (double)fv[(((s + 1) * 2) * O + o) * WAVE], f3 = (double)fv[(((s + 1) * 2 + 1) * O + o) * WAVE];
                const int q = term0 + tt;
                // the stated order [f(u_k, v_m) - f(u_{k-1}, v_m)] - [f(u_k, v_{m-1}) - f(u_{k-1}, v_{m-1})], whichever input the slots hold
                d = a.pairs[2 * q] < a.pairs[2 * q + 1] ? (f0 - f1) - (f2 - f3) : (f0 - f2) - (f1 - f3);
            }
            a.fx[(((size_t)(r0 + l) * T + tbase + tt) * O + o) * cm.U + u0 + v] = (float)d;
        }
    }
}
