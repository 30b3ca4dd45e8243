// ptnn.hip -- host side of libptnn.so: the C ABI of include/ptnn.h over the gfx950 kernels of ptnn_device.hpp.
//
// Replaces, for the hot path only, what the reference does with one forked ptReplica process per chain plus the
// parent's swap loop (REG = multicore-pt-regression/pt_timeseries_regression.py:223-485, 659-771;
// CLS = multicore-pt-classification/pt_classification.py:232-494, 668-776).
#include "ptnn_shapes.hpp"
#include "ptnn_comm.hpp"
#include "ptnn_text.hpp"
#include "../../include/ptnn.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sched.h>

using namespace ptnn;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            (void)hipGetLastError(); /* reported here: must not surface again at the next launch check */   \
            return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
        }                                                                                                  \
    } while (0)

}  // namespace

// one table per shape, each defined in its own translation unit (ptnn_shape.hip)
#define X_DECL(T, I, O) extern "C" const ptnn::Shape ptnn_shape_##T##_##I##_##O;
PTNN_SHAPES(X_DECL)
#undef X_DECL

namespace {

#define X_ENTRY(T, I, O) &ptnn_shape_##T##_##I##_##O,
const Shape* const g_shapes[] = {PTNN_SHAPES(X_ENTRY)};
#undef X_ENTRY
constexpr int MAX_HIDDEN = MAX_WAVES * WAVE;    // wide nets: one thread per hidden unit

const Shape* find_shape(int task, int I, int O) {
    for (const Shape* s : g_shapes)
        if (s->task == task && s->I == I && s->O == O) return s;
    return nullptr;
}

inline int round_up4(int v) { return (v + 3) & ~3; }

constexpr size_t LDS_MAX = 160 * 1024;          // LDS of one work-group
constexpr size_t LDS_CEILING = 152 * 1024;      // largest dynamic-LDS ceiling the runtime accepts (just below LDS_MAX it refuses)

enum SegKind { SEG_COOP, SEG_SPEC, SEG_PACK, SEG_PACKM, SEG_TREE, SEG_WIDE, SEG_WIDE_RES, SEG_KINDS };   // the segment kernels

struct SegKernel {
    const char* name;       // ptnn_describe's "kernel"
    const char* label;      // ... and "schedule" (wide nets over several work-groups: "speculative-wide")
    seg_fn Shape::*fn;
    bool per_group;         // the grid has `groups` work-groups per replica (else one)
};
const SegKernel g_seg[SEG_KINDS] = {
    {"segment_kernel", "cooperative", &Shape::seg, false},
    {"segment_spec_kernel", "speculative", &Shape::spec, true},
    {"segment_pack_kernel", "packed-speculative", &Shape::pack, false},             // one CU per replica
    {"segment_packm_kernel", "packed-speculative", &Shape::packm, true},
    {"segment_tree_kernel", "prefetching-tree", &Shape::tree, true},
    {"segment_wide_kernel", "cooperative-wide", &Shape::seg_wide, true},
    {"segment_wide_res_kernel", "cooperative-wide", &Shape::seg_wide_res, true},
};

// What ptnn_set_data decided: the segment kernel, its launch shape and the buffers it needs (plan_launch)
struct LaunchPlan {
    SegKind kind = SEG_COOP;
    int threads = 64, model_threads = 64;       // segment kernel; model_kernel / model_wide_kernel (ptnn_evaluate and friends)
    size_t seg_lds = 0, model_lds = 0;
    int groups = 1;                 // work-groups (CUs) per replica; tree: 2^depth - 1
    int pk_nred = 3;                // packed schedules: lane-group width 2^3 (H <= 8) or 2^4 hidden units
    int fw_mfma = 0;                // forward pass on the matrix cores: 1 exact fp32, 2 split bf16 operands
    bool xy_global = false;         // split forward pass: no room for the row-major data image in LDS, its rare readers go to global memory
    bool tree_ahead = false;        // tree: room in LDS for two sets of tapes
    bool compact = false;           // wide nets with all trace rows resident: rejected steps record a row index, no pos_w row
    int blocks_per_cu = 0;          // occupancy of the segment kernel as the runtime reports it (0 = not queried)
    bool persistent = false;        // all work-groups of the grid are resident: ptnn_run queues ONE launch, swap rounds inside
    // bytes of the buffers the plan needs (0 = none): multi-group exchange slots / rows / verdicts, in-launch swap granules, wide scratch
    size_t xslots = 0, xw = 0, xverdict = 0, xswap = 0, wide_scratch = 0;
    bool wide() const { return kind == SEG_WIDE || kind == SEG_WIDE_RES; }
    int grid(int replicas) const { return replicas * (g_seg[kind].per_group ? groups : 1); }
};

}  // namespace

struct ptnn_handle {
    ptnn_config cfg{};
    const Shape* shape = nullptr;
    hipStream_t stream = nullptr;
    int P = 0, PS = 0, PW = 0, IPY = 0, FWS = 0, Ntr = 0, Nte = 0;
    LaunchPlan plan;
    unsigned* d_barrier = nullptr;  // grid barrier of the persistent launch: one slot per work-group
    int barrier_slots = 0;
    float* d_wide_scratch = nullptr;
    float* d_xt = nullptr;          // transposed data image for the MFMA forward pass
    uint16_t* d_xs = nullptr;       // wide nets: the data image split into three bf16 levels (split-operand forward pass)
    int Npad = 0;
    unsigned epoch_base = 0;
    int num_cus = 0;
    unsigned long long *d_xslots = nullptr, *d_xw = nullptr, *d_xverdict = nullptr, *d_xswap = nullptr;
    int* d_error = nullptr;
    float *h_stage = nullptr, *d_stage = nullptr;   // initial weights + temperatures on their way to the device (ptnn_set_state)
    int* h_progress = nullptr;      // pinned host word: swap rounds the device has completed (swap_kernel stores it)
    bool failed = false;            // a run on this handle ended in an error (-5 / -7): results are refused until the chains restart
    std::string failure;
    unsigned long long* d_stamps = nullptr;
    bool have_data = false, have_state = false, finalized = false;
    int cap = 0;            // trace ring rows per replica
    int drained = 0;        // rows [0, drained] have been fetched by the caller (streaming mode)
    int first_row = 0;      // trace rows below this one are not on this device (chains restored from a checkpoint)
    int cur = 0;            // next MH step index
    int rounds_done = 0;    // swap rounds counted (including the phantom one)
    int max_rounds = 0;
    int flip = 0;           // which state buffer is current
    // device memory
    float* d_data = nullptr;
    float* d_state[2] = {nullptr, nullptr};
    float *d_rec_w = nullptr, *d_st_f = nullptr, *d_temps = nullptr;
    float* d_gd_w[2] = {nullptr, nullptr};
    int* d_gd_valid[2] = {nullptr, nullptr};
    int* d_st_i = nullptr;
    float *d_L_handoff = nullptr, *d_L_final = nullptr;
    float *d_L_raw = nullptr, *d_prior_post = nullptr, *d_temps_global = nullptr;   // swap_rule 1
    bool have_ladder = false;
    // ladder adaptation during burn-in (ptnn_set_ladder_adaptation, ptnn_dev_ladder.hpp): histories on the device, the initial
    // ladder and log-gaps on the host (a restart starts from them again)
    bool have_adapt = false;
    ptnn_ladder_adapt_spec adapt{};
    float* d_lad_hist = nullptr;    // [A+1][R]
    double* d_lad_s = nullptr;      // [2][R-1]
    float* d_lad_acc = nullptr;     // [max_rounds][R-1]
    std::vector<float> lad_T0;
    std::vector<double> lad_s0;
    int *d_label[2] = {nullptr, nullptr}, *d_slot_of[2] = {nullptr, nullptr};   // label_swap: slot <-> temperature maps, ping-pong
    int lflip = 0;
    float *d_pos_w = nullptr;       // [Rl][cap][PW]
    float *d_scal = nullptr;        // [Rl][cap][TR_COUNT] scalar trace rows
    int *d_src = nullptr, *d_src_log = nullptr;
    int* h_src = nullptr;
    float* d_xchg = nullptr;                                // [R_global][XS] exchange rows of the gathered sharding mode                                   // pinned staging for the permutation of a round (sharded ladder)
    long long* d_counters = nullptr;
    // sharded ladder: transport and what a swap round moves through it
    Comm comm;
    std::vector<RowMsg> route;
    // trace images on the host (ptnn_trace_image*): pinned copies of d_pos_w / d_scal that a second stream fills while the chains
    // go on sampling
    hipStream_t copy_stream = nullptr;
    float *h_img_pos = nullptr, *h_img_rows = nullptr;
    std::vector<hipEvent_t> img_events;                     // ticket k: the copy of its rows has landed
    // kernel timing (HIP events on our stream)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing;
    size_t timing_used = 0;
    int timing_stride = 1;          // PTNN_TIMING_STRIDE: 0 = never, n = every n-th segment launch
    long long launch_count = 0;
    int64_t timed_launches = 0;
    double timed_ms = 0.0;

    SegParams seg_params() const {
        SegParams p{};
        p.H = cfg.n_hidden; p.P = P; p.PS = PS;
        p.Ntr = Ntr; p.Nte = Nte; p.IPY = IPY; p.FWS = FWS;
        p.S = cfg.n_samples; p.switch_step = cfg.pt_switch_step; p.use_lg = cfg.use_langevin;
        p.trace_cap = cap;
        p.first_global = cfg.first_global_replica;
        p.l_prob = cfg.l_prob; p.lr = cfg.learn_rate; p.step_w = cfg.step_w; p.step_eta = cfg.step_eta;
        p.inv_2sig2 = 1.0f / (2.0f * cfg.sigma_squared);
        const int I = cfg.n_in, H = cfg.n_hidden, O = cfg.n_out;
        // part1 of prior_likelihood: REG uses d*h + h + 2 (REG:218), CLS d*h + h + o + h*o (CLS:227)
        const double cnt = (cfg.task == PTNN_TASK_REG) ? (double)(I * H + H + 2) : (double)(I * H + H + O + H * O);
        p.prior_c = (float)(-1.0 * (cnt / 2.0) * std::log((double)cfg.sigma_squared));
        p.nu1 = cfg.nu_1; p.nu2 = cfg.nu_2;
        p.seed_lo = (uint32_t)(cfg.seed & 0xffffffffull); p.seed_hi = (uint32_t)(cfg.seed >> 32);
        p.data = d_data; p.w_state = d_state[flip]; p.rec_w = d_rec_w; p.gd_w = d_gd_w[flip]; p.gd_valid = d_gd_valid[flip];
        p.st_f = d_st_f; p.st_i = d_st_i; p.temps = d_temps;
        p.L_handoff = d_L_handoff; p.L_final = d_L_final;
        p.L_raw = (cfg.swap_rule == 1) ? d_L_raw : nullptr; p.prior_post = d_prior_post;
        p.tr_pos_w = d_pos_w; p.tr_scal = d_scal; p.PW = PW;
        p.G = plan.groups; p.epoch_base = epoch_base; p.xslots = d_xslots; p.xw = d_xw; p.xverdict = d_xverdict; p.error_flag = d_error; p.stamps = d_stamps; p.wide_scratch = d_wide_scratch; p.noise_shared = cfg.shared_noise ? 1 : 0; p.pk_nred = plan.pk_nred; p.xt = d_xt; p.xs = reinterpret_cast<const uint4*>(d_xs); p.Npad = Npad; p.fw_mfma = plan.fw_mfma; p.xy_global = plan.xy_global ? 1 : 0; p.forward_bf16 = cfg.forward_bf16 == 1 ? 1 : 0; p.tree_ahead = plan.tree_ahead ? 1 : 0; p.compact = plan.compact ? 1 : 0;
        {
            // records through the XCD's L2: asked for only where xcd_block (ptnn_device.hpp) can put a replica's work-groups on one XCD --
            // a grid of 8 k blocks with k a multiple of the groups per replica; elsewhere the in-kernel handshake could only time out
            const int grid_ = cfg.n_replicas_local * plan.groups;
            const bool can = plan.groups > 1 && (grid_ & 7) == 0 && ((grid_ >> 3) % plan.groups) == 0;
            p.xcd_granules = (cfg.shared_device || !can) ? 0 : 1;
        }
        p.xswap = d_xswap;
        // wide nets over several work-groups: a window of 16 steps lets the groups balance Langevin (10 units) against random-walk
        // (1) steps (measured on config 5: 8 steps 0.680 M, 12: 0.692 M, 16: 0.698 M samples/s; wide nets accept 1 - 5 %, so little of
        // a window is thrown away); random-walk-only runs have nothing to balance and a longer window only wastes what follows an accept
        p.wide_window = cfg.use_langevin ? 16 : plan.groups;
        return p;
    }
};

namespace {

int wait_stream(ptnn_handle* h);

inline int tree_depth(int groups) { int d = 0; while ((1 << (d + 1)) - 1 <= groups) ++d; return d; }   // groups = 2^d - 1

// Q10: REG hands off after step i when i % si == 0 and i != 0 (REG:427); CLS when (i+1) % si == 0 (CLS:438)
inline bool swap_trigger(const ptnn_config& c, int i) {
    if (c.task == PTNN_TASK_REG) return (i % c.swap_interval == 0) && i != 0;
    return ((i + 1) % c.swap_interval) == 0;
}

seg_fn segment_function(const Shape* sh, SegKind k) { return sh->*g_seg[k].fn; }

void collect_timing(ptnn_handle* h) {
    for (size_t k = 0; k < h->timing_used; ++k) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->timing[k].first, h->timing[k].second) == hipSuccess) {
            h->timed_ms += ms;
            h->timed_launches += 1;
        }
    }
    h->timing_used = 0;
}

void fill_swap_params(ptnn_handle* h, bool phantom, SwapParams& sp) {
    sp.R = h->cfg.n_replicas_global; sp.Rl = h->cfg.n_replicas_local; sp.first_global = h->cfg.first_global_replica;
    sp.PS = h->PS;
    sp.seed_lo = (uint32_t)(h->cfg.seed & 0xffffffffull); sp.seed_hi = (uint32_t)(h->cfg.seed >> 32);
    sp.L = phantom ? h->d_L_final : h->d_L_handoff;
    sp.cur = h->d_state[h->flip]; sp.next = h->d_state[h->flip ^ 1];
    sp.gd_cur = h->d_gd_w[h->flip]; sp.gd_next = h->d_gd_w[h->flip ^ 1];
    sp.gd_valid_cur = h->d_gd_valid[h->flip]; sp.gd_valid_next = h->d_gd_valid[h->flip ^ 1];
    sp.src_out = nullptr;
    sp.counters = h->d_counters; sp.src_log = h->d_src_log; sp.log_capacity = h->max_rounds;
    sp.rule = h->cfg.swap_rule; sp.L_raw = h->d_L_raw; sp.prior_post = h->d_prior_post; sp.temps_global = h->d_temps_global;
    sp.st_f = h->d_st_f;
    sp.canonical = (h->cfg.pt_switch_step >= 0 && h->cur - 1 >= h->cfg.pt_switch_step) ? 1 : 0;
    sp.xchg = h->d_xchg; sp.XS = xchg_row_floats(h->PS); sp.L_stride = 1;
    sp.label_mode = h->cfg.label_swap ? 1 : 0;
    sp.label_cur = h->d_label[h->lflip]; sp.slot_cur = h->d_slot_of[h->lflip];
    sp.label_next = h->d_label[h->lflip ^ 1]; sp.slot_next = h->d_slot_of[h->lflip ^ 1];
    sp.temps_local = h->d_temps;
    sp.progress = nullptr;
    if (h->have_adapt) {
        const int R = h->cfg.n_replicas_global;
        sp.lad_hist = h->d_lad_hist; sp.lad_s = h->d_lad_s; sp.lad_acc = h->d_lad_acc; sp.lad_out = h->d_temps_global;
        sp.lad_A = h->adapt.rounds; sp.lad_acc_cap = h->max_rounds;
        sp.lad_kappa0 = h->adapt.kappa0; sp.lad_t0 = h->adapt.t0;
        sp.temps_global = h->d_lad_hist + (size_t)std::min(h->rounds_done, h->adapt.rounds) * R;   // the ladder of this round
    } else {
        sp.lad_hist = nullptr; sp.lad_s = nullptr; sp.lad_acc = nullptr; sp.lad_out = nullptr;
        sp.lad_A = 0; sp.lad_acc_cap = 0; sp.lad_kappa0 = 0.0; sp.lad_t0 = 0.0;
    }
}

// drop the adaptation buffers (ptnn_set_ladder, a new spec, a checkpoint without one)
void ladder_adapt_release(ptnn_handle* h) {
    for (void* p : {(void*)h->d_lad_hist, (void*)h->d_lad_s, (void*)h->d_lad_acc})
        if (p) (void)hipFree(p);
    h->d_lad_hist = nullptr; h->d_lad_s = nullptr; h->d_lad_acc = nullptr;
    h->have_adapt = false; h->adapt = ptnn_ladder_adapt_spec{};
    h->lad_T0.clear(); h->lad_s0.clear();
}

int ladder_adapt_alloc(ptnn_handle* h, const ptnn_ladder_adapt_spec& spec) {
    ladder_adapt_release(h);
    const size_t R = h->cfg.n_replicas_global;
    HIP_TRY(hipMalloc(&h->d_lad_hist, (size_t)(spec.rounds + 1) * R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_lad_s, 2 * (R - 1) * sizeof(double)));
    HIP_TRY(hipMalloc(&h->d_lad_acc, (size_t)h->max_rounds * (R - 1) * sizeof(float)));
    h->adapt = spec; h->have_adapt = true;
    return 0;
}

// the adaptation back at its start: ladder row 0 = the initial ladder (also in d_temps_global), s = its log-gaps, rows not yet
// written are NaN
int ladder_adapt_reset(ptnn_handle* h) {
    const size_t R = h->cfg.n_replicas_global;
    HIP_TRY(hipMemsetAsync(h->d_lad_hist, 0xff, (size_t)(h->adapt.rounds + 1) * R * sizeof(float), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_lad_acc, 0xff, (size_t)h->max_rounds * (R - 1) * sizeof(float), h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_lad_hist, h->lad_T0.data(), R * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_temps_global, h->lad_T0.data(), R * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_lad_s, h->lad_s0.data(), (R - 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));            // the host vectors are pageable and may change later
    return 0;
}

// MH steps [begin, end) in one launch.  swap_inside: the swap rounds between the intervals run inside it (persistent launch:
// every work-group resident, grid barriers); otherwise [begin, end) is one interval and the caller queues swap_kernel behind it.
int launch_segment(ptnn_handle* h, int begin, int end, bool swap_inside = false, bool round_follows = false) {
    if (end <= begin) return 0;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    SegParams p = h->seg_params();
    if (round_follows && h->comm.kind == COMM_RCCL) { p.seg_progress = h->h_progress + 1; p.seg_ordinal = h->rounds_done + 1; }
    PersistParams pp{};
    pp.end = end; pp.swap_inside = swap_inside ? 1 : 0; pp.task = h->cfg.task; pp.si = h->cfg.swap_interval;
    pp.round0 = h->rounds_done; pp.flip0 = h->flip; pp.lflip0 = h->lflip;
    const int grid = h->plan.grid(h->cfg.n_replicas_local);
    pp.nblocks = grid; pp.barrier = h->d_barrier;
    for (int b = 0; b < 2; ++b) {
        pp.state[b] = h->d_state[b]; pp.gd[b] = h->d_gd_w[b]; pp.gd_valid[b] = h->d_gd_valid[b];
        pp.label[b] = h->d_label[b]; pp.slot_of[b] = h->d_slot_of[b];
    }
    fill_swap_params(h, false, pp.sp);
    if (swap_inside) {
        if (grid > h->barrier_slots) {
            if (h->d_barrier) HIP_TRY(hipFree(h->d_barrier));
            h->d_barrier = nullptr;
            HIP_TRY(hipMalloc(&h->d_barrier, (size_t)grid * sizeof(unsigned)));
            h->barrier_slots = grid;
            pp.barrier = h->d_barrier;
        }
        HIP_TRY(hipMemsetAsync(h->d_barrier, 0, (size_t)grid * sizeof(unsigned), h->stream));
    }
    // event pairs around a launch cost a pipeline bubble each; time every timing_stride-th launch only
    const bool timed = h->timing_stride > 0 && (h->launch_count++ % h->timing_stride) == 0;
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    if (timed) {
        if (h->timing_used == h->timing.size()) {
            if (h->timing.size() >= 4096) {               // keep the pool bounded: drain it (synchronises)
                if (int rc = wait_stream(h)) return rc;
                collect_timing(h);
            } else {
                hipEvent_t a, b;
                HIP_TRY(hipEventCreate(&a));
                HIP_TRY(hipEventCreate(&b));
                h->timing.emplace_back(a, b);
            }
        }
        ev = &h->timing[h->timing_used++];
        HIP_TRY(hipEventRecord(ev->first, h->stream));
    }
    hipLaunchKernelGGL(segment_function(h->shape, h->plan.kind), dim3(grid), dim3(h->plan.threads), h->plan.seg_lds, h->stream, p, pp, begin);
    h->epoch_base += (unsigned)(end - begin) + 1u + (swap_inside ? (unsigned)((end - begin) / h->cfg.swap_interval + 2) : 0u);   // granule tags never repeat across launches
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev->second, h->stream));
    return 0;
}

// mode bit 0 = apply moves (and flip), bit 1 = count + log, bit 2 = L and the source rows come from the gathered exchange
// buffer; src_out optional.  mode -1 = pack the exchange rows of the local replicas.
int launch_swap(ptnn_handle* h, bool phantom, int mode, bool want_src) {
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    SwapParams sp{};
    fill_swap_params(h, phantom, sp);
    sp.src_out = want_src ? h->d_src : nullptr;
    sp.progress = (mode >= 0 && (mode & 2)) ? h->h_progress : nullptr;     // the counting pass of a round is its last kernel
    if (mode == -1) {
        hipLaunchKernelGGL(xchg_pack_kernel, dim3(sp.Rl), dim3(64), 0, h->stream, sp);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (mode & 4) {
        sp.L = h->d_xchg + 2 * h->PS + 1; sp.L_stride = sp.XS;
        sp.L_raw = h->d_xchg + 2 * h->PS + 2; sp.prior_post = h->d_xchg + 2 * h->PS + 3;
    }
    const size_t lds = (size_t)(3 * sp.R + 1) * sizeof(float);        // L, ln 2u, src (+ count)
    const int swap_threads = (sp.R <= 512 && sp.PS <= 256) ? 64 : 256;     // more threads for long ladders and long rows
    hipLaunchKernelGGL(swap_kernel, dim3(sp.Rl), dim3(swap_threads), lds, h->stream, sp, h->rounds_done, mode);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The dynamic-LDS ceiling of a kernel is a property of the function, shared by every handle of the process: only ever raise
// it, so that a handle created later with a smaller data set does not pull it below what an earlier one launches with.
int raise_lds_limit(const void* func, size_t bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> limit;
    if (bytes <= 64 * 1024) return 0;
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[func];
    if (bytes > cur) {
        HIP_TRY(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        cur = bytes;
    }
    return 0;
}

// Wait for everything queued on the handle's stream.  With an RCCL communicator attached the wait is bounded: a collective
// whose peer never arrives would otherwise block the host for ever (the reference's parent at least polls is_alive() every
// round, REG:721-727).  "No progress" = the stream is busy and the device has not completed a swap round (swap_kernel stores the
// round count into a pinned host word) for comm_timeout_s() seconds; a long segment between two rounds is far below that.
int wait_stream(ptnn_handle* h) {
    if (h->comm.kind != COMM_RCCL) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        return 0;
    }
    const double limit = comm_timeout_s();
    volatile int* prog = h->h_progress;      // [0] swap rounds completed, [1] index + 1 of the round whose segment has ended
    int seen0 = prog[0], seen1 = prog[1];
    double t_seen = comm_clock();
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) return fail(-2, "hipStreamQuery failed: %s", hipGetErrorString(q));
        const int now0 = prog[0], now1 = prog[1];
        // the clock runs only while a collective is at the head of the stream: the segment before round k has ended (prog[1] ==
        // k + 1) and the round has not (prog[0] == k).  A segment, however long, is bounded by its own kernel spins.
        if (now0 != seen0 || now1 != seen1 || now1 <= now0) { seen0 = now0; seen1 = now1; t_seen = comm_clock(); }
        else if (comm_clock() - t_seen > limit) {
            h->failed = true; h->comm.failed = true;
            h->failure = "no progress on the handle's stream for " + std::to_string((int)limit) + " s inside swap round " + std::to_string(now0) +
                         " (" + std::to_string(h->rounds_done) + " queued); last communicator stage: " + comm_last_stage();
            return fail(-7, "%s", h->failure.c_str());
        }
        if (spins < 4096) sched_yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// wait_stream + the device's error flag: a bounded spin that expired inside a segment kernel invalidates the run
int finish_stream(ptnn_handle* h) {
    if (h->failed) return fail(h->failure.find("no progress") == 0 ? -7 : -5, "%s", h->failure.c_str());
    if (int rc = wait_stream(h)) return rc;
    int err = 0;
    HIP_TRY(hipMemcpy(&err, h->d_error, sizeof(int), hipMemcpyDeviceToHost));
    if (err) {
        h->failed = true;
        h->failure = "a cross-work-group hand-off timed out inside the segment kernel (" + std::to_string(err) +
                     " work-groups gave up); the run is invalid -- restart the chains (ptnn_set_state / ptnn_checkpoint_load); schedules "
                     "with several work-groups per replica expect the GPU to themselves";
        return fail(-5, "%s", h->failure.c_str());
    }
    return 0;
}

// wide nets: the split-operand forward pass (SplitK, eval_rows_mfma_wsplit) unless the caller asked for bf16 or exact fp32 operands
bool wide_split(const ptnn_handle& h) {
    const int H = h.cfg.n_hidden;
    return H > WAVE && H % 32 == 0 && h.shape->split_ch > 0 && h.cfg.forward_bf16 == 0;
}

// LDS of the split-operand images of the cooperative / tree forward pass
size_t split_lds_bytes(const ptnn_handle& h, int Npad) {
    return (split_lds_floats(h.shape->split_ch, h.shape->split_kr, h.cfg.n_out, h.cfg.n_hidden, Npad) + 4) * sizeof(float);
}

// exchange buffers of the multi-group schedules (segment_spec_body's layout): slots, rows of `row_groups` x 2 vectors, verdicts
void plan_exchange(const ptnn_handle& h, int row_groups, LaunchPlan& plan) {
    const size_t Rl = h.cfg.n_replicas_local, g = sizeof(unsigned long long);
    plan.xslots = Rl * 2 * MAX_SLOTS * SL_COUNT * g;
    plan.xw = Rl * 2 * row_groups * 2 * h.PS * g;
    plan.xverdict = Rl * 2 * MAX_SLOTS * g;
}

// Granules of the swap rounds a multi-group launch runs by itself (ptnn_device.hpp: segment_tree_body, segment_pack_body<MULTI>): two
// parities of swap_xchg_granules(R, row); only when the whole ladder is on this handle (a sharded ladder exchanges through its communicator)
size_t swap_granule_bytes(const ptnn_handle& h, int row) {
    if (h.cfg.n_replicas_local != h.cfg.n_replicas_global) return 0;
    return 2 * swap_xchg_granules(h.cfg.n_replicas_global, row) * sizeof(unsigned long long);
}

// Wide net (64 < H): one thread per hidden unit, vectors in HBM, only the packed forward image + scratch in LDS.  Matrix-core layout
// (H a multiple of 32): the state vector joins the proposal in LDS when both fit.
int plan_wide(const ptnn_handle& h, LaunchPlan& plan) {
    const int H = h.cfg.n_hidden, Rl = h.cfg.n_replicas_local;
    plan.fw_mfma = wide_split(h) ? 2 : 0;
    const size_t lds_res = wide_lds_floats(H, h.FWS, h.cfg.n_out, h.PS, true) * sizeof(float);
    plan.kind = (H % 32 == 0 && lds_res <= LDS_CEILING) ? SEG_WIDE_RES : SEG_WIDE;
    const size_t lds = plan.kind == SEG_WIDE_RES ? lds_res : wide_lds_floats(H, h.FWS, h.cfg.n_out, h.PS) * sizeof(float);
    if (lds > LDS_MAX) return fail(-3, "wide net needs %zu B of LDS (> 160 KiB)", lds);
    if (h.cfg.schedule == PTNN_SCHED_SPECULATIVE || h.cfg.schedule == PTNN_SCHED_PACKED || h.cfg.schedule == PTNN_SCHED_TREE)
        return fail(-3, "schedules 2-4 are built for n_hidden <= 64; a wide net speculates over work-groups through groups_per_replica");
    plan.compact = h.cap == h.cfg.n_samples;
    plan.threads = plan.model_threads = ((H + WAVE - 1) / WAVE) * WAVE;
    plan.seg_lds = plan.model_lds = lds;
    // Speculation over work-groups (one per CU): group g computes step i + g; all Rl x G groups must be resident (they wait for each
    // other's verdicts).  groups_per_replica 1, 2 or 4; 0 = as many of 4, 2 as are resident, else 1.
    const void* fn = reinterpret_cast<const void*>(segment_function(h.shape, plan.kind));
    if (int rc = raise_lds_limit(fn, lds)) return rc;
    const int want = h.cfg.groups_per_replica;
    if (want != 0 && want != 1 && want != 2 && want != 4) return fail(-1, "wide nets: groups_per_replica must be 0 (auto), 1, 2 or 4");
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, plan.threads, lds));
    plan.blocks_per_cu = per_cu;
    const long long cap = (long long)per_cu * h.num_cus;
    if (want > 1) {
        if ((long long)Rl * want > cap)
            return fail(-3, "%d replicas x %d work-groups cannot all be resident: %d work-group(s) of %d threads with %zu B of LDS fit "
                            "on each of the %d CUs", Rl, want, per_cu, plan.threads, lds, h.num_cus);
        plan.groups = want;
    } else if (want == 0 && !h.cfg.shared_device) {     // (work-groups that wait for each other want the GPU to themselves)
        if ((long long)Rl * 4 <= cap) plan.groups = 4;
        else if ((long long)Rl * 2 <= cap) plan.groups = 2;
    }
    plan.wide_scratch = (size_t)Rl * plan.groups * 5 * h.PS * sizeof(float);
    if (plan.groups > 1) plan_exchange(h, plan.groups, plan);
    return 0;
}

// Packed speculative: all slots of a round on one CU, the SGD epochs of the slots in the lane groups of two waves: 16 slots in groups
// of 8 lanes for n_hidden <= 8, 8 slots in groups of 16 lanes for n_hidden <= 16.  Taken automatically for Langevin runs of such nets
// (faster than 4 CUs per replica on a quarter of the GPU, and more than twice the throughput once there are more replicas than CUs);
// random-walk-only runs have no epochs to pack and keep the multi-CU speculative schedule.  Leaves the plan alone when not taken.
int plan_packed(const ptnn_handle& h, int Nall, int sched, LaunchPlan& plan) {
    const ptnn_config& c = h.cfg;
    const int H = c.n_hidden, Rl = c.n_replicas_local;
    const size_t pk = pack_lds_floats(Nall, h.IPY, h.PS, H, h.FWS, pack_slots(plan.pk_nred)) * sizeof(float);
    const bool fits = H <= 16 && pk <= LDS_MAX;
    if (sched == PTNN_SCHED_PACKED && !fits)
        return fail(-3, "the packed schedule needs n_hidden <= 16 and %zu B of LDS <= 160 KiB", pk);
    // 16-lane groups give 8 slots per round on one CU.  With CUs to spare the packed round runs on 2 or 4 CUs per replica (16 / 32
    // slots per round, segment_packm_kernel): Mackey-Glass 4-10-1, 64 replicas needs 18.7 / 13.6 / 11.6 rounds per swap interval
    // with 8 / 16 / 32 slots (profiles/r03_window_sim.jsonl) and a packed round is shorter than the multi-CU speculative one (the
    // forward passes run beside the epochs).  groups_per_replica = 1, 2, 4 decides otherwise.
    int G = 1;
    const size_t pkm = pack_multi_lds_floats(Nall, h.IPY, h.PS, H, h.FWS, pack_slots(plan.pk_nred)) * sizeof(float);
    if (fits && pkm <= LDS_MAX && c.use_langevin && !c.shared_device && (sched == PTNN_SCHED_PACKED || c.schedule == PTNN_SCHED_AUTO) &&
        c.waves_per_replica == 0) {
        const int want = c.groups_per_replica;
        if (want == 2 || want == 4) G = want;                       // (8-lane groups: on request only -- 16 slots on one CU already)
        else if (want == 0 && plan.pk_nred == 4) { if (Rl * 4 <= h.num_cus) G = 4; else if (Rl * 2 <= h.num_cus) G = 2; }
    }
    const bool pays = (H <= 8) || G > 1 || Rl * 4 > h.num_cus;
    if (sched != PTNN_SCHED_PACKED &&
        !(c.schedule == PTNN_SCHED_AUTO && sched == PTNN_SCHED_SPECULATIVE && fits && pays && c.use_langevin && c.waves_per_replica == 0 &&
          (c.groups_per_replica == 0 || G > 1)))
        return 0;
    plan.kind = G > 1 ? SEG_PACKM : SEG_PACK;
    plan.groups = G;
    // eight waves (forward passes two to a SIMD) while every replica has a CU to itself, four beyond that; an explicit
    // waves_per_replica of 4 or 8 decides otherwise
    const int pkw = (c.waves_per_replica == 4 || c.waves_per_replica == 8) ? c.waves_per_replica : (Rl <= h.num_cus ? PK_WAVES : 4);
    plan.threads = (G > 1 ? PK_WAVES : pkw) * WAVE;
    plan.seg_lds = G > 1 ? pkm : pk;
    if (G > 1) {
        plan_exchange(h, G, plan);
        plan.xswap = swap_granule_bytes(h, 2 * h.PS + 8);         // in-launch swap rounds: state + cached gradient + flag
    }
    return 0;
}

// Speculative over work-groups.  Two waves on one SIMD slow each other ~1.65x (the SGD sweep is VALU-issue bound), so speculation
// depth comes from more CUs first: G work-groups of 4 waves (one per SIMD) per replica while R*G <= number of CUs, and 8 waves on a
// single CU otherwise.  Leaves the plan alone (the cooperative schedule) when the automatic choice finds no room in LDS.
int plan_speculative(const ptnn_handle& h, int Nall, LaunchPlan& plan) {
    const ptnn_config& c = h.cfg;
    const int Rl = c.n_replicas_local, nw = c.waves_per_replica;
    int G = 1;
    if (c.groups_per_replica > 0) G = c.groups_per_replica;
    else if (!c.shared_device) { while (G < 4 && Rl * (G * 2) <= h.num_cus) G *= 2; }
    if (G != 1 && G != 2 && G != 4 && G != 8) return fail(-1, "groups_per_replica must be 0 (auto), 1, 2, 4 or 8");
    auto lds = [&](int k) { return spec_lds_floats(Nall, h.IPY, h.PS, c.n_hidden, h.FWS, k, G) * sizeof(float); };
    int k = nw ? nw : (G > 1 ? 4 : 8);
    while (k > 1 && lds(k) > LDS_MAX) k >>= 1;
    if (nw && k != nw) {
        if (c.schedule == PTNN_SCHED_AUTO) k = 0;      // auto: fall back to the cooperative schedule
        else return fail(-3, "speculative schedule with %d waves needs more than 160 KiB of LDS", nw);
    }
    if (k * G > MAX_SLOTS) return fail(-1, "waves x groups must not exceed %d", MAX_SLOTS);
    if (k == 0 || lds(k) > LDS_MAX) return 0;
    plan.kind = SEG_SPEC; plan.threads = k * 64; plan.groups = G; plan.seg_lds = lds(k);
    if (G > 1) {
        // The work-groups of one replica wait for each other inside the kernel, so all Rl x G of them must be resident at once: ask
        // the runtime how many blocks of THIS kernel (its registers, this LDS size, this block size) fit on a CU instead of guessing,
        // and refuse the configuration otherwise (a non-resident partner would be a bounded spin and an error from ptnn_sync).  The
        // count is for a GPU this handle has to itself: other handles or processes on the same device take CUs this query does not see.
        const void* fn = reinterpret_cast<const void*>(h.shape->spec);
        if (int rc = raise_lds_limit(fn, plan.seg_lds)) return rc;
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, plan.threads, plan.seg_lds));
        plan.blocks_per_cu = per_cu;
        if ((long long)Rl * G > (long long)per_cu * h.num_cus)
            return fail(-3, "%d replicas x %d work-groups cannot all be resident: %d work-group(s) of %d threads with %zu B "
                            "of LDS fit on each of the %d CUs; use fewer groups_per_replica or the packed schedule",
                        Rl, G, per_cu, plan.threads, plan.seg_lds, h.num_cus);
        plan_exchange(h, MAX_SLOTS, plan);
    }
    return 0;
}

// Cooperative: one work-group per replica, the forward pass row-parallel over its waves
void plan_cooperative(const ptnn_handle& h, int Nall, int Npad, LaunchPlan& plan) {
    const ptnn_config& c = h.cfg;
    const int I = c.n_in, H = c.n_hidden, lg = c.use_langevin;
    plan.threads = c.waves_per_replica ? c.waves_per_replica * 64 : plan.model_threads;
    const size_t seg_lds = lds_floats(Nall, h.IPY, h.PS, H, h.FWS, lg != 0) * sizeof(float);
    plan.seg_lds = seg_lds;
    // a hidden layer that fills most of a 32-unit tile and at least three k-steps: forward pass on the matrix cores
    // (the VALU pass re-reads the weights from LDS with broadcast reads and is bound by the LDS pipe at this size)
    const size_t extra = (mfma_coop_lds_floats(I, c.n_out, H, Npad) + 4) * sizeof(float);
    if (!(H >= 24 && I >= 6 && seg_lds + extra <= LDS_MAX)) return;
    plan.fw_mfma = 1;
    plan.seg_lds = seg_lds + extra;
    // Split bf16 operands (ptnn_device.hpp, SplitK): the default where the matrix cores are used, unless the caller asked for
    // the exact fp32 instruction (forward_bf16 = 2: bit-identical to the VALU schedules) or the images do not fit.  They take
    // more LDS than the transposed fp32 image; a random-walk launch may give up the row-major data image for them (its only
    // readers left are the chain start and the SGD epochs of a Langevin launch, which therefore keeps it).
    if (h.shape->split_ch <= 0 || c.forward_bf16 == 2) return;
    const size_t with_xy = seg_lds + split_lds_bytes(h, Npad);
    const size_t without_xy = lds_floats(Nall, h.IPY, h.PS, H, h.FWS, lg != 0, false) * sizeof(float) + split_lds_bytes(h, Npad);
    if (with_xy <= LDS_MAX) { plan.fw_mfma = 2; plan.xy_global = false; plan.seg_lds = with_xy; }
    else if (!lg && without_xy <= LDS_MAX) { plan.fw_mfma = 2; plan.xy_global = true; plan.seg_lds = without_xy; }
}

// Prefetching tree: 2^D - 1 work-groups per replica, all of them resident (they wait for each other's records).  Explicit:
// groups_per_replica = 3, 7, 15 or 31 (0: deepest that fits); auto: deepest of 31 / 15 / 7 / 3 that fits (31 nodes: five steps per
// round; Iris 16 x 31 = 496 work-groups, two to a CU: 11.8 M against 11.4 M samples/s with 15), none -> the plan stays cooperative.
int plan_tree(const ptnn_handle& h, int Nall, int Npad, bool explicit_tree, LaunchPlan& plan) {
    const ptnn_config& c = h.cfg;
    const int I = c.n_in, H = c.n_hidden, Rl = c.n_replicas_local, want = c.groups_per_replica;
    if (explicit_tree && want != 0 && want != 3 && want != 7 && want != 15 && want != 31)
        return fail(-1, "tree schedule: groups_per_replica must be 0 (auto), 3, 7, 15 or 31");
    const int threads = c.waves_per_replica ? c.waves_per_replica * 64 : plan.model_threads;
    // same forward pass as the cooperative schedule would run (matrix cores or not): a deeper tree that has no room for the
    // transposed data image is not taken
    const size_t mfma_lds = (mfma_coop_lds_floats(I, c.n_out, H, Npad) + 4) * sizeof(float);
    const bool mfma = H >= 24 && I >= 6 && lds_floats(Nall, h.IPY, h.PS, H, h.FWS, false) * sizeof(float) + mfma_lds <= LDS_MAX;
    // the split-operand forward pass of the cooperative kernel (same arithmetic: the tree commits the cooperative chain bit for
    // bit either way), when its images fit next to the shallowest tree
    const bool split = mfma && h.shape->split_ch > 0 && c.forward_bf16 != 2 &&
                       tree_lds_floats(Nall, h.IPY, h.PS, H, h.FWS, 2, false, true) * sizeof(float) + split_lds_bytes(h, Npad) <= LDS_CEILING;
    const size_t extra = !mfma ? 0 : split ? split_lds_bytes(h, Npad) : mfma_lds;
    const void* fn = reinterpret_cast<const void*>(h.shape->tree);
    for (int G = (explicit_tree && want) ? want : TREE_MAX_NODES; G >= 3; G = (G - 1) / 2) {
        const int Dp = tree_depth(G);
        // two sets of tapes (the next round's drawn while the records travel) when they fit
        const bool ahead = tree_lds_floats(Nall, h.IPY, h.PS, H, h.FWS, Dp, true, mfma) * sizeof(float) + extra <= LDS_CEILING;
        const size_t lds = tree_lds_floats(Nall, h.IPY, h.PS, H, h.FWS, Dp, ahead, mfma) * sizeof(float) + extra;
        // (the runtime may refuse a dynamic-LDS ceiling just below 160 KiB: such a depth does not fit either)
        if (lds <= LDS_MAX && raise_lds_limit(fn, lds) == 0) {   // (raise_lds_limit clears a refused ceiling's error)
            int per_cu = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds));
            if ((long long)Rl * G <= (long long)per_cu * h.num_cus) {
                plan.kind = SEG_TREE; plan.threads = threads; plan.groups = G; plan.seg_lds = lds; plan.blocks_per_cu = per_cu;
                plan.fw_mfma = mfma ? (split ? 2 : 1) : 0; plan.xy_global = false; plan.tree_ahead = ahead;
                plan.xslots = (size_t)Rl * 2 * (TREE_MAX_NODES + 1) * TREE_REC * sizeof(unsigned long long);
                plan.xswap = swap_granule_bytes(h, h.PS);        // the in-launch swap rounds
                return 0;
            }
        }
        if (explicit_tree && want) break;
    }
    if (explicit_tree)
        return fail(-3, "tree schedule: %d replicas x %d work-groups of %d threads cannot all be resident on %d CUs (or need more than "
                        "160 KiB of LDS)", Rl, want ? want : 3, threads, h.num_cus);
    return 0;
}

// One launch per run needs every work-group of the grid resident at once (they meet at grid barriers) and room in LDS for the
// cascade of a swap round.  Taken by default where it is measured to pay: one work-group per replica (packed, cooperative,
// one-group wide: one barrier per round; Sunspot + 2.6 %, Ionosphere + 0.2 %); with several work-groups per replica a round needs a
// second rendezvous and the launch boundary it replaces is cheaper (Iris tree - 5 %, Mackey-Glass - 2 %,
// profiles/r03_persistent_ab.json).  $PTNN_PERSISTENT=0: never; =1: wherever resident.
int plan_persistent(const ptnn_handle& h, LaunchPlan& plan) {
    const ptnn_config& c = h.cfg;
    const char* e = std::getenv("PTNN_PERSISTENT");
    if ((e && e[0] == '0') || c.shared_device) return 0;     // grid barriers want every work-group resident: not on a shared GPU
    const bool forced = e && e[0] == '1';
    const int R = c.n_replicas_global;
    // The prefetching tree runs its swap rounds inside the launch by itself (segment_tree_body: the root groups exchange scalars and
    // state rows as granules, no grid barrier): the reference's cascade without label swapping, a ladder that is not sharded, and as
    // many replicas as the cascade has room for in the record area of LDS.  One launch per run then, unless $PTNN_PERSISTENT=0.
    const bool whole = c.swap_rule == 0 && !c.label_swap && plan.xswap > 0 && c.n_replicas_local == R;
    const bool tree_inside = plan.kind == SEG_TREE && whole && R <= TREE_PERSIST_MAX_R;
    // ... and so does the packed round over several CUs (segment_pack_body<MULTI>; the cascade's 3 R + 1 floats live in the slots' area)
    const bool packm_inside = plan.kind == SEG_PACKM && whole && (size_t)(3 * R + 1) <= (size_t)pack_slots(plan.pk_nred) * pack_slot_floats(h.PS);
    const bool own_rounds = tree_inside || packm_inside;
    if (plan.grid(1) > 1 && !own_rounds && !forced) return 0;
    // One barrier per round (G == 1) leaves the posted scalars single-buffered: a work-group that has left the barrier reads all R of
    // them into LDS at once (cascade_lds), and the next write to any of them comes a whole swap interval later, at the end of the
    // writer's next interval.  The invariant "no resident work-group falls a whole interval behind between leaving a barrier and its
    // next few loads" holds with orders of magnitude to spare for intervals of tens of microseconds; for intervals of a few MH steps
    // of a small net it is not worth relying on: those runs take one launch per interval (a kernel boundary orders everything).
    if (c.swap_interval < 8 && !own_rounds && !forced) return 0;
    // kernels compiled without the interval loop (ptnn_device.hpp: persistent_loop<false>)
    if (plan.kind == SEG_SPEC || (plan.kind == SEG_TREE && !tree_inside) || (plan.kind == SEG_PACKM && !packm_inside)) return 0;
    if (plan.kind == SEG_PACK && !(h.shape->loops & 2)) return 0;
    if (plan.kind == SEG_COOP && !(h.shape->loops & 1)) return 0;
    const size_t swap_lds = (size_t)(3 * R + 1) * sizeof(float);
    if (swap_lds > plan.seg_lds) {
        if (swap_lds > LDS_CEILING) return 0;
        plan.seg_lds = swap_lds;
    }
    const void* fn = reinterpret_cast<const void*>(segment_function(h.shape, plan.kind));
    if (int rc = raise_lds_limit(fn, plan.seg_lds)) return rc;
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, plan.threads, plan.seg_lds));
    plan.persistent = (long long)plan.grid(c.n_replicas_local) <= (long long)per_cu * h.num_cus;
    return 0;
}

// The launch plan of a handle for a data set of Nall rows: a function of the config, the data shape and the device ($PTNN_PERSISTENT
// aside).  Queries the runtime (occupancy, dynamic-LDS ceilings), never writes to the handle; 0 or the refusal.
int plan_launch(const ptnn_handle& h, int Nall, int Npad, LaunchPlan& plan) {
    const ptnn_config& c = h.cfg;
    plan = LaunchPlan{};
    if (c.n_hidden > WAVE) {
        if (int rc = plan_wide(h, plan)) return rc;
    } else {
        // LDS budget: the data set, the state vectors and the packed forward weights live in LDS for the whole launch
        plan.model_lds = lds_floats(Nall, h.IPY, h.PS, c.n_hidden, h.FWS) * sizeof(float);
        if (plan.model_lds > LDS_MAX)
            return fail(-3, "replica working set needs %zu B of LDS (> 160 KiB): data %d rows x %d floats, P = %d", plan.model_lds, Nall,
                        h.IPY, h.P);
        // schedule: speculative pays when MH acceptance is low (regression chains: 1-15 %) or the step is dominated by the
        // sequential SGD sweep; cooperative when one step's row-parallel forward pass is the bulk of the work
        int sched = c.schedule;
        if (sched == PTNN_SCHED_AUTO) sched = (c.task == PTNN_TASK_REG || c.use_langevin) ? PTNN_SCHED_SPECULATIVE : PTNN_SCHED_COOPERATIVE;
        if (sched != PTNN_SCHED_COOPERATIVE && sched != PTNN_SCHED_SPECULATIVE && sched != PTNN_SCHED_PACKED && sched != PTNN_SCHED_TREE)
            return fail(-1, "unknown schedule %d", sched);
        if (sched == PTNN_SCHED_TREE && (c.task != PTNN_TASK_CLS || c.use_langevin))
            return fail(-3, "the prefetching tree schedule is built for random-walk classification runs");
        plan.pk_nred = (c.n_hidden <= 8) ? 3 : 4;
        if (int rc = plan_packed(h, Nall, sched, plan)) return rc;
        if (plan.kind != SEG_COOP) sched = PTNN_SCHED_PACKED;
        const int nw = c.waves_per_replica;
        if (nw != 0 && nw != 1 && nw != 2 && nw != 4 && nw != 8) return fail(-1, "waves_per_replica must be 0 (auto), 1, 2, 4 or 8");
        int pow2 = 1;
        while (pow2 < (Nall + 63) / 64) pow2 <<= 1;
        plan.model_threads = std::min(pow2, 8) * 64;
        if (sched == PTNN_SCHED_SPECULATIVE) {
            if (int rc = plan_speculative(h, Nall, plan)) return rc;
            if (plan.kind == SEG_COOP) sched = PTNN_SCHED_COOPERATIVE;
        }
        if (sched == PTNN_SCHED_COOPERATIVE) plan_cooperative(h, Nall, Npad, plan);
        const bool auto_tree = sched == PTNN_SCHED_COOPERATIVE && c.schedule == PTNN_SCHED_AUTO && c.task == PTNN_TASK_CLS &&
                               !c.use_langevin && c.groups_per_replica == 0 && c.waves_per_replica == 0 && !c.shared_device;
        if (sched == PTNN_SCHED_TREE || auto_tree)
            if (int rc = plan_tree(h, Nall, Npad, sched == PTNN_SCHED_TREE, plan)) return rc;
    }
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(segment_function(h.shape, plan.kind)), plan.seg_lds)) return rc;
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(plan.wide() ? h.shape->model_wide : h.shape->model), plan.model_lds)) return rc;
    return plan_persistent(h, plan);
}

// Host images of a data set: row-major {x, y, d} rows (xy), transposed (xt), split into bf16 levels (xs: wide nets, else empty)
struct DataImages {
    int ntr = 0, nte = 0, Npad = 0;
    std::vector<float> xy, xt;
    std::vector<uint16_t> xs;
};

int pack_data(const ptnn_handle& h, const float* train, int ntr, const float* test, int nte, int ncols, DataImages& img) {
    const int I = h.cfg.n_in, IPY = h.IPY, Nall = ntr + nte;
    img.ntr = ntr; img.nte = nte;
    std::vector<float>& packed = img.xy;
    packed.assign((size_t)(Nall + 2) * IPY, 0.0f);                 // two zero rows: look-ahead of the SGD sweep
    for (int n = 0; n < Nall; ++n) {
        const float* row = (n < ntr) ? train + (size_t)n * ncols : test + (size_t)(n - ntr) * ncols;
        for (int c = 0; c <= I; ++c) packed[(size_t)n * IPY + c] = row[c];
        if (n > 0) {                                                 // see sgd_sweep: z[n] = zpart + lhd[n-1] * (1 + x[n].x[n-1])
            float d = 1.0f;
            for (int c = 0; c < I; ++c) d = std::fmaf(row[c], packed[(size_t)(n - 1) * IPY + c], d);
            packed[(size_t)n * IPY + I + 1] = d;
        }
        if (h.cfg.task == PTNN_TASK_CLS) {
            const float y = row[I];
            if (!(y >= 0.0f) || y >= (float)h.cfg.n_out || y != std::floor(y))
                return fail(-1, "class label %g in row %d is not an integer in [0, %d)", (double)y, n, h.cfg.n_out);
        }
    }
    // transposed image Xt[k][Npad] for the MFMA forward passes (rows = data rows are the lanes of the B operand)
    const int Npad = img.Npad = (Nall + 31) & ~31;
    img.xt.assign((size_t)I * Npad, 0.0f);
    for (int n = 0; n < Nall; ++n)
        for (int k = 0; k < I; ++k) img.xt[(size_t)k * Npad + n] = packed[(size_t)n * IPY + k];
    if (wide_split(h)) {
        // split-operand forward pass of the wide kernels: x = hi + mid + lo, three bf16 roundings (nearest even; x - hi and
        // x - hi - mid are exact in fp32), rows of 8 * CH bf16, k contiguous
        const int KBF = 8 * h.shape->split_ch;
        auto bf16 = [](float f) -> uint32_t { uint32_t u; std::memcpy(&u, &f, 4); return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16; };
        auto back = [](uint32_t b) -> float { const uint32_t u = b << 16; float f; std::memcpy(&f, &u, 4); return f; };
        img.xs.assign((size_t)3 * Npad * KBF, 0);
        for (int n = 0; n < Nall; ++n)
            for (int k = 0; k < I && k < KBF; ++k) {
                const float x = packed[(size_t)n * IPY + k];
                const uint32_t hi = bf16(x);
                const float r1 = x - back(hi);
                const uint32_t mid = bf16(r1);
                const float r2 = r1 - back(mid);
                const uint32_t lo = bf16(r2);
                img.xs[((size_t)0 * Npad + n) * KBF + k] = (uint16_t)hi;
                img.xs[((size_t)1 * Npad + n) * KBF + k] = (uint16_t)mid;
                img.xs[((size_t)2 * Npad + n) * KBF + k] = (uint16_t)lo;
            }
    }
    return 0;
}

// free *ptr, then allocate `bytes` (0: none) and fill them from the host (src) or with zeros (zero)
template <class T>
int replace_buffer(T*& ptr, size_t bytes, bool zero, const void* src = nullptr) {
    if (ptr) { HIP_TRY(hipFree(ptr)); ptr = nullptr; }
    if (bytes == 0) return 0;
    HIP_TRY(hipMalloc(&ptr, bytes));
    if (src) HIP_TRY(hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice));
    else if (zero) HIP_TRY(hipMemset(ptr, 0, bytes));
    return 0;
}

// Upload the images and allocate the plan's buffers; a failed allocation leaves the handle without data (it refuses to run)
int apply_plan(ptnn_handle* h, const DataImages& img, const LaunchPlan& plan) {
    h->have_data = false;
    if (int rc = replace_buffer(h->d_data, img.xy.size() * sizeof(float), false, img.xy.data())) return rc;
    if (int rc = replace_buffer(h->d_xt, img.xt.size() * sizeof(float), false, img.xt.data())) return rc;
    if (int rc = replace_buffer(h->d_xs, img.xs.size() * sizeof(uint16_t), false, img.xs.data())) return rc;
    if (int rc = replace_buffer(h->d_wide_scratch, plan.wide_scratch, false)) return rc;
    if (int rc = replace_buffer(h->d_xslots, plan.xslots, true)) return rc;
    if (int rc = replace_buffer(h->d_xw, plan.xw, true)) return rc;
    if (int rc = replace_buffer(h->d_xverdict, plan.xverdict, true)) return rc;
    if (int rc = replace_buffer(h->d_xswap, plan.xswap, true)) return rc;
    if (plan.xslots) h->epoch_base = 1;                 // fresh granules: tag 0 = never written
    h->Ntr = img.ntr; h->Nte = img.nte; h->Npad = img.Npad;
    h->plan = plan;
    h->have_data = true;
    return 0;
}

int check_ready(ptnn_handle* h) {
    if (!h) return fail(-1, "null handle");
    if (!h->have_data) return fail(-1, "ptnn_set_data has not been called");
    if (!h->have_state) return fail(-1, "ptnn_set_state has not been called");
    return 0;
}

}  // namespace

namespace {
// everything of ptnn_create that can fail after the handle exists: the caller destroys the handle on a non-zero return
int create_buffers(ptnn_handle* h, const ptnn_config* cfg, const Shape* sh, const hipDeviceProp_t& prop) {
    h->cfg = *cfg;
    h->shape = sh;
    h->num_cus = prop.multiProcessorCount;
    if (const char* ts = std::getenv("PTNN_TIMING_STRIDE")) h->timing_stride = std::atoi(ts);
    const int I = cfg->n_in, H = cfg->n_hidden, O = cfg->n_out;
    h->P = I * H + H * O + H + O;
    h->PS = round_up4(h->P + 1);
    h->PW = (h->P + 15) & ~15;                             // pos_w trace rows: whole 64-byte sectors
    h->IPY = round_up4(I + 2);                             // x[I], y, then 1 + x[n].x[n-1] for the pipelined SGD epoch
    h->FWS = round_up4(I + 1 + O);
    h->max_rounds = cfg->n_samples / cfg->swap_interval + 2;
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->cap = (cfg->trace_capacity > 0 && cfg->trace_capacity < cfg->n_samples) ? cfg->trace_capacity : cfg->n_samples;
    const size_t Rl = cfg->n_replicas_local, R = cfg->n_replicas_global, S = h->cap;
    HIP_TRY(hipMalloc(&h->d_state[0], Rl * h->PS * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_state[1], Rl * h->PS * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_rec_w, Rl * h->PS * sizeof(float)));
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(hipMalloc(&h->d_gd_w[b], Rl * h->PS * sizeof(float)));
        HIP_TRY(hipMalloc(&h->d_gd_valid[b], Rl * sizeof(int)));
    }
    HIP_TRY(hipMalloc(&h->d_st_f, Rl * SF_COUNT * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_st_i, Rl * SI_COUNT * sizeof(int)));
    HIP_TRY(hipMalloc(&h->d_temps, Rl * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_L_handoff, R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_L_final, R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_L_raw, R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_prior_post, R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_temps_global, R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_pos_w, Rl * S * h->PW * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_scal, Rl * S * TR_COUNT * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_src, R * sizeof(int)));
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(hipMalloc(&h->d_label[b], R * sizeof(int)));
        HIP_TRY(hipMalloc(&h->d_slot_of[b], R * sizeof(int)));
    }
    HIP_TRY(hipHostMalloc(&h->h_src, R * sizeof(int), hipHostMallocDefault));
    HIP_TRY(hipMalloc(&h->d_xchg, (size_t)R * xchg_row_floats(h->PS) * sizeof(float)));
    HIP_TRY(hipMemsetAsync(h->d_xchg, 0, (size_t)R * xchg_row_floats(h->PS) * sizeof(float), h->stream));
    HIP_TRY(hipMalloc(&h->d_src_log, (size_t)h->max_rounds * R * sizeof(int)));
    HIP_TRY(hipMalloc(&h->d_counters, 2 * sizeof(long long)));
    HIP_TRY(hipMalloc(&h->d_error, sizeof(int)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_stage), (Rl * h->P + Rl) * sizeof(float), hipHostMallocDefault));
    HIP_TRY(hipMalloc(&h->d_stage, (Rl * h->P + Rl) * sizeof(float)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_progress), 2 * sizeof(int), hipHostMallocDefault));
    h->h_progress[0] = h->h_progress[1] = 0;
    HIP_TRY(hipMalloc(&h->d_stamps, 160 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(h->d_stamps, 0, 160 * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_error, 0, sizeof(int), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_counters, 0, 2 * sizeof(long long), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_L_handoff, 0, R * sizeof(float), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_L_final, 0, R * sizeof(float), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_src_log, 0xff, (size_t)h->max_rounds * R * sizeof(int), h->stream));
    return 0;
}
}  // namespace

extern "C" {

int ptnn_abi_version(void) { return PTNN_ABI_VERSION; }
const char* ptnn_last_error(void) { return g_err.c_str(); }

int ptnn_supports(int task, int n_in, int n_hidden, int n_out) {
    return (find_shape(task, n_in, n_out) != nullptr && n_hidden >= 1 && n_hidden <= MAX_HIDDEN) ? 1 : 0;
}

int ptnn_create(const ptnn_config* cfg, ptnn_handle** out) {
    if (!cfg || !out) return fail(-1, "null argument");
    if (cfg->struct_bytes != (int32_t)sizeof(ptnn_config))
        return fail(-1, "ptnn_config size mismatch: caller %d, library %d", cfg->struct_bytes, (int)sizeof(ptnn_config));
    if (cfg->task != PTNN_TASK_REG && cfg->task != PTNN_TASK_CLS) return fail(-1, "unknown task %d", cfg->task);
    if (cfg->n_in < 1 || cfg->n_hidden < 1 || cfg->n_out < 1) return fail(-1, "bad topology");
    if (cfg->task == PTNN_TASK_REG && cfg->n_out != 1) return fail(-1, "regression needs n_out == 1");
    const Shape* sh = find_shape(cfg->task, cfg->n_in, cfg->n_out);
    if (!sh)
        return fail(-3, "no gfx950 kernel compiled for task=%d n_in=%d n_out=%d: add it to PTNN_SHAPES and rebuild",
                    cfg->task, cfg->n_in, cfg->n_out);
    if (cfg->n_hidden > MAX_HIDDEN)
        return fail(-3, "n_hidden=%d > %d: the SGD sweep holds one hidden unit per thread of one work-group", cfg->n_hidden, MAX_HIDDEN);
    if (cfg->n_replicas_local < 1 || cfg->n_replicas_global < 2 || cfg->first_global_replica < 0 ||
        cfg->first_global_replica + cfg->n_replicas_local > cfg->n_replicas_global)
        return fail(-1, "bad replica partition: local=%d global=%d first=%d", cfg->n_replicas_local,
                    cfg->n_replicas_global, cfg->first_global_replica);
    if (cfg->n_samples < 2) return fail(-1, "n_samples must be >= 2");
    if (cfg->swap_interval < 1) return fail(-1, "swap_interval must be >= 1 (the reference divides by it, REG:427)");
    if (cfg->swap_rule != 0 && cfg->swap_rule != 1) return fail(-1, "swap_rule must be 0 (reference cascade) or 1 (even/odd Metropolis)");
    if (cfg->label_swap != 0 && cfg->label_swap != 1) return fail(-1, "label_swap must be 0 or 1");
    if (cfg->shared_device != 0 && cfg->shared_device != 1) return fail(-1, "shared_device must be 0 or 1");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(-2, "device %d not present (%d devices)", cfg->device_id, ndev);
    HIP_TRY(hipSetDevice(cfg->device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(-2, "device %d is %s; libptnn is built for gfx950 only", cfg->device_id, prop.gcnArchName);

    if (cfg->trace_capacity < 0 || (cfg->trace_capacity > 0 && cfg->trace_capacity < 2))
        return fail(-1, "trace_capacity must be 0 (= n_samples) or >= 2");
    ptnn_handle* h = new ptnn_handle();
    if (int rc = create_buffers(h, cfg, sh, prop)) {       // frees whatever was allocated (stream included); g_err keeps the cause
        const std::string why = g_err;
        ptnn_destroy(h);
        g_err = why;
        return rc;
    }
    *out = h;
    return 0;
}

int ptnn_destroy(ptnn_handle* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device_id);
    if (h->stream && !h->comm.failed) (void)wait_stream(h);
    h->comm.release();                                       // a failed communicator is aborted: its kernels leave the stream
    if (h->comm.failed && h->stream) {
        // give the aborted collective a few seconds to drain; if the stream still does not empty, leak the handle rather than
        // block in hipFree for ever
        const double t0 = comm_clock();
        while (hipStreamQuery(h->stream) == hipErrorNotReady && comm_clock() - t0 < 5.0) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        if (hipStreamQuery(h->stream) == hipErrorNotReady) return fail(-7, "the stream of a failed communicator did not drain: handle leaked");
    }
    void* ptrs[] = {h->d_data, h->d_state[0], h->d_state[1], h->d_rec_w, h->d_gd_w[0], h->d_gd_w[1], h->d_gd_valid[0], h->d_gd_valid[1], h->d_st_f, h->d_st_i, h->d_temps,
                    h->d_L_handoff, h->d_L_final, h->d_L_raw, h->d_prior_post, h->d_temps_global, h->d_pos_w, h->d_scal, h->d_src, h->d_label[0], h->d_label[1], h->d_slot_of[0], h->d_slot_of[1], h->d_src_log, h->d_counters, h->d_error, h->d_xslots, h->d_xw, h->d_xverdict, h->d_xswap, h->d_stamps, h->d_wide_scratch, h->d_xt, h->d_xs, h->d_barrier};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_src) (void)hipHostFree(h->h_src);
    if (h->h_progress) (void)hipHostFree(h->h_progress);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->d_stage) (void)hipFree(h->d_stage);
    if (h->d_xchg) (void)hipFree(h->d_xchg);
    ladder_adapt_release(h);
    for (auto& ev : h->timing) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
    for (auto& ev : h->img_events) (void)hipEventDestroy(ev);
    if (h->h_img_pos) (void)hipHostFree(h->h_img_pos);
    if (h->h_img_rows) (void)hipHostFree(h->h_img_rows);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int ptnn_set_data(ptnn_handle* h, const float* train, int ntr, const float* test, int nte, int ncols) {
    if (!h || !train || !test) return fail(-1, "null argument");
    if (ncols < h->cfg.n_in + 1) return fail(-1, "data needs at least n_in + 1 = %d columns, got %d", h->cfg.n_in + 1, ncols);
    if (ntr < 1 || nte < 1) return fail(-1, "empty data set");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // a refused data set (-1, -3) leaves the handle as it was
    DataImages img;
    if (int rc = pack_data(*h, train, ntr, test, nte, ncols, img)) return rc;
    LaunchPlan plan;
    if (int rc = plan_launch(*h, ntr + nte, img.Npad, plan)) return rc;
    return apply_plan(h, img, plan);
}

int ptnn_set_state(ptnn_handle* h, const float* w0, const float* temperatures) {
    if (!h || !w0 || !temperatures) return fail(-1, "null argument");
    if (!h->have_data) return fail(-1, "call ptnn_set_data before ptnn_set_state");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = wait_stream(h)) return rc;                // a restart must not overtake a run still in flight (nor the staging buffer)
    if (h->copy_stream) {                                   // ... nor the trace rows of the previous run on their way to the host
        HIP_TRY(hipStreamSynchronize(h->copy_stream));
        for (auto& ev : h->img_events) (void)hipEventDestroy(ev);
        h->img_events.clear();
    }
    const int Rl = h->cfg.n_replicas_local, P = h->P;
    // one pinned staging buffer, one asynchronous copy, one kernel -- all on the handle's stream (a whole-run restart is part of
    // the benchmark's timed region).  Trace rows 1 .. S-1 need no clearing: every one of them is written by the MH step it
    // belongs to before ptnn_get_traces lets anybody read it.
    std::memcpy(h->h_stage, w0, (size_t)Rl * P * sizeof(float));
    std::memcpy(h->h_stage + (size_t)Rl * P, temperatures, (size_t)Rl * sizeof(float));
    HIP_TRY(hipMemcpyAsync(h->d_stage, h->h_stage, ((size_t)Rl * P + Rl) * sizeof(float), hipMemcpyHostToDevice, h->stream));
    ResetParams q{};
    q.R = h->cfg.n_replicas_global; q.Rl = Rl; q.P = P; q.PS = h->PS; q.PW = h->PW; q.cap = (size_t)h->cap;
    q.w0 = h->d_stage; q.temps_in = h->d_stage + (size_t)Rl * P;
    q.state0 = h->d_state[0]; q.state1 = h->d_state[1]; q.rec_w = h->d_rec_w; q.gd0 = h->d_gd_w[0]; q.gd1 = h->d_gd_w[1];
    q.st_f = h->d_st_f; q.temps = h->d_temps; q.pos_w = h->d_pos_w; q.scal = h->d_scal;
    q.gd_valid0 = h->d_gd_valid[0]; q.gd_valid1 = h->d_gd_valid[1]; q.st_i = h->d_st_i; q.error = h->d_error;
    q.label0 = h->d_label[0]; q.label1 = h->d_label[1]; q.slot0 = h->d_slot_of[0]; q.slot1 = h->d_slot_of[1];
    q.counters = h->d_counters;
    hipLaunchKernelGGL(chain_reset_kernel, dim3(Rl), dim3(256), 0, h->stream, q);
    HIP_TRY(hipGetLastError());
    if (h->have_adapt)
        if (int rc = ladder_adapt_reset(h)) return rc;
    h->flip = 0; h->cur = 0; h->rounds_done = 0; h->finalized = false; h->drained = 0; h->first_row = 0; h->lflip = 0;
    if (!h->comm.failed) { h->failed = false; h->failure.clear(); }   // a restart clears a failed run (a failed communicator stays failed)
    h->h_progress[0] = h->h_progress[1] = 0;
    h->have_state = true;
    return 0;
}

int ptnn_set_ladder(ptnn_handle* h, const float* temperatures_global) {
    if (!h || !temperatures_global) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (h->have_adapt) {                                     // a new ladder drops the adaptation: set it again
        if (int rc = wait_stream(h)) return rc;
        ladder_adapt_release(h);
    }
    HIP_TRY(hipMemcpy(h->d_temps_global, temperatures_global, h->cfg.n_replicas_global * sizeof(float), hipMemcpyHostToDevice));
    h->have_ladder = true;
    return 0;
}

int ptnn_set_ladder_adaptation(ptnn_handle* h, const ptnn_ladder_adapt_spec* spec) {
    if (!h || !spec) return fail(-1, "null argument");
    if (spec->struct_bytes != (int32_t)sizeof(ptnn_ladder_adapt_spec))
        return fail(-1, "ptnn_ladder_adapt_spec.struct_bytes = %d, this library expects %zu", spec->struct_bytes, sizeof(ptnn_ladder_adapt_spec));
    const ptnn_config& c = h->cfg;
    if (c.swap_rule != 1)
        return fail(-1, "ladder adaptation needs swap_rule 1: the reference's cascade (swap_rule 0) has no per-pair Metropolis "
                        "acceptance to equalise");
    if (!h->have_ladder) return fail(-1, "call ptnn_set_ladder before ptnn_set_ladder_adaptation");
    if (h->cur > 0 || h->rounds_done > 0) return fail(-1, "ptnn_set_ladder_adaptation after MH steps have run: restart the chains (ptnn_set_state) first");
    if (!(std::isfinite(spec->kappa0) && spec->kappa0 > 0.0) || !(std::isfinite(spec->t0) && spec->t0 > 0.0))
        return fail(-1, "kappa0 = %g and t0 = %g must be finite and > 0", spec->kappa0, spec->t0);
    const int R = c.n_replicas_global, S = c.n_samples, si = c.swap_interval;
    // the hand-off step of every swap round (Q10), as the runs find them
    std::vector<int> hand;
    for (int i = 0; i < S - 1; ++i)
        if (swap_trigger(c, i)) hand.push_back(i);
    const int A = spec->rounds;
    if (A < 0 || A > (int)hand.size())
        return fail(-1, "rounds = %d: the run has %zu swap rounds (n_samples %d, swap_interval %d)", A, hand.size(), S, si);
    if (A > 0 && c.pt_switch_step >= 0 && hand[A - 1] > c.pt_switch_step)
        return fail(-1, "rounds = %d: the last adapted round hands off after step %d, past the temperature switch at step %d "
                        "(every chain runs at T = 1 from there)", A, hand[A - 1], c.pt_switch_step);
    HIP_TRY(hipSetDevice(c.device_id));
    if (int rc = wait_stream(h)) return rc;
    std::vector<float> T(R);
    HIP_TRY(hipMemcpy(T.data(), h->d_temps_global, R * sizeof(float), hipMemcpyDeviceToHost));
    if (R < 2 || T[0] != 1.0f) return fail(-1, "the ladder must start at exactly 1 (T_0 = %g) and have at least two rungs", R ? (double)T[0] : 0.0);
    for (int k = 0; k + 1 < R; ++k)
        if (!(T[k + 1] > T[k]) || !std::isfinite(T[k + 1]))
            return fail(-1, "the ladder is not strictly increasing and finite: T_%d = %g, T_%d = %g", k, (double)T[k], k + 1, (double)T[k + 1]);
    if (int rc = ladder_adapt_alloc(h, *spec)) return rc;
    h->lad_T0 = T;
    h->lad_s0.resize(R - 1);
    for (int k = 0; k + 1 < R; ++k) h->lad_s0[k] = std::log((double)T[k + 1] - (double)T[k]);
    return ladder_adapt_reset(h);
}

int ptnn_get_ladder_adaptation(ptnn_handle* h, ptnn_ladder_adapt_spec* spec) {
    if (!h || !spec) return fail(-1, "null argument");
    if (!h->have_adapt) return 0;
    *spec = h->adapt;
    return 1;
}

int ptnn_get_ladder_history(ptnn_handle* h, float* ladders, float* accept, int32_t* rounds_recorded) {
    if (!h) return fail(-1, "null argument");
    if (!h->have_adapt) return fail(-1, "no ladder adaptation on this handle (ptnn_set_ladder_adaptation)");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    const size_t R = h->cfg.n_replicas_global;
    const int n = std::min(h->rounds_done, h->max_rounds);
    if (ladders) HIP_TRY(hipMemcpy(ladders, h->d_lad_hist, (size_t)(h->adapt.rounds + 1) * R * sizeof(float), hipMemcpyDeviceToHost));
    if (accept && n > 0) HIP_TRY(hipMemcpy(accept, h->d_lad_acc, (size_t)n * (R - 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (rounds_recorded) *rounds_recorded = n;
    return 0;
}

int ptnn_steps_done(ptnn_handle* h) { return h ? h->cur : -1; }

// what a swap round moves between GPUs for this handle: AUTO = gather while the gathered buffer stays small
static int resolved_xchg_mode(const ptnn_handle* h) {
    if (h->cfg.swap_rule == 1) return PTNN_XCHG_GATHER;       // the moved state brings likelihood and prior along: rows only
    if (h->comm.mode != PTNN_XCHG_AUTO) return h->comm.mode;
    const size_t gathered = (size_t)h->cfg.n_replicas_global * xchg_row_floats(h->PS) * sizeof(float);
    return gathered <= (size_t)4 << 20 ? PTNN_XCHG_GATHER : PTNN_XCHG_BOUNDARY;
}

// bookkeeping after the kernels of a round are queued: which buffers are current now
static void round_queued(ptnn_handle* h, bool phantom) {
    if (!phantom) {
        if (h->cfg.label_swap) h->lflip ^= 1;                // the maps changed, the chains stayed where they are
        else h->flip ^= 1;
    }
    h->rounds_done += 1;
}

// One swap round of a sharded ladder (the handle owns a block of it), everything queued on the handle's stream.
static int comm_swap_round(ptnn_handle* h, bool phantom) {
    Comm& c = h->comm;
    const int Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global;
    if (h->cfg.label_swap) {
        // zero payload: only the posted scalars travel (4 R bytes; the untempered ones too under swap_rule 1)
        if (!c.all_gather(phantom ? h->d_L_final : h->d_L_handoff, (size_t)Rl * sizeof(float), h->stream)) return fail(-7, "%s", c.err.c_str());
        if (h->cfg.swap_rule == 1 && !c.all_gather(h->d_L_raw, (size_t)Rl * sizeof(float), h->stream)) return fail(-7, "%s", c.err.c_str());
        if (int rc = launch_swap(h, phantom, phantom ? 2 : 3, false)) return rc;
        round_queued(h, phantom);
        c.rounds += 1;
        return 0;
    }
    if (resolved_xchg_mode(h) == PTNN_XCHG_GATHER) {
        if (int rc = launch_swap(h, phantom, -1, false)) return rc;                     // exchange rows of the local replicas
        if (!c.all_gather(h->d_xchg, (size_t)Rl * xchg_row_floats(h->PS) * sizeof(float), h->stream)) return fail(-7, "%s", c.err.c_str());
        if (int rc = launch_swap(h, phantom, phantom ? (2 | 4) : (3 | 4), false)) return rc;   // identical cascade + source rows
    } else {
        if (!c.all_gather(phantom ? h->d_L_final : h->d_L_handoff, (size_t)Rl * sizeof(float), h->stream)) return fail(-7, "%s", c.err.c_str());
        if (phantom) {                                                                  // counted, result discarded (Q13)
            if (int rc = launch_swap(h, true, 2, false)) return rc;
        } else {
            if (int rc = launch_swap(h, false, 0, true)) return rc;                     // cascade only: src[R]
            HIP_TRY(hipMemcpyAsync(h->h_src, h->d_src, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            if (int rc = wait_stream(h)) return rc;                                   // the one host wait of this mode
            route_rows(h->h_src, R, Rl, c.rank, h->route);
            float* cur = h->d_state[h->flip];
            float* next = h->d_state[h->flip ^ 1];
            const size_t PS = h->PS;
            if (!c.exchange_rows(h->route, PS * sizeof(float), h->stream,
                                 [&](int row) { return static_cast<void*>(cur + (size_t)row * PS); },
                                 [&](int row) { return static_cast<void*>(next + (size_t)row * PS); }))
                return fail(-7, "%s", c.err.c_str());
            if (int rc = launch_swap(h, false, 3, false)) return rc;                    // local moves (arrived rows stay), count, log
        }
    }
    round_queued(h, phantom);
    c.rounds += 1;
    return 0;
}

int ptnn_run(ptnn_handle* h, int n_steps) {
    if (int rc = check_ready(h)) return rc;
    // with a communicator attached the swap rounds go through it, also when it has a single rank (rehearsal of the path)
    const bool sharded = h->comm.kind != COMM_NONE;
    if (h->cfg.n_replicas_local != h->cfg.n_replicas_global && !sharded)
        return fail(-1, "this handle owns replicas %d..%d of %d: attach a communicator first (ptnn_comm_init / ptnn_comm_init_host), "
                        "or drive the pieces yourself with ptnn_run_segment + ptnn_swap_*", h->cfg.first_global_replica,
                    h->cfg.first_global_replica + h->cfg.n_replicas_local - 1, h->cfg.n_replicas_global);
    if ((h->cfg.swap_rule == 1 || h->cfg.label_swap) && !h->have_ladder)
        return fail(-1, "swap_rule 1 and label_swap need ptnn_set_ladder (all temperatures)");
    const int S = h->cfg.n_samples;
    const int last = S - 1;                                  // steps are i = 0 .. S-2
    int end = (n_steps < 0) ? last : std::min(last, h->cur + n_steps);
    if (h->cap < S && end - h->drained > h->cap - 1)
        return fail(-6, "trace ring of %d rows would overflow: rows from %d on have not been fetched; call ptnn_get_traces "
                        "first or run fewer steps", h->cap, h->drained + 1);
    if (h->plan.persistent && !sharded && h->cur < end) {
        // every work-group of the grid is resident: ONE launch runs all the intervals up to `end`, the swap rounds between them
        // inside the kernel (persistent_loop in ptnn_device.hpp); what is left to do here is the bookkeeping of those rounds
        int n_ho = 0;
        for (int c = h->cur; c < end;) {
            int seg_end = c;
            while (seg_end < end && !swap_trigger(h->cfg, seg_end)) ++seg_end;
            if (seg_end >= end) break;
            ++n_ho;
            c = seg_end + 1;
        }
        if (int rc = launch_segment(h, h->cur, end, true)) return rc;
        h->cur = end;
        for (int k = 0; k < n_ho; ++k) round_queued(h, false);
    }
    while (h->cur < end) {
        int seg_end = h->cur;
        while (seg_end < end && !swap_trigger(h->cfg, seg_end)) ++seg_end;
        const bool handoff = seg_end < end;                  // step seg_end triggers a hand-off
        const int stop = handoff ? seg_end + 1 : end;
        const bool phantom_next = !handoff && stop == last && !h->finalized && h->cfg.swap_rule == 0 && S / h->cfg.swap_interval > h->rounds_done;
        if (int rc = launch_segment(h, h->cur, stop, false, sharded && (handoff || phantom_next))) return rc;
        h->cur = stop;
        if (handoff) {
            if (sharded) {
                if (int rc = comm_swap_round(h, false)) return rc;
            } else {
                if (int rc = launch_swap(h, false, 3, false)) return rc;
                round_queued(h, false);
            }
        }
    }
    if (h->cur == last && !h->finalized) {
        // Q13: the parent loops int(S/si) rounds; a round beyond the replicas' hand-offs consumes the end-of-chain
        // vectors, is counted in swap_perc and its result is discarded
        if (h->cfg.swap_rule == 0 && S / h->cfg.swap_interval > h->rounds_done) {
            if (sharded) {
                if (int rc = comm_swap_round(h, true)) return rc;
            } else {
                if (int rc = launch_swap(h, true, 2, false)) return rc;
                h->rounds_done += 1;
            }
        }
        h->finalized = true;
    }
    return 0;
}

// ---- communicators of the sharded ladder ----
static int comm_check_partition(ptnn_handle* h, int rank, int nranks) {
    if (!h) return fail(-1, "null handle");
    if (h->comm.kind != COMM_NONE) return fail(-1, "this handle already has a communicator");
    const int Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global;
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(-1, "bad rank %d of %d", rank, nranks);
    if (Rl * nranks != R || h->cfg.first_global_replica != rank * Rl)
        return fail(-1, "the ladder must be cut into equal contiguous blocks: rank %d of %d owns replicas %d..%d of %d, expected "
                        "first_global_replica == rank * n_replicas_local and n_replicas_local * nranks == n_replicas_global",
                    rank, nranks, h->cfg.first_global_replica, h->cfg.first_global_replica + Rl - 1, R);
    return 0;
}

int ptnn_comm_unique_id(void* id_out, int nbytes) {
    if (!id_out || nbytes < (int)sizeof(ncclUniqueId)) return fail(-1, "the unique id needs a buffer of %d bytes", (int)sizeof(ncclUniqueId));
    // fault injection for the fall-back tests ($PTNN_COMM_FAULT=ncclGetUniqueId): fails before RCCL is loaded
    if (const char* f = std::getenv("PTNN_COMM_FAULT"))
        if (std::strstr(f, "ncclGetUniqueId")) return fail(-7, "ncclGetUniqueId failed: injected by $PTNN_COMM_FAULT");
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (!api) return fail(-7, "cannot load RCCL: %s", why.c_str());
    // static storage: the helper thread may outlive this call when the stage is abandoned
    static ncclUniqueId id;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    comm_stage("ncclGetUniqueId");
    int r = 0;
    if (!run_bounded([api]() -> int { return (int)api->GetUniqueId(&id); }, comm_timeout_s(), &r))
        return fail(-7, "ncclGetUniqueId did not return within %d s (it opens the bootstrap listener: NCCL_SOCKET_IFNAME=%s)",
                    (int)comm_timeout_s(), std::getenv("NCCL_SOCKET_IFNAME") ? std::getenv("NCCL_SOCKET_IFNAME") : "unset");
    if (r != (int)ncclSuccess) return fail(-7, "ncclGetUniqueId failed: %s", api->GetErrorString((ncclResult_t)r));
    comm_stage("ncclGetUniqueId done");
    std::memcpy(id_out, &id, sizeof id);
    return (int)sizeof id;
}

int ptnn_comm_init(ptnn_handle* h, const void* unique_id, int nbytes, int rank, int nranks) {
    if (int rc = comm_check_partition(h, rank, nranks)) return rc;
    if (!unique_id || nbytes != (int)sizeof(ncclUniqueId)) return fail(-1, "the unique id must be the %d bytes ptnn_comm_unique_id wrote", (int)sizeof(ncclUniqueId));
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (!api) return fail(-7, "cannot load RCCL: %s", why.c_str());
    // fault injection for the fall-back tests ($PTNN_COMM_FAULT=ncclCommInitRank): fails where a refused bring-up would, RCCL not called
    if (const char* f = std::getenv("PTNN_COMM_FAULT"))
        if (std::strstr(f, "ncclCommInitRank"))
            return fail(-7, "ncclCommInitRank(rank %d of %d, device %d) failed: injected by $PTNN_COMM_FAULT", rank, nranks, h->cfg.device_id);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // ncclCommInitRank is a collective: it returns when all nranks have joined.  A peer that never does (it failed before, or was
    // never started) would block this thread for ever, so the call runs on a helper that is abandoned after comm_timeout_s().
    struct Job { ncclUniqueId id; ncclComm_t comm = nullptr; };
    auto job = std::make_shared<Job>();
    std::memcpy(&job->id, unique_id, sizeof job->id);
    const int dev = h->cfg.device_id;
    comm_stage("ncclCommInitRank(rank %d of %d, device %d)", rank, nranks, dev);
    int r = 0;
    const bool finished = run_bounded([api, job, dev, rank, nranks]() -> int {
        if (hipSetDevice(dev) != hipSuccess) return (int)ncclUnhandledCudaError;
        return (int)api->CommInitRank(&job->comm, nranks, job->id, rank);
    }, comm_timeout_s(), &r);
    if (!finished)
        return fail(-7, "ncclCommInitRank(rank %d of %d, device %d) did not return within %d s: a rank never joined, or the bring-up "
                        "stalled ($PTNN_COMM_TRACE=1 and NCCL_DEBUG=INFO show where)", rank, nranks, dev, (int)comm_timeout_s());
    if (r != (int)ncclSuccess) return fail(-7, "ncclCommInitRank(rank %d of %d, device %d) failed: %s", rank, nranks, dev, api->GetErrorString((ncclResult_t)r));
    comm_stage("ncclCommInitRank done (rank %d of %d)", rank, nranks);
    h->comm.api = api; h->comm.nccl = job->comm; h->comm.rank = rank; h->comm.nranks = nranks; h->comm.kind = COMM_RCCL;
    return 0;
}

// One bounded round trip of RCCL among `devices` from THIS process: unique id, one ncclCommInitRank per device (a thread each),
// a 4-byte all-gather, destroy.  Meant to be run in a fresh CHILD process before the long-lived one touches RCCL (Python:
// distributed.rccl_probe): a bring-up that stalls or fails is then the child's, which is killed -- an RCCL left half
// initialised in the caller's own process (a unique id that no ncclCommInitRank follows, helpers abandoned inside
// ncclCommInitRank) can keep that process from exiting.  Honours $PTNN_COMM_FAULT like the real bring-up.
int ptnn_comm_probe(const int32_t* devices, int n, double* seconds) {
    if (!devices || n < 1 || n > 64) return fail(-1, "bad argument");
    const double t0 = comm_clock();
    const char* fault = std::getenv("PTNN_COMM_FAULT");
    if (fault && std::strstr(fault, "ncclGetUniqueId")) return fail(-7, "ncclGetUniqueId failed: injected by $PTNN_COMM_FAULT");
    char id[sizeof(ncclUniqueId)];
    if (int rc = ptnn_comm_unique_id(id, (int)sizeof id); rc < 0) return rc;
    if (fault && std::strstr(fault, "ncclCommInitRank")) return fail(-7, "ncclCommInitRank failed: injected by $PTNN_COMM_FAULT");
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (devices[a] == devices[b]) return fail(-1, "RCCL needs one distinct device per rank (device %d appears twice)", devices[a]);
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (!api) return fail(-7, "cannot load RCCL: %s", why.c_str());
    struct Shared { ncclUniqueId id; std::vector<int> rc; std::vector<std::string> msg; };
    auto sh = std::make_shared<Shared>();
    std::memcpy(&sh->id, id, sizeof sh->id);
    sh->rc.assign((size_t)n, -1); sh->msg.resize((size_t)n);
    std::vector<int> devs(devices, devices + n);
    comm_stage("probe: ncclCommInitRank x %d + one all-gather", n);
    int r = 0;
    const bool finished = run_bounded([api, sh, devs, n]() -> int {
        std::vector<std::thread> th;
        for (int k = 0; k < n; ++k)
            th.emplace_back([api, sh, devs, n, k]() {
                auto bad = [&](const char* what, const char* detail) { sh->msg[(size_t)k] = std::string(what) + ": " + detail; sh->rc[(size_t)k] = 1; };
                if (hipSetDevice(devs[(size_t)k]) != hipSuccess) return bad("hipSetDevice", "failed");
                ncclComm_t comm = nullptr;
                ncclResult_t e = api->CommInitRank(&comm, n, sh->id, k);
                if (e != ncclSuccess) return bad("ncclCommInitRank", api->GetErrorString(e));
                hipStream_t st = nullptr;
                int32_t* buf = nullptr;
                bool ok = hipStreamCreate(&st) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&buf), sizeof(int32_t) * (size_t)n) == hipSuccess;
                const int32_t mine = 1000 + k;
                ok = ok && hipMemcpyAsync(buf + k, &mine, sizeof mine, hipMemcpyHostToDevice, st) == hipSuccess;
                if (ok) {
                    e = api->AllGather(buf + k, buf, sizeof(int32_t), ncclChar, comm, st);
                    std::vector<int32_t> got((size_t)n, 0);
                    ok = e == ncclSuccess && hipMemcpyAsync(got.data(), buf, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st) == hipSuccess &&
                         hipStreamSynchronize(st) == hipSuccess;
                    for (int j = 0; ok && j < n; ++j) ok = got[(size_t)j] == 1000 + j;
                    if (!ok) bad("ncclAllGather", e == ncclSuccess ? "wrong or missing data" : api->GetErrorString(e));
                } else bad("hip", "stream / buffer set-up failed");
                if (buf) (void)hipFree(buf);
                if (st) (void)hipStreamDestroy(st);
                (void)api->CommDestroy(comm);
                if (ok) sh->rc[(size_t)k] = 0;
            });
        for (auto& t : th) t.join();
        for (int k = 0; k < n; ++k) if (sh->rc[(size_t)k] != 0) return 1 + k;
        return 0;
    }, comm_timeout_s(), &r);
    if (seconds) *seconds = comm_clock() - t0;
    if (!finished) return fail(-7, "the RCCL probe over %d devices did not finish within %d s (last stage: %s)", n, (int)comm_timeout_s(), comm_last_stage().c_str());
    if (r != 0) return fail(-7, "the RCCL probe failed on rank %d: %s", r - 1, sh->msg[(size_t)(r - 1)].c_str());
    comm_stage("probe done");
    return 0;
}

int ptnn_comm_info(ptnn_handle* h, int32_t* transport, int32_t* rank, int32_t* nranks, int32_t* device) {
    if (!h) return fail(-1, "null handle");
    if (transport) *transport = h->comm.kind;
    if (rank) *rank = h->comm.kind == COMM_NONE ? 0 : h->comm.rank;
    if (device) *device = h->cfg.device_id;
    if (nranks) {
        *nranks = h->comm.kind == COMM_NONE ? 1 : h->comm.nranks;
        if (h->comm.kind == COMM_RCCL && h->comm.api && h->comm.api->CommCount && h->comm.nccl) {
            int c = 0;                                         // what the communicator itself says, not what the caller passed in
            if (h->comm.api->CommCount(h->comm.nccl, &c) != ncclSuccess) return fail(-7, "ncclCommCount failed");
            *nranks = c;
        }
    }
    return 0;
}

int ptnn_comm_last_stage(char* buf, int nbytes) {
    if (!buf || nbytes < 1) return fail(-1, "bad argument");
    const std::string s = comm_last_stage();
    std::snprintf(buf, (size_t)nbytes, "%s", s.c_str());
    return (int)std::min<size_t>(s.size(), (size_t)nbytes - 1);
}

int ptnn_comm_init_host(ptnn_handle* h, int rank, int nranks, ptnn_all_gather_fn all_gather, ptnn_send_recv_fn send_recv, void* ctx) {
    if (int rc = comm_check_partition(h, rank, nranks)) return rc;
    if (!all_gather || !send_recv) return fail(-1, "null callback");
    h->comm.h_all_gather = all_gather; h->comm.h_send_recv = send_recv; h->comm.h_ctx = ctx;
    h->comm.rank = rank; h->comm.nranks = nranks; h->comm.kind = COMM_HOST;
    return 0;
}

int ptnn_comm_set_mode(ptnn_handle* h, int mode) {
    if (!h) return fail(-1, "null handle");
    if (mode != PTNN_XCHG_AUTO && mode != PTNN_XCHG_GATHER && mode != PTNN_XCHG_BOUNDARY) return fail(-1, "unknown exchange mode %d", mode);
    if (mode == PTNN_XCHG_BOUNDARY && h->cfg.swap_rule != 0)
        return fail(-3, "the boundary exchange implements the reference's cascade (swap_rule 0) only: use the gathered exchange");
    h->comm.mode = mode;
    return 0;
}

int ptnn_comm_stats(ptnn_handle* h, int64_t* bytes_sent, int64_t* bytes_received, int64_t* rounds, int32_t* mode) {
    if (!h) return fail(-1, "null handle");
    if (bytes_sent) *bytes_sent = h->comm.bytes_sent;
    if (bytes_received) *bytes_received = h->comm.bytes_received;
    if (rounds) *rounds = h->comm.rounds;
    if (mode) *mode = h->comm.kind == COMM_NONE ? 0 : resolved_xchg_mode(h);
    return 0;
}

int ptnn_comm_finalize(ptnn_handle* h) {
    if (!h) return fail(-1, "null handle");
    (void)hipSetDevice(h->cfg.device_id);
    int rc = 0;
    if (h->stream && !h->comm.failed) rc = wait_stream(h);
    h->comm.release();
    return rc;
}

int ptnn_route(const int32_t* src, int n_global, int n_local, int rank, int32_t* msg, int max_msgs) {
    if (!src || !msg || n_local < 1 || n_global < n_local || n_global % n_local != 0 || rank < 0 || rank >= n_global / n_local)
        return fail(-1, "bad argument");
    for (int k = 0; k < n_global; ++k)
        if (src[k] < 0 || src[k] >= n_global) return fail(-1, "src[%d] = %d is not a slot", k, src[k]);
    std::vector<RowMsg> r;
    route_rows(src, n_global, n_local, rank, r);
    if ((int)r.size() > max_msgs) return fail(-1, "%d messages, room for %d", (int)r.size(), max_msgs);
    for (size_t m = 0; m < r.size(); ++m) {
        msg[4 * m] = r[m].is_send; msg[4 * m + 1] = r[m].peer; msg[4 * m + 2] = r[m].local_row; msg[4 * m + 3] = r[m].global_dst;
    }
    return (int)r.size();
}

int ptnn_sync(ptnn_handle* h) {
    if (!h) return fail(-1, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    collect_timing(h);
    return 0;
}

int ptnn_run_segment(ptnn_handle* h, int* handoff) {
    if (int rc = check_ready(h)) return rc;
    if (!handoff) return fail(-1, "null argument");
    const int S = h->cfg.n_samples, last = S - 1;
    *handoff = 0;
    if (h->cur < last) {
        int seg_end = h->cur;
        while (seg_end < last && !swap_trigger(h->cfg, seg_end)) ++seg_end;
        const bool ho = seg_end < last;
        const int stop = ho ? seg_end + 1 : last;
        if (h->cap < S && stop - h->drained > h->cap - 1)
            return fail(-6, "trace ring of %d rows would overflow: fetch rows from %d on with ptnn_get_traces first", h->cap,
                        h->drained + 1);
        if (int rc = launch_segment(h, h->cur, stop)) return rc;
        h->cur = stop;
        if (ho) { *handoff = 1; return 0; }
    }
    if (h->cur == last && !h->finalized) {
        h->finalized = true;
        if (h->cfg.swap_rule == 0 && S / h->cfg.swap_interval > h->rounds_done) *handoff = 2;   // no phantom round in rule 1
    }
    return 0;
}

int ptnn_swap_L_ptr(ptnn_handle* h, int phantom, void** dev_ptr) {
    if (!h || !dev_ptr) return fail(-1, "null argument");
    *dev_ptr = phantom ? h->d_L_final : h->d_L_handoff;
    return 0;
}

int ptnn_swap_set_L(ptnn_handle* h, int phantom, const float* L_host) {
    if (!h || !L_host) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = wait_stream(h)) return rc;
    HIP_TRY(hipMemcpy(phantom ? h->d_L_final : h->d_L_handoff, L_host, h->cfg.n_replicas_global * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int ptnn_swap_cascade(ptnn_handle* h, int phantom, int32_t* src_host) {
    if (!h || !src_host) return fail(-1, "null argument");
    if (h->cfg.swap_rule != 0)
        return fail(-3, "the point-to-point exchange implements the reference's cascade (swap_rule 0) only: use the gathered mode");
    if (int rc = launch_swap(h, phantom != 0, 0, true)) return rc;
    const size_t bytes = h->cfg.n_replicas_global * sizeof(int);
    HIP_TRY(hipMemcpyAsync(h->h_src, h->d_src, bytes, hipMemcpyDeviceToHost, h->stream));   // pinned: no staging copy
    if (int rc = wait_stream(h)) return rc;
    std::memcpy(src_host, h->h_src, bytes);
    return 0;
}

int ptnn_state_row_floats(ptnn_handle* h) { return h ? h->PS : -1; }

int ptnn_stream(ptnn_handle* h, void** hip_stream) {
    if (!h || !hip_stream) return fail(-1, "null argument");
    *hip_stream = reinterpret_cast<void*>(h->stream);
    return 0;
}

int ptnn_swap_row_ptr(ptnn_handle* h, int local_replica, void** cur_row, void** next_row) {
    if (!h) return fail(-1, "null handle");
    if (local_replica < 0 || local_replica >= h->cfg.n_replicas_local) return fail(-1, "replica %d out of range", local_replica);
    if (cur_row) *cur_row = h->d_state[h->flip] + (size_t)local_replica * h->PS;
    if (next_row) *next_row = h->d_state[h->flip ^ 1] + (size_t)local_replica * h->PS;
    return 0;
}

int ptnn_swap_apply(ptnn_handle* h, const int32_t* src_host, int phantom) {
    if (int rc = check_ready(h)) return rc;
    if (h->cfg.label_swap) return fail(-3, "label swapping moves no rows: drive it with ptnn_run");
    (void)src_host;   // the device recomputes the identical cascade; the host copy only routed the remote rows
    if (int rc = launch_swap(h, phantom != 0, phantom ? 2 : 3, false)) return rc;
    if (!phantom) h->flip ^= 1;
    h->rounds_done += 1;
    return 0;
}

int ptnn_xchg_ptr(ptnn_handle* h, void** base, int* row_floats) {
    if (!h || !base || !row_floats) return fail(-1, "null argument");
    *base = h->d_xchg;
    *row_floats = xchg_row_floats(h->PS);
    return 0;
}

int ptnn_swap_pack(ptnn_handle* h, int phantom) {
    if (int rc = check_ready(h)) return rc;
    if (h->cfg.label_swap) return fail(-3, "label swapping moves no rows: drive it with ptnn_run");
    if (h->cfg.swap_rule == 1 && !h->have_ladder) return fail(-1, "swap_rule 1 needs ptnn_set_ladder (all temperatures)");
    return launch_swap(h, phantom != 0, -1, false);
}

int ptnn_swap_apply_gathered(ptnn_handle* h, int phantom) {
    if (int rc = check_ready(h)) return rc;
    if (h->cfg.label_swap) return fail(-3, "label swapping moves no rows: drive it with ptnn_run");
    if (int rc = launch_swap(h, phantom != 0, phantom ? (2 | 4) : (3 | 4), false)) return rc;
    if (!phantom) h->flip ^= 1;
    h->rounds_done += 1;
    return 0;
}

int ptnn_get_traces(ptnn_handle* h, int step0, int nsteps, float* pos_w, float* likeh, float* rmse_train,
                    float* rmse_test, float* acc_train, float* acc_test, int32_t* accept_count) {
    if (int rc = check_ready(h)) return rc;
    const int S = h->cfg.n_samples, Rl = h->cfg.n_replicas_local, P = h->P, cap = h->cap;
    if (step0 < 0 || nsteps < 0 || step0 + nsteps > S) return fail(-1, "trace range [%d, %d) outside [0, %d)", step0, step0 + nsteps, S);
    if (nsteps == 0) return 0;
    if (step0 + nsteps > h->cur + 1) return fail(-1, "rows up to %d requested but only %d MH steps have been queued", step0 + nsteps - 1, h->cur);
    if (step0 < h->first_row) return fail(-1, "rows below %d were produced before the checkpoint these chains were restored from", h->first_row);
    if (step0 < h->cur + 1 - cap) return fail(-1, "row %d has already been overwritten in the trace ring (capacity %d, %d steps done)", step0, cap, h->cur);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    collect_timing(h);
    // the range may wrap around the ring: at most two contiguous pieces
    auto copy2d = [&](void* dst, const void* src_base, size_t elem_bytes, size_t per_step) -> hipError_t {
        if (!dst) return hipSuccess;
        const size_t dpitch = (size_t)nsteps * per_step * elem_bytes;
        const size_t spitch = (size_t)cap * per_step * elem_bytes;
        int done = 0;
        while (done < nsteps) {
            const int slot = (step0 + done) % cap;
            const int n = std::min(nsteps - done, cap - slot);
            const size_t width = (size_t)n * per_step * elem_bytes;
            const char* src = static_cast<const char*>(src_base) + (size_t)slot * per_step * elem_bytes;
            char* d = static_cast<char*>(dst) + (size_t)done * per_step * elem_bytes;
            hipError_t e = hipMemcpy2D(d, dpitch, src, spitch, width, Rl, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return e;
            done += n;
        }
        return hipSuccess;
    };
    std::vector<float> rows;
    const bool want_scalars = likeh || rmse_train || rmse_test || acc_train || acc_test || accept_count;
    if (want_scalars || (pos_w && h->plan.compact)) {
        // the scalars of a step sit in one 32-byte row on the device (one sector per step instead of seven); the per-file
        // arrays of the reference's layout (REG:454-481) are split out below
        rows.resize((size_t)Rl * nsteps * TR_COUNT);
        HIP_TRY(copy2d(rows.data(), h->d_scal, sizeof(float), TR_COUNT));
    }
    if (pos_w && h->plan.compact) {
        // compact traces (wide nets, every row resident): a rejected step wrote no pos_w row, only the index of the row it
        // repeats (pos_w[i+1] = pos_w[i], REG:417).  Fetch every distinct source row once and fill the repeats in on the host.
        const size_t PW = h->PW;
        for (int r = 0; r < Rl; ++r) {
            int prev = -1;
            for (int t = 0; t < nsteps; ++t) {
                int32_t src;
                std::memcpy(&src, &rows[((size_t)r * nsteps + t) * TR_COUNT + TR_SRC], sizeof src);
                if (src < 0 || src > step0 + t || src < h->first_row - 1)
                    return fail(-2, "trace row %d of replica %d refers to row %d (internal error)", step0 + t, r, src);
                float* dst = pos_w + ((size_t)r * nsteps + t) * P;
                if (t > 0 && src == prev) std::memcpy(dst, dst - P, (size_t)P * sizeof(float));
                else HIP_TRY(hipMemcpy(dst, h->d_pos_w + ((size_t)r * cap + (size_t)(src % cap)) * PW, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
                prev = src;
            }
        }
    } else if (pos_w) {
        // device rows are padded to PW floats (whole sectors); the caller's array is dense: one strided copy per replica
        // and ring piece
        const size_t PW = h->PW;
        for (int r = 0; r < Rl; ++r) {
            int done = 0;
            while (done < nsteps) {
                const int slot = (step0 + done) % cap;
                const int n = std::min(nsteps - done, cap - slot);
                HIP_TRY(hipMemcpy2D(pos_w + ((size_t)r * nsteps + done) * P, (size_t)P * sizeof(float),
                                    h->d_pos_w + ((size_t)r * cap + slot) * PW, PW * sizeof(float), (size_t)P * sizeof(float), n,
                                    hipMemcpyDeviceToHost));
                done += n;
            }
        }
    }
    if (want_scalars) {
        float* outs[5] = {likeh, rmse_train, rmse_test, acc_train, acc_test};
        const int cols[5] = {TR_LIKEH, TR_RMSE_TR, TR_RMSE_TE, TR_ACC_TR, TR_ACC_TE};
        const size_t n = (size_t)Rl * nsteps;
        for (int c = 0; c < 5; ++c)
            if (outs[c])
                for (size_t k = 0; k < n; ++k) outs[c][k] = rows[k * TR_COUNT + cols[c]];
        // a regression has no accuracy (acc_train[i+1] = 0 on every step, REG:403): its TR_ACC_TR slot records eta (ptnn_device.hpp:
        // finish_eval<TASK, true>; ptnn_get_trace_rows shows it), the array of the reference's layout is zeros
        if (acc_train && h->cfg.task == PTNN_TASK_REG) std::fill(acc_train, acc_train + n, 0.0f);
        if (accept_count)
            for (size_t k = 0; k < n; ++k) std::memcpy(&accept_count[k], &rows[k * TR_COUNT + TR_ACCEPT], sizeof(int32_t));
    }
    h->drained = std::max(h->drained, step0 + nsteps - 1);
    return 0;
}

int ptnn_get_trace_rows(ptnn_handle* h, int step0, int nsteps, float* rows) {
    if (int rc = check_ready(h)) return rc;
    if (!rows) return fail(-1, "null argument");
    const int S = h->cfg.n_samples, Rl = h->cfg.n_replicas_local, cap = h->cap;
    if (step0 < 0 || nsteps < 1 || step0 + nsteps > S) return fail(-1, "trace range [%d, %d) outside [0, %d)", step0, step0 + nsteps, S);
    if (step0 + nsteps > h->cur + 1) return fail(-1, "rows up to %d requested but only %d MH steps have been queued", step0 + nsteps - 1, h->cur);
    if (step0 < h->first_row || step0 < h->cur + 1 - cap) return fail(-1, "row %d is no longer (or was never) on this device", step0);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    const size_t rowb = TR_COUNT * sizeof(float);
    int done = 0;
    while (done < nsteps) {                                  // the range may wrap around the ring
        const int slot = (step0 + done) % cap;
        const int n = std::min(nsteps - done, cap - slot);
        HIP_TRY(hipMemcpy2D(reinterpret_cast<char*>(rows) + (size_t)done * rowb, (size_t)nsteps * rowb,
                            reinterpret_cast<const char*>(h->d_scal) + (size_t)slot * rowb, (size_t)cap * rowb, (size_t)n * rowb, Rl,
                            hipMemcpyDeviceToHost));
        done += n;
    }
    return 0;
}

// ---- trace images: the download of the trace rows overlapped with sampling ----
// The reference's chains write their files after their last step and the parent reads them back (REG:454-481, 775-871); here the
// rows of the steps queued so far can leave for the host while the steps queued behind them are being sampled: a pinned host copy
// of the device's trace arrays (same layout, so a range of rows is one strided copy per array) filled by a second stream behind an
// event of the handle's stream.
int ptnn_trace_image(ptnn_handle* h, float** pos_w, int32_t* row_floats, float** rows) {
    if (int rc = check_ready(h)) return rc;
    if (!pos_w || !row_floats || !rows) return fail(-1, "null argument");
    const int S = h->cfg.n_samples, Rl = h->cfg.n_replicas_local;
    if (h->cap != S) return fail(-1, "trace images need every row resident (trace_capacity 0 or >= n_samples; this handle keeps a ring of %d)", h->cap);
    if (h->plan.compact) return fail(-1, "trace images are not available with compact traces (wide nets): fetch with ptnn_get_traces");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (!h->h_img_pos) {
        // all three or none: a half-made set must not be handed out by the next call
        float *pos = nullptr, *rws = nullptr;
        hipStream_t st = nullptr;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&pos), (size_t)Rl * S * h->PW * sizeof(float), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&rws), (size_t)Rl * S * TR_COUNT * sizeof(float), hipHostMallocDefault);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e != hipSuccess) {
            if (pos) (void)hipHostFree(pos);
            if (rws) (void)hipHostFree(rws);
            (void)hipGetLastError();
            return fail(-2, "pinned trace images of %zu MB: %s", ((size_t)Rl * S * (h->PW + TR_COUNT) * sizeof(float)) >> 20, hipGetErrorString(e));
        }
        h->h_img_pos = pos; h->h_img_rows = rws; h->copy_stream = st;
    }
    *pos_w = h->h_img_pos; *row_floats = h->PW; *rows = h->h_img_rows;
    return 0;
}

int ptnn_trace_image_fetch(ptnn_handle* h, int step0, int nsteps) {
    if (int rc = check_ready(h)) return rc;
    if (!h->h_img_pos) return fail(-1, "call ptnn_trace_image first");
    if (h->failed) return fail(-5, "%s", h->failure.c_str());
    const int S = h->cfg.n_samples, Rl = h->cfg.n_replicas_local;
    if (step0 < 0 || nsteps < 1 || step0 + nsteps > S) return fail(-1, "trace range [%d, %d) outside [0, %d)", step0, step0 + nsteps, S);
    if (step0 + nsteps > h->cur + 1) return fail(-1, "rows up to %d requested but only %d MH steps have been queued", step0 + nsteps - 1, h->cur);
    if (step0 < h->first_row) return fail(-1, "rows below %d were produced before the checkpoint these chains were restored from", h->first_row);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    hipEvent_t queued = nullptr, landed = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&queued, hipEventDisableTiming));
    hipError_t e = hipEventRecord(queued, h->stream);                         // everything queued so far: the steps that write these rows
    if (e == hipSuccess) e = hipStreamWaitEvent(h->copy_stream, queued, 0);
    (void)hipEventDestroy(queued);                                           // released once it has completed
    HIP_TRY(e);
    // one strided copy per array (a replica's rows [step0, step0 + nsteps) are contiguous; replicas lie S rows apart in both layouts).
    // Measured against one linear copy per replica and array (128 enqueues per window for 64 replicas): the rows land 1 ms earlier,
    // and neither shape takes time from the kernels -- Mackey-Glass, every CU full of work-groups that wait for each other: 28.0 ms
    // of kernel time with the copies in flight against 27.9 ms without (profiles/tools/chunk_probe.py)
    const size_t PWb = (size_t)h->PW * sizeof(float), RWb = (size_t)TR_COUNT * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(reinterpret_cast<char*>(h->h_img_pos) + (size_t)step0 * PWb, (size_t)S * PWb,
                             reinterpret_cast<const char*>(h->d_pos_w) + (size_t)step0 * PWb, (size_t)S * PWb, (size_t)nsteps * PWb, Rl,
                             hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(hipMemcpy2DAsync(reinterpret_cast<char*>(h->h_img_rows) + (size_t)step0 * RWb, (size_t)S * RWb,
                             reinterpret_cast<const char*>(h->d_scal) + (size_t)step0 * RWb, (size_t)S * RWb, (size_t)nsteps * RWb, Rl,
                             hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(hipEventCreateWithFlags(&landed, hipEventDisableTiming));
    e = hipEventRecord(landed, h->copy_stream);
    if (e != hipSuccess) { (void)hipEventDestroy(landed); HIP_TRY(e); }
    h->img_events.push_back(landed);
    h->drained = std::max(h->drained, step0 + nsteps - 1);
    return (int)h->img_events.size() - 1;
}

int ptnn_trace_image_wait(ptnn_handle* h, int ticket) {
    if (!h) return fail(-1, "null handle");
    if (ticket < 0 || ticket >= (int)h->img_events.size() || !h->img_events[(size_t)ticket]) return fail(-1, "no such ticket");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    HIP_TRY(hipEventSynchronize(h->img_events[(size_t)ticket]));
    return 0;
}

int ptnn_get_swap_stats(ptnn_handle* h, int64_t* num_swap, int64_t* total_proposals, int32_t* rounds_done) {
    if (!h) return fail(-1, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    long long c[2];
    HIP_TRY(hipMemcpy(c, h->d_counters, sizeof c, hipMemcpyDeviceToHost));
    if (num_swap) *num_swap = c[0];
    if (total_proposals) *total_proposals = c[1];
    if (rounds_done) *rounds_done = h->rounds_done;
    return 0;
}

int ptnn_get_labels(ptnn_handle* h, int32_t* label) {
    if (!h || !label) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    HIP_TRY(hipMemcpy(label, h->d_label[h->lflip], (size_t)h->cfg.n_replicas_global * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int ptnn_get_swap_log(ptnn_handle* h, int32_t* src, int max_rounds) {
    if (!h || !src) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    const int n = std::min(max_rounds, std::min(h->rounds_done, h->max_rounds));
    if (n > 0) HIP_TRY(hipMemcpy(src, h->d_src_log, (size_t)n * h->cfg.n_replicas_global * sizeof(int), hipMemcpyDeviceToHost));
    return n;
}

int ptnn_get_state(ptnn_handle* h, float* w, float* eta, float* likelihood, float* prior, int32_t* num_accepted,
                   int32_t* langevin_count, int32_t* langevin_accepted) {
    if (int rc = check_ready(h)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    const int Rl = h->cfg.n_replicas_local, P = h->P, PS = h->PS;
    std::vector<float> st((size_t)Rl * PS), sf((size_t)Rl * SF_COUNT);
    std::vector<int> si((size_t)Rl * SI_COUNT);
    HIP_TRY(hipMemcpy(st.data(), h->d_state[h->flip], st.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sf.data(), h->d_st_f, sf.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(si.data(), h->d_st_i, si.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int r = 0; r < Rl; ++r) {
        if (w) std::memcpy(w + (size_t)r * P, &st[(size_t)r * PS], P * sizeof(float));
        if (eta) eta[r] = st[(size_t)r * PS + P];
        if (likelihood) likelihood[r] = sf[(size_t)r * SF_COUNT + SF_LIK];
        if (prior) prior[r] = sf[(size_t)r * SF_COUNT + SF_PRIOR];
        if (num_accepted) num_accepted[r] = si[(size_t)r * SI_COUNT + SI_NACC];
        if (langevin_count) langevin_count[r] = si[(size_t)r * SI_COUNT + SI_LG_COUNT];
        if (langevin_accepted) langevin_accepted[r] = si[(size_t)r * SI_COUNT + SI_LG_ACC];
    }
    return 0;
}

// ---- checkpoint / resume: the RNG is counter based, so the chain state is small and a restored handle
// continues the chains bit for bit.  Traces are not part of it: the caller keeps the rows it has fetched. ----
namespace {
struct CkHeader {
    uint32_t magic, version;
    ptnn_config cfg;
    int32_t P, PS, cur, rounds_done, finalized, have_ladder, log_rounds, reserved;
    long long counters[2];
};
constexpr uint32_t CK_MAGIC = 0x4b435450u;      // "PTCK"

// ladder adaptation (header word `reserved` = 1): the spec, both log-gap rows, the ladder history and the recorded acceptances
size_t ck_adapt_bytes(size_t R, int A, size_t logr) {
    return sizeof(ptnn_ladder_adapt_spec) + sizeof(double) * 2 * (R - 1) + sizeof(float) * ((size_t)(A + 1) * R + logr * (R - 1));
}

size_t ck_bytes(const ptnn_handle* h) {
    const size_t Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global, PS = h->PS;
    const size_t logr = (size_t)std::min(h->rounds_done, h->max_rounds);
    return sizeof(CkHeader) + sizeof(float) * (3 * Rl * PS + Rl * SF_COUNT + Rl + 5 * R) + sizeof(int) * (Rl + Rl * SI_COUNT + logr * R + 2 * R) +
           (h->have_adapt ? ck_adapt_bytes(R, h->adapt.rounds, logr) : 0);
}

bool same_chain(const ptnn_config& a, const ptnn_config& b) {
    return a.task == b.task && a.n_in == b.n_in && a.n_hidden == b.n_hidden && a.n_out == b.n_out &&
           a.n_replicas_local == b.n_replicas_local && a.n_replicas_global == b.n_replicas_global &&
           a.first_global_replica == b.first_global_replica && a.n_samples == b.n_samples && a.swap_interval == b.swap_interval &&
           a.pt_switch_step == b.pt_switch_step && a.use_langevin == b.use_langevin && a.swap_rule == b.swap_rule &&
           a.shared_noise == b.shared_noise && a.label_swap == b.label_swap && a.forward_bf16 == b.forward_bf16 && a.l_prob == b.l_prob &&
           a.learn_rate == b.learn_rate && a.step_w == b.step_w && a.step_eta == b.step_eta && a.sigma_squared == b.sigma_squared &&
           a.nu_1 == b.nu_1 && a.nu_2 == b.nu_2 && a.seed == b.seed;
}
}  // namespace

int ptnn_checkpoint_size(ptnn_handle* h, int64_t* bytes) {
    if (int rc = check_ready(h)) return rc;
    if (!bytes) return fail(-1, "null argument");
    *bytes = (int64_t)ck_bytes(h);
    return 0;
}

int ptnn_checkpoint_save(ptnn_handle* h, void* buf, int64_t bytes) {
    if (int rc = check_ready(h)) return rc;
    if (!buf || bytes < (int64_t)ck_bytes(h)) return fail(-1, "checkpoint buffer too small: %lld < %zu", (long long)bytes, ck_bytes(h));
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    const size_t Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global, PS = h->PS;
    CkHeader hd{};
    hd.magic = CK_MAGIC; hd.version = 3; hd.cfg = h->cfg; hd.P = h->P; hd.PS = h->PS; hd.cur = h->cur;
    hd.rounds_done = h->rounds_done; hd.finalized = h->finalized ? 1 : 0; hd.have_ladder = h->have_ladder ? 1 : 0;
    hd.log_rounds = std::min(h->rounds_done, h->max_rounds);
    hd.reserved = h->have_adapt ? 1 : 0;
    HIP_TRY(hipMemcpy(hd.counters, h->d_counters, sizeof(hd.counters), hipMemcpyDeviceToHost));
    char* q = static_cast<char*>(buf);
    std::memcpy(q, &hd, sizeof(hd)); q += sizeof(hd);
    auto get = [&](const void* dev, size_t n) -> int {
        if (n) HIP_TRY(hipMemcpy(q, dev, n, hipMemcpyDeviceToHost));
        q += n;
        return 0;
    };
    if (int rc = get(h->d_state[h->flip], sizeof(float) * Rl * PS)) return rc;
    if (int rc = get(h->d_gd_w[h->flip], sizeof(float) * Rl * PS)) return rc;
    if (int rc = get(h->d_rec_w, sizeof(float) * Rl * PS)) return rc;
    if (int rc = get(h->d_st_f, sizeof(float) * Rl * SF_COUNT)) return rc;
    if (int rc = get(h->d_temps, sizeof(float) * Rl)) return rc;
    if (int rc = get(h->d_L_handoff, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_L_final, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_L_raw, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_prior_post, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_temps_global, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_gd_valid[h->flip], sizeof(int) * Rl)) return rc;
    if (int rc = get(h->d_st_i, sizeof(int) * Rl * SI_COUNT)) return rc;
    if (int rc = get(h->d_src_log, sizeof(int) * (size_t)hd.log_rounds * R)) return rc;
    if (int rc = get(h->d_label[h->lflip], sizeof(int) * R)) return rc;          // slot <-> temperature maps (identity unless label_swap)
    if (int rc = get(h->d_slot_of[h->lflip], sizeof(int) * R)) return rc;
    if (h->have_adapt) {
        std::memcpy(q, &h->adapt, sizeof(h->adapt)); q += sizeof(h->adapt);
        if (int rc = get(h->d_lad_s, sizeof(double) * 2 * (R - 1))) return rc;
        if (int rc = get(h->d_lad_hist, sizeof(float) * (size_t)(h->adapt.rounds + 1) * R)) return rc;
        if (int rc = get(h->d_lad_acc, sizeof(float) * (size_t)hd.log_rounds * (R - 1))) return rc;
    }
    return 0;
}

int ptnn_checkpoint_load(ptnn_handle* h, const void* buf, int64_t bytes) {
    if (!h || !buf) return fail(-1, "null argument");
    if (!h->have_data) return fail(-1, "call ptnn_set_data before ptnn_checkpoint_load");
    if (bytes < (int64_t)sizeof(CkHeader)) return fail(-1, "not a checkpoint (too short)");
    CkHeader hd;
    std::memcpy(&hd, buf, sizeof(hd));
    if (hd.magic != CK_MAGIC || hd.version != 3) return fail(-1, "not a libptnn checkpoint (magic %08x version %u)", hd.magic, hd.version);
    if (!same_chain(hd.cfg, h->cfg) || hd.P != h->P || hd.PS != h->PS)
        return fail(-1, "the checkpoint was written by chains with a different configuration (topology, replicas, samples, seed ...)");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = wait_stream(h)) return rc;
    const size_t Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global, PS = h->PS;
    const size_t need = sizeof(CkHeader) + sizeof(float) * (3 * Rl * PS + Rl * SF_COUNT + Rl + 5 * R) +
                        sizeof(int) * (Rl + Rl * SI_COUNT + (size_t)hd.log_rounds * R + 2 * R);
    if ((size_t)bytes < need) return fail(-1, "truncated checkpoint: %lld < %zu bytes", (long long)bytes, need);
    if (hd.log_rounds > h->max_rounds) return fail(-1, "checkpoint holds more swap rounds than this handle can log");
    if (hd.reserved != 0 && hd.reserved != 1) return fail(-1, "not a libptnn checkpoint (unknown trailer %d)", hd.reserved);
    ptnn_ladder_adapt_spec ad{};
    if (hd.reserved == 1) {
        if ((size_t)bytes < need + sizeof(ad)) return fail(-1, "truncated checkpoint: no ladder adaptation spec");
        std::memcpy(&ad, static_cast<const char*>(buf) + need, sizeof(ad));
        if (ad.struct_bytes != (int32_t)sizeof(ad) || ad.rounds < 0 || ad.rounds > h->max_rounds)
            return fail(-1, "the checkpoint's ladder adaptation spec is not valid here");
        if (h->have_adapt && (h->adapt.rounds != ad.rounds || h->adapt.kappa0 != ad.kappa0 || h->adapt.t0 != ad.t0))
            return fail(-1, "the checkpoint adapts the ladder over %d rounds (kappa0 %g, t0 %g), this handle over %d (kappa0 %g, t0 %g): "
                            "set the same adaptation, or none, before loading it", ad.rounds, ad.kappa0, ad.t0, h->adapt.rounds,
                        h->adapt.kappa0, h->adapt.t0);
        const size_t full = need + ck_adapt_bytes(R, ad.rounds, (size_t)hd.log_rounds);
        if ((size_t)bytes < full) return fail(-1, "truncated checkpoint: %lld < %zu bytes", (long long)bytes, full);
    } else if (h->have_adapt) {
        return fail(-1, "the checkpoint was written without ladder adaptation, this handle adapts the ladder: clear it first "
                        "(ptnn_set_ladder)");
    }
    const char* q = static_cast<const char*>(buf) + sizeof(CkHeader);
    auto put = [&](void* dev, size_t n) -> int {
        if (n) HIP_TRY(hipMemcpy(dev, q, n, hipMemcpyHostToDevice));
        q += n;
        return 0;
    };
    h->flip = 0;
    if (int rc = put(h->d_state[0], sizeof(float) * Rl * PS)) return rc;
    if (int rc = put(h->d_gd_w[0], sizeof(float) * Rl * PS)) return rc;
    if (int rc = put(h->d_rec_w, sizeof(float) * Rl * PS)) return rc;
    if (int rc = put(h->d_st_f, sizeof(float) * Rl * SF_COUNT)) return rc;
    if (int rc = put(h->d_temps, sizeof(float) * Rl)) return rc;
    if (int rc = put(h->d_L_handoff, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_L_final, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_L_raw, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_prior_post, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_temps_global, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_gd_valid[0], sizeof(int) * Rl)) return rc;
    if (int rc = put(h->d_st_i, sizeof(int) * Rl * SI_COUNT)) return rc;
    if (int rc = put(h->d_src_log, sizeof(int) * (size_t)hd.log_rounds * R)) return rc;
    h->lflip = 0;
    if (int rc = put(h->d_label[0], sizeof(int) * R)) return rc;
    if (int rc = put(h->d_slot_of[0], sizeof(int) * R)) return rc;
    if (hd.reserved == 1) {
        // the adaptation travels with the chains: spec, log-gaps and both records as they were
        if (int rc = ladder_adapt_alloc(h, ad)) return rc;
        q += sizeof(ad);
        if (int rc = put(h->d_lad_s, sizeof(double) * 2 * (R - 1))) return rc;
        if (int rc = put(h->d_lad_hist, sizeof(float) * (size_t)(ad.rounds + 1) * R)) return rc;
        HIP_TRY(hipMemset(h->d_lad_acc, 0xff, (size_t)h->max_rounds * (R - 1) * sizeof(float)));
        if (int rc = put(h->d_lad_acc, sizeof(float) * (size_t)hd.log_rounds * (R - 1))) return rc;
        // a restart of this handle (ptnn_set_state) starts from the checkpoint's initial ladder, row 0 of its history
        h->lad_T0.resize(R);
        HIP_TRY(hipMemcpy(h->lad_T0.data(), h->d_lad_hist, R * sizeof(float), hipMemcpyDeviceToHost));
        h->lad_s0.resize(R - 1);
        for (size_t k = 0; k + 1 < R; ++k) h->lad_s0[k] = std::log((double)h->lad_T0[k + 1] - (double)h->lad_T0[k]);
    }
    HIP_TRY(hipMemcpy(h->d_state[1], h->d_state[0], sizeof(float) * Rl * PS, hipMemcpyDeviceToDevice));
    if (h->plan.compact) {
        // compact traces: the rows a later rejected step may repeat are not on this device -- put the recorded row of every chain
        // into trace row hd.cur (the last one before the checkpoint) and point the chains at it
        HIP_TRY(hipMemcpy2D(h->d_pos_w + (size_t)(hd.cur % h->cap) * h->PW, (size_t)h->cap * h->PW * sizeof(float), h->d_rec_w,
                            PS * sizeof(float), (size_t)h->P * sizeof(float), Rl, hipMemcpyDeviceToDevice));
        std::vector<int> si(Rl * SI_COUNT);
        HIP_TRY(hipMemcpy(si.data(), h->d_st_i, si.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < Rl; ++r) si[r * SI_COUNT + SI_REC_ROW] = hd.cur;
        HIP_TRY(hipMemcpy(h->d_st_i, si.data(), si.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(h->d_counters, hd.counters, sizeof(hd.counters), hipMemcpyHostToDevice));
    h->cur = hd.cur; h->rounds_done = hd.rounds_done; h->finalized = hd.finalized != 0; h->have_ladder = hd.have_ladder != 0;
    h->drained = hd.cur; h->first_row = hd.cur + 1;
    HIP_TRY(hipMemset(h->d_error, 0, sizeof(int)));
    if (!h->comm.failed) { h->failed = false; h->failure.clear(); }
    h->h_progress[0] = h->h_progress[1] = hd.rounds_done;
    h->have_state = true;
    return 0;
}

// ---- the posterior analysis calls: predict, convergence, elpd, forecast, evidence ----
}  // extern "C" (the scratch guard below is a class)

namespace {
struct DeviceScratch {            // every buffer of one analysis call, released on every return path
    std::vector<void*> ptrs;
    ~DeviceScratch() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T> hipError_t alloc(T** p, size_t n) {
        *p = nullptr;
        if (n == 0) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e == hipSuccess) { ptrs.push_back(q); *p = static_cast<T*>(q); }
        return e;
    }
    template <typename T> hipError_t upload(T** p, const T* src, size_t n, hipStream_t st) {     // alloc + copy of n host values
        const hipError_t e = alloc(p, n);
        return e != hipSuccess ? e : hipMemcpyAsync(*p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
    }
};

template <typename T> hipError_t fetch(T* dst, const T* src, size_t n, hipStream_t st) {   // an output the caller asked for (non-null)
    return dst ? hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}

size_t scratch_budget(const char* var) {    // $var bytes, default 1 GiB
    const char* e = std::getenv(var);
    if (e && *e) {
        const long long v = std::atoll(e);
        if (v > 0) return (size_t)v;
    }
    return (size_t)1 << 30;
}

// the first check of every analysis call: the spec itself
template <class Spec> int check_spec(const Spec* spec, const char* name) {
    if (!spec) return fail(-1, "null argument");
    if (spec->struct_bytes != (int32_t)sizeof(Spec)) return fail(-1, "%s.struct_bytes = %d, expected %d", name, spec->struct_bytes, (int)sizeof(Spec));
    return 0;
}
// the handle of an analysis call (after the argument checks): ready, and one GPU
int check_handle(ptnn_handle* h, const char* fn) {
    if (int rc = check_ready(h)) return rc;
    if (h->comm.kind != COMM_NONE) return fail(-3, "%s serves one GPU: this handle has a communicator attached", fn);
    return 0;
}
// the device work of an analysis call starts behind everything queued; a failed run is refused here
int start_device(ptnn_handle* h) {
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    return finish_stream(h);
}

// the trace rows step0, step0 + thin, ... < step0 + nsteps of the listed local replicas (NULL = all): the residency, checkpoint
// and ring rules of ptnn_get_traces; *reps = the chains, *m = rows per chain.
int select_trace_rows(const ptnn_handle* h, const int32_t* replicas, int n_replicas, int step0, int nsteps, int thin,
                      std::vector<int32_t>* reps, int* m) {
    const int S = h->cfg.n_samples, Rl = h->cfg.n_replicas_local, cap = h->cap;
    if (step0 < 0 || nsteps < 1 || step0 + nsteps > S) return fail(-1, "trace range [%d, %d) outside [0, %d)", step0, step0 + nsteps, S);
    if (step0 + nsteps > h->cur + 1) return fail(-1, "rows up to %d requested but only %d MH steps have been queued", step0 + nsteps - 1, h->cur);
    if (step0 < h->first_row) return fail(-1, "rows below %d were produced before the checkpoint these chains were restored from", h->first_row);
    if (step0 < h->cur + 1 - cap) return fail(-1, "row %d has already been overwritten in the trace ring (capacity %d, %d steps done)", step0, cap, h->cur);
    reps->clear();
    if (replicas) {
        for (int k = 0; k < n_replicas; ++k) {
            if (replicas[k] < 0 || replicas[k] >= Rl) return fail(-1, "replica %d out of range [0, %d)", replicas[k], Rl);
            reps->push_back(replicas[k]);
        }
    } else {
        for (int r = 0; r < Rl; ++r) reps->push_back(r);
    }
    *m = (nsteps + thin - 1) / thin;
    return 0;
}

// The weight vectors an analysis call reads, from the fields every spec names alike: host vectors w [n_w][P] (with eta [n_w] and
// integer multiplicities [n_w], each optional), or the trace rows of select_trace_rows.
struct SampleSource {
    bool host;                      // host vectors (ptnn_elpd: also a host loglik); else trace rows
    const float* w;
    const float* eta;
    int64_t n_w;
    const int32_t* multiplicity;
    const int32_t* replicas;
    int n_replicas, step0, nsteps, thin;
    std::vector<int32_t> reps;      // trace: the chains
    int m = 0;                      // trace: rows per chain
    long long n_items = 0, M = 0;   // host vectors or trace rows; samples, multiplicities counted
    const int32_t* weights() const { return host ? multiplicity : nullptr; }
};
template <class Spec> SampleSource source_of(const Spec& s, bool host, const float* eta) {
    return SampleSource{host, s.w, eta, s.n_w, s.multiplicity, s.replicas, s.n_replicas, s.step0, s.nsteps, s.thin};
}
// the checks that need no handle; `unit` names a host item in the message
int check_source(const SampleSource& src, const char* unit) {
    if (src.host) return src.n_w < 1 ? fail(-1, "n_w = %lld host %s: need at least one", (long long)src.n_w, unit) : 0;
    if (src.thin < 1) return fail(-1, "thin = %d must be >= 1", src.thin);
    if (src.replicas && src.n_replicas < 1) return fail(-1, "n_replicas = %d with a replica list", src.n_replicas);
    return 0;
}
// n_items and M: host multiplicities summed (no handle needed), or the trace rows selected
int count_samples(const ptnn_handle* h, SampleSource& src) {
    if (src.host) {
        src.n_items = src.n_w;
        src.M = src.multiplicity ? 0 : src.n_w;
        for (int64_t k = 0; src.multiplicity && k < src.n_w; ++k) {
            if (src.multiplicity[k] < 0) return fail(-1, "multiplicity[%lld] = %d is negative", (long long)k, src.multiplicity[k]);
            src.M += src.multiplicity[k];
        }
        return 0;
    }
    if (int rc = select_trace_rows(h, src.replicas, src.n_replicas, src.step0, src.nsteps, src.thin, &src.reps, &src.m)) return rc;
    src.n_items = src.M = (long long)src.reps.size() * src.m;
    return 0;
}
int sample_limit(const SampleSource& src) {
    if (src.M > 0x7fffffffLL || src.n_items > 0x7fffffffLL) return fail(-1, "%lld samples: at most 2^31 - 1 per call", src.M);
    return 0;
}

// Stage a: the items of a source collapse into distinct samples -- maximal runs of bitwise-equal consecutive vectors of one chain
// or of the host list -- with integer multiplicities (sample_runs_kernel, predict_scan_kernel).  `eta`: the samples are (w, eta)
// -- a regression's eta is read, compared and checked, a classification's is 0 -- and every run gets its eta
// (elpd_run_eta_kernel).  Without `merge` every item is a sample of its own with count 1 (forecast with noise: every occurrence
// is its own trajectory).
struct Distinct {
    const float* base = nullptr;    // the vectors: d_pos_w rows or the uploaded host vectors
    long long* run_off = nullptr;   // [U] float offset of sample u in base
    int* run_cnt = nullptr;         // [U] its multiplicity
    int* item_run = nullptr;        // [n_items] the sample of every item (merge)
    float* run_eta = nullptr;       // [U] its eta (eta)
    int U = 0;
};
int distinct_samples(ptnn_handle* h, DeviceScratch& mem, const SampleSource& src, bool eta, bool merge, Distinct* d) {
    const long long n = src.n_items;
    const bool reg = eta && h->cfg.task == PTNN_TASK_REG;
    hipStream_t st = h->stream;
    long long* item_off = nullptr;
    int *flag = nullptr, *err = nullptr, *weight = nullptr, *reps = nullptr;
    float *item_eta = nullptr, *w = nullptr, *host_eta = nullptr;
    HIP_TRY(mem.alloc(&item_off, (size_t)n));
    HIP_TRY(mem.alloc(&flag, (size_t)n));
    HIP_TRY(mem.alloc(&d->run_cnt, (size_t)n));
    HIP_TRY(mem.alloc(&err, 4));        // [0] runs, [1] unresolved compact rows, [2] rows without eta, [3] the first such chain
    if (eta) HIP_TRY(mem.alloc(&item_eta, (size_t)n));
    if (merge) {
        HIP_TRY(mem.alloc(&d->run_off, (size_t)n));
        HIP_TRY(mem.alloc(&d->item_run, (size_t)n));
        if (eta) HIP_TRY(mem.alloc(&d->run_eta, (size_t)n));
        HIP_TRY(hipMemsetAsync(d->run_cnt, 0, (size_t)n * sizeof(int), st));
    } else {
        d->run_off = item_off;
        d->run_eta = item_eta;
        HIP_TRY(hipMemsetD32Async(d->run_cnt, 1, (size_t)n, st));
    }
    HIP_TRY(hipMemsetAsync(err, 0, 3 * sizeof(int), st));
    if (eta) HIP_TRY(hipMemsetAsync(err + 3, 0x7f, sizeof(int), st));
    SampleSel sel{};
    sel.reg = reg ? 1 : 0; sel.P = h->P; sel.n_items = n; sel.item_off = item_off; sel.item_eta = item_eta; sel.flag = flag;
    sel.error = err + 1;
    if (src.host) {
        HIP_TRY(mem.upload(&w, src.w, (size_t)n * h->P, st));
        if (reg) HIP_TRY(mem.upload(&host_eta, src.eta, (size_t)n, st));
        if (merge && src.multiplicity) HIP_TRY(mem.upload(&weight, src.multiplicity, (size_t)n, st));
        sel.host = 1; sel.pos_w = w; sel.host_eta = host_eta;
    } else {
        HIP_TRY(mem.upload(&reps, src.reps.data(), src.reps.size(), st));
        sel.host = 0; sel.pos_w = h->d_pos_w; sel.scal = h->d_scal; sel.replicas = reps; sel.st_i = h->d_st_i; sel.cap = h->cap;
        sel.PW = h->PW; sel.step0 = src.step0; sel.thin = src.thin; sel.m = src.m; sel.compact = h->plan.compact ? 1 : 0; sel.cur = h->cur;
    }
    d->base = sel.pos_w;
    const unsigned item_blocks = (unsigned)((n + PRED_THREADS - 1) / PRED_THREADS);
    hipLaunchKernelGGL(sample_runs_kernel, dim3(item_blocks), dim3(PRED_THREADS), 0, st, sel);
    HIP_TRY(hipGetLastError());
    if (merge) {
        PredictScan sc{n, flag, item_off, weight, d->item_run, d->run_off, d->run_cnt, err};
        hipLaunchKernelGGL(predict_scan_kernel, dim3(1), dim3(PRED_SCAN_THREADS), 0, st, sc);
        HIP_TRY(hipGetLastError());
        if (eta) {
            hipLaunchKernelGGL(elpd_run_eta_kernel, dim3(item_blocks), dim3(ELPD_THREADS), 0, st, n, (const int*)flag,
                               (const int*)d->item_run, (const float*)item_eta, d->run_eta);
            HIP_TRY(hipGetLastError());
        }
    }
    int e[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(e, err, sizeof e, hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream(h)) return rc;          // also keeps the host arrays of `src` alive until the copies are done
    if (e[1]) return fail(-2, "%d selected compact trace rows refer to rows that are not resident (internal error)", e[1]);
    if (e[2]) {
        const int c = e[3] >= 0 && e[3] < (int)src.reps.size() ? e[3] : 0;
        return fail(-1, "%s%d selected trace rows precede their chain's first accepted MH step (chain %d, local replica %d, among "
                        "others): no eta = log tau^2 was recorded for them; start the selection later (a larger burn_in)",
                    merge ? "" : "noise: ", e[2], c, src.reps.empty() ? 0 : src.reps[(size_t)c]);
    }
    d->U = merge ? e[0] : (int)n;
    if (d->U < 1 || d->U > n) return fail(-2, "run-length pass found %d distinct samples among %lld rows (internal error)", d->U, n);
    return 0;
}
// the sample of every item on the host, for the selection-order outputs (queued: valid after the next wait_stream)
int item_runs(ptnn_handle* h, const Distinct& d, long long n_items, std::vector<int>* out) {
    out->resize((size_t)n_items);
    if (!d.item_run) {
        for (long long i = 0; i < n_items; ++i) (*out)[(size_t)i] = (int)i;
        return 0;
    }
    HIP_TRY(hipMemcpyAsync(out->data(), d.item_run, (size_t)n_items * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return 0;
}
// A block of per-sample outputs blk [ncols][U] on the device, expanded to the selection's order (chain-major, item i `mult[i]`
// times, null: once): selected sample `row` gets its columns at out + row * row_stride + col0.
template <typename T>
int scatter_samples(ptnn_handle* h, const T* blk, int ncols, int U, const std::vector<int>& item_run, const int32_t* mult, T* out,
                    size_t row_stride, size_t col0) {
    std::vector<T> hb((size_t)ncols * U);
    HIP_TRY(hipMemcpyAsync(hb.data(), blk, hb.size() * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (int rc = wait_stream(h)) return rc;
    size_t row = 0;
    for (size_t i = 0; i < item_run.size(); ++i) {
        const size_t u = (size_t)item_run[i];
        for (int k = 0, reps = mult ? mult[i] : 1; k < reps; ++k, ++row) {
            T* dst = out + row * row_stride + col0;
            for (int c = 0; c < ncols; ++c) dst[c] = hb[(size_t)c * U + u];
        }
    }
    return 0;
}

// Input rows of an analysis call: `source` PTNN_PREDICT_X_HOST with host rows, or the handle's train / test set
static_assert(PTNN_FORECAST_ORIGIN_HOST == PTNN_PREDICT_X_HOST && PTNN_FORECAST_ORIGIN_TRAIN == PTNN_PREDICT_X_TRAIN &&
              PTNN_FORECAST_ORIGIN_TEST == PTNN_PREDICT_X_TEST, "ptnn.h row sources");
struct RowSource {
    int source;
    const float* host;
    int n;
    const char *field, *prefix, *arg, *count;   // names in the messages: "x_source", "PTNN_PREDICT_X", "x", "n_rows"
};
int check_rows(const RowSource& r) {        // no handle needed
    if (r.source != PTNN_PREDICT_X_HOST && r.source != PTNN_PREDICT_X_TRAIN && r.source != PTNN_PREDICT_X_TEST)
        return fail(-1, "%s = %d is not %s_HOST, _TRAIN or _TEST", r.field, r.source, r.prefix);
    if (r.source == PTNN_PREDICT_X_HOST && !r.host) return fail(-1, "%s %s_HOST needs %s", r.field, r.prefix, r.arg);
    return 0;
}
int fit_rows(const ptnn_handle* h, const RowSource& r) {
    if (r.source == PTNN_PREDICT_X_TRAIN && r.n != h->Ntr) return fail(-1, "%s = %d but the train set has %d rows", r.count, r.n, h->Ntr);
    if (r.source == PTNN_PREDICT_X_TEST && r.n != h->Nte) return fail(-1, "%s = %d but the test set has %d rows", r.count, r.n, h->Nte);
    return 0;
}
// the rows on the device: the host rows (`width` floats each) uploaded, or the data set; row k at *x + k * *xs
int upload_rows(ptnn_handle* h, DeviceScratch& mem, const RowSource& r, int width, const float** x, int* xs) {
    if (r.source == PTNN_PREDICT_X_HOST) {
        float* d = nullptr;
        HIP_TRY(mem.upload(&d, r.host, (size_t)r.n * width, h->stream));
        *x = d; *xs = width;
    } else {
        *x = h->d_data + (r.source == PTNN_PREDICT_X_TEST ? (size_t)h->Ntr * h->IPY : 0);
        *xs = h->IPY;
    }
    return 0;
}

// Stage b of predict, elpd and evidence: the per-shape predict_fwd, NV distinct vectors staged in LDS per work-group
struct ForwardPlan {
    int PV = 0, NV = 0;
    size_t lds = 0;
    int init(const ptnn_handle* h, const char* what) {
        const int P = h->P;
        PV = round_up4(P);
        const int per_vec = PV + (PRED_THREADS / WAVE + 1) * h->cfg.n_out * WAVE;   // staged vector + partial sums + transposed tile
        NV = std::max(1, std::min(PRED_MAX_NV, (48 * 1024 / 4) / per_vec));
        lds = (size_t)NV * per_vec * sizeof(float);
        if (lds > 152 * 1024) return fail(-3, "%s: a %d-parameter vector does not fit in LDS", what, P);
        return raise_lds_limit(reinterpret_cast<const void*>(h->shape->predict_fwd), lds);
    }
    // fx [nr * O][U] = the outputs of vectors base + run_off[u] on rows [r0, r0 + nr) of x
    int launch(const ptnn_handle* h, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U, float* fx) const {
        PredictFwd fa{base, run_off, x, xs, r0, nr, h->cfg.n_hidden, h->P, PV, U, NV, fx};
        hipLaunchKernelGGL(h->shape->predict_fwd, dim3((unsigned)((U + NV - 1) / NV), (unsigned)((nr + WAVE - 1) / WAVE)), dim3(PRED_THREADS), lds,
                           h->stream, fa);
        HIP_TRY(hipGetLastError());
        return 0;
    }
};
// rows per block of the forward pass: `budget` bytes of scratch at `row_bytes` per row, and at most 65535 work-groups of WAVE
// rows (grid.y of predict_fwd)
long long row_block(size_t budget, size_t row_bytes, long long n_rows) {
    return std::max(1LL, std::min<long long>({(long long)(budget / row_bytes), 65535LL * WAVE, n_rows}));
}

// the order statistics of predict and forecast: ranks [n_ranks] in the expanded multiset of M samples
int check_ranks(int n_ranks, const int64_t* ranks, const void* order_stats) {
    if (n_ranks < 0 || n_ranks > PTNN_PREDICT_MAX_RANKS) return fail(-1, "n_ranks = %d outside [0, %d]", n_ranks, PTNN_PREDICT_MAX_RANKS);
    if (n_ranks > 0 && !ranks) return fail(-1, "n_ranks = %d but ranks is NULL", n_ranks);
    if (order_stats && n_ranks == 0) return fail(-1, "order_stats requested without ranks");
    return 0;
}
int check_rank_values(int n_ranks, const int64_t* ranks, long long M) {
    for (int k = 0; k < n_ranks; ++k)
        if (ranks[k] < 0 || ranks[k] >= M) return fail(-1, "rank %lld outside [0, %lld)", (long long)ranks[k], M);
    return 0;
}
}  // namespace

extern "C" {

// ---- posterior predictive (ptnn_dev_predict.hpp) ----
int ptnn_predict(ptnn_handle* h, const ptnn_predict_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_predict_spec")) return rc;
    const ptnn_predict_spec& s = *spec;
    SampleSource src = source_of(s, s.w != nullptr, nullptr);
    const RowSource rows{s.x_source, s.x, s.n_rows, "x_source", "PTNN_PREDICT_X", "x", "n_rows"};
    if (int rc = check_source(src, "vectors")) return rc;
    if (int rc = check_rows(rows)) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    if (int rc = check_ranks(s.n_ranks, s.ranks, s.order_stats)) return rc;
    if (int rc = check_handle(h, "ptnn_predict")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    if (s.vote && h->cfg.task != PTNN_TASK_CLS) return fail(-1, "vote: a regression has no classes");
    if (int rc = fit_rows(h, rows)) return rc;
    if (int rc = count_samples(h, src)) return rc;
    const long long M = src.M;
    if (M < 1) return fail(-1, "the selection holds no sample");
    if (int rc = sample_limit(src)) return rc;
    if (int rc = check_rank_values(s.n_ranks, s.ranks, M)) return rc;
    if (s.n_samples) *s.n_samples = M;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const int ncols = s.n_rows * O;
    const float* d_x = nullptr;
    int xs = 0;
    if (int rc = upload_rows(h, mem, rows, I, &d_x, &xs)) return rc;
    Distinct d;
    if (int rc = distinct_samples(h, mem, src, false, true, &d)) return rc;
    const int U = d.U;
    if (s.n_distinct) *s.n_distinct = U;
    // outputs on the device for every column; votes as integer counts (exact whatever the order)
    double* d_mean = nullptr; float* d_ostat = nullptr; long long* d_votes = nullptr; long long* d_ranks = nullptr;
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    if (s.n_ranks) {
        HIP_TRY(mem.alloc(&d_ostat, (size_t)s.n_ranks * ncols));
        HIP_TRY(mem.upload(&d_ranks, (const long long*)s.ranks, (size_t)s.n_ranks, st));
    }
    if (h->cfg.task == PTNN_TASK_CLS) HIP_TRY(mem.alloc(&d_votes, (size_t)ncols));
    // stage b + c in blocks of rows: fx scratch U x (rows x O) floats under the budget
    const long long rows_blk = row_block(scratch_budget("PTNN_PREDICT_SCRATCH_BYTES"), (size_t)U * sizeof(float) * O, s.n_rows);
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * O * U));
    ForwardPlan fwd;
    if (int rc = fwd.init(h, "posterior predictive")) return rc;
    std::vector<int> item_run;
    if (s.samples) if (int rc = item_runs(h, d, src.n_items, &item_run)) return rc;
    for (long long r0 = 0; r0 < s.n_rows; r0 += rows_blk) {
        const int nr = (int)std::min<long long>(rows_blk, s.n_rows - r0);
        if (int rc = fwd.launch(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
        PredictRed ra{d_fx, d.run_cnt, U, O, (int)r0 * O, ncols, M, s.n_ranks, d_ranks, d_mean, d_ostat, d_votes};
        hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)(nr * O)), dim3(PRED_THREADS), 0, st, ra);
        HIP_TRY(hipGetLastError());
        if (s.samples)
            if (int rc = scatter_samples(h, d_fx, nr * O, U, item_run, src.weights(), s.samples, (size_t)s.n_rows * O, (size_t)r0 * O)) return rc;
    }
    std::vector<long long> votes_h(s.vote ? (size_t)ncols : 0);
    HIP_TRY(fetch(s.mean, d_mean, (size_t)ncols, st));
    HIP_TRY(fetch(s.order_stats, d_ostat, (size_t)s.n_ranks * ncols, st));
    HIP_TRY(fetch(s.vote ? votes_h.data() : nullptr, d_votes, (size_t)ncols, st));
    if (int rc = wait_stream(h)) return rc;
    if (s.vote)
        for (int c = 0; c < ncols; ++c) s.vote[c] = (double)votes_h[(size_t)c] / (double)M;
    return 0;
}

// ---- convergence diagnostics (ptnn_dev_convergence.hpp) ----
static_assert(PTNN_TR_LIKEH == TR_LIKEH && PTNN_TR_ACC_TE == TR_ACC_TE && PTNN_TR_ACCEPT == TR_ACCEPT && PTNN_TR_SRC == TR_SRC, "ptnn.h TR order");

// split-R-hat / split-ESS of Q quantities over C chains of n draws, gathered by `ga` (its source fields set: trace rows, or
// draws [C][n][Q] in device memory); outputs are host arrays, any may be null.  Shared by ptnn_convergence and ptnn_evidence.
static int conv_drive(ptnn_handle* h, DeviceScratch& mem, ConvGather ga, const std::vector<int>& qcol, int C, int n, int n_lags,
                      double* mean, double* var, double* r_hat, double* ess, int32_t* trunc_lag, double* ess_chain, double* rho) {
    const int hl = n / 2, M = 2 * C, Q = (int)qcol.size();
    const bool per_chain = ess_chain != nullptr;
    const int NS = 1 + (per_chain ? C : 0);
    hipStream_t st = h->stream;
    int *d_qcol = nullptr, *d_error = nullptr;
    HIP_TRY(mem.upload(&d_qcol, qcol.data(), (size_t)Q, st));
    HIP_TRY(mem.alloc(&d_error, 1));
    HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), st));
    ga.C = C; ga.n = n; ga.h = hl; ga.error = d_error;
    // outputs of every quantity
    double *d_mean = nullptr, *d_var = nullptr, *d_rhat = nullptr, *d_ess = nullptr, *d_essc = nullptr, *d_rho = nullptr;
    int* d_trunc = nullptr;
    HIP_TRY(mem.alloc(&d_mean, (size_t)Q));
    HIP_TRY(mem.alloc(&d_var, (size_t)Q));
    HIP_TRY(mem.alloc(&d_rhat, (size_t)Q));
    HIP_TRY(mem.alloc(&d_ess, (size_t)Q));
    HIP_TRY(mem.alloc(&d_trunc, (size_t)Q));
    if (per_chain) HIP_TRY(mem.alloc(&d_essc, (size_t)C * Q));
    if (n_lags) HIP_TRY(mem.alloc(&d_rho, (size_t)n_lags * Q));
    // blocks of quantities: the scratch of one quantity, every stage's
    const size_t per_q = sizeof(double) * ((size_t)M * hl + 2 * (size_t)M + 2 * (size_t)C + 2 + (size_t)CONV_MAX_LAGS * C)
                       + sizeof(ConvSeq) * NS + sizeof(int) * (3 + (per_chain ? (size_t)C : 0));
    const int Qb = (int)std::max<size_t>(1, std::min<size_t>(scratch_budget("PTNN_CONVERGENCE_SCRATCH_BYTES") / per_q, (size_t)Q));
    double *d_x = nullptr, *d_smean = nullptr, *d_ssq = nullptr, *d_csum = nullptr, *d_cm2 = nullptr, *d_pmean = nullptr, *d_pvar = nullptr;
    double* d_chain = nullptr;
    ConvSeq* d_seq = nullptr;
    int *d_full = nullptr, *d_copen = nullptr, *d_any = nullptr, *d_open = nullptr;
    HIP_TRY(mem.alloc(&d_x, (size_t)Qb * M * hl));
    HIP_TRY(mem.alloc(&d_smean, (size_t)Qb * M));
    HIP_TRY(mem.alloc(&d_ssq, (size_t)Qb * M));
    HIP_TRY(mem.alloc(&d_csum, (size_t)Qb * C));
    HIP_TRY(mem.alloc(&d_cm2, (size_t)Qb * C));
    HIP_TRY(mem.alloc(&d_pmean, (size_t)Qb));
    HIP_TRY(mem.alloc(&d_pvar, (size_t)Qb));
    HIP_TRY(mem.alloc(&d_chain, (size_t)CONV_MAX_LAGS * C * Qb));
    HIP_TRY(mem.alloc(&d_seq, (size_t)Qb * NS));
    HIP_TRY(mem.alloc(&d_full, (size_t)Qb));
    if (per_chain) HIP_TRY(mem.alloc(&d_copen, (size_t)Qb * C));
    HIP_TRY(mem.alloc(&d_any, (size_t)Qb));
    HIP_TRY(mem.alloc(&d_open, (size_t)Qb));
    std::vector<int> any_h((size_t)Qb), open_h((size_t)Qb);
    for (int q0 = 0; q0 < Q; q0 += Qb) {
        const int nq = std::min(Qb, Q - q0);
        // 1. gather and moments
        ga.qcol = d_qcol + q0; ga.nq = nq; ga.x = d_x; ga.smean = d_smean; ga.ssq = d_ssq; ga.csum = d_csum; ga.cm2 = d_cm2;
        hipLaunchKernelGGL(conv_gather_kernel, dim3((unsigned)C, (unsigned)((nq + CONV_TILE - 1) / CONV_TILE)), dim3(CONV_THREADS), 0, st, ga);
        HIP_TRY(hipGetLastError());
        // 2. W, var+ and the state of every sequence
        ConvMoments mo{d_smean, d_ssq, d_csum, d_cm2, nq, C, n, hl, NS, d_seq, d_pmean, d_pvar};
        const long long nseq = (long long)nq * NS;
        hipLaunchKernelGGL(conv_moments_kernel, dim3((unsigned)((nseq + CONV_THREADS - 1) / CONV_THREADS)), dim3(CONV_THREADS), 0, st, mo);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(d_full, 1, (size_t)nq * sizeof(int), st));             // non-zero: every sequence starts open
        if (per_chain) HIP_TRY(hipMemsetAsync(d_copen, 1, (size_t)nq * C * sizeof(int), st));
        int n_open = nq;
        for (int k = 0; k < nq; ++k) open_h[(size_t)k] = k;
        HIP_TRY(hipMemcpyAsync(d_open, open_h.data(), (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
        // 3. blocks of lags, each twice the last, for the quantities with a sequence still open
        for (int t0 = 0, nl = CONV_LAG_TILE; n_open > 0 && t0 < hl; t0 += nl, nl = std::min(2 * nl, CONV_MAX_LAGS)) {
            nl = std::min(nl, (hl - t0 + CONV_LAG_TILE - 1) / CONV_LAG_TILE * CONV_LAG_TILE);
            ConvLags la{d_x, C, hl, d_open, n_open, d_full, d_copen, t0, d_chain};
            hipLaunchKernelGGL(conv_lags_kernel, dim3((unsigned)((n_open + CONV_TILE - 1) / CONV_TILE), (unsigned)(nl / CONV_LAG_TILE), (unsigned)C), dim3(CONV_THREADS), 0, st, la);
            HIP_TRY(hipGetLastError());
            ConvStep sp{d_chain, d_open, n_open, C, hl, NS, t0, nl, n_lags, Q, q0, d_seq, d_full, d_copen, d_any, d_rho};
            hipLaunchKernelGGL(conv_step_kernel, dim3((unsigned)n_open), dim3(WAVE), 0, st, sp);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(any_h.data(), d_any, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, st));
            if (int rc = wait_stream(h)) return rc;
            const int was_open = n_open;
            n_open = 0;
            for (int k = 0; k < was_open; ++k)
                if (any_h[(size_t)open_h[(size_t)k]]) open_h[(size_t)n_open++] = open_h[(size_t)k];
            if (n_open) HIP_TRY(hipMemcpyAsync(d_open, open_h.data(), (size_t)n_open * sizeof(int), hipMemcpyHostToDevice, st));
        }
        if (n_open) return fail(-2, "%d quantities still open after every lag (internal error)", n_open);
        // 4. tau, ess, r_hat
        ConvFinish fi{d_seq, d_pmean, d_pvar, nq, NS, C, hl, Q, q0, d_mean, d_var, d_rhat, d_ess, d_essc, d_trunc};
        hipLaunchKernelGGL(conv_finish_kernel, dim3((unsigned)((nseq + CONV_THREADS - 1) / CONV_THREADS)), dim3(CONV_THREADS), 0, st, fi);
        HIP_TRY(hipGetLastError());
    }
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_error, sizeof(int), hipMemcpyDeviceToHost, st));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, d_mean, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (var) HIP_TRY(hipMemcpyAsync(var, d_var, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (r_hat) HIP_TRY(hipMemcpyAsync(r_hat, d_rhat, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (ess) HIP_TRY(hipMemcpyAsync(ess, d_ess, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (trunc_lag) HIP_TRY(hipMemcpyAsync(trunc_lag, d_trunc, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (per_chain) HIP_TRY(hipMemcpyAsync(ess_chain, d_essc, (size_t)C * Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n_lags) HIP_TRY(hipMemcpyAsync(rho, d_rho, (size_t)n_lags * Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream(h)) return rc;
    if (err) return fail(-2, "%d selected compact trace rows refer to rows that are not resident (internal error)", err);
    return 0;
}

int ptnn_convergence(ptnn_handle* h, const ptnn_convergence_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_convergence_spec")) return rc;
    const ptnn_convergence_spec& s = *spec;
    const bool host_src = s.draws != nullptr;
    constexpr int scalar_cols = (1 << TR_LIKEH) | (1 << TR_RMSE_TR) | (1 << TR_RMSE_TE) | (1 << TR_ACC_TR) | (1 << TR_ACC_TE);
    if (host_src) {
        if (s.n_chains < 1) return fail(-1, "n_chains = %d must be >= 1", s.n_chains);
        if (s.n_draws < 4) return fail(-1, "n_draws = %d: the split chains need at least 4 draws per chain", s.n_draws);
        if (s.n_quantities < 1) return fail(-1, "n_quantities = %d must be >= 1", s.n_quantities);
    } else {
        if (s.thin < 1) return fail(-1, "thin = %d must be >= 1", s.thin);
        if (s.replicas && s.n_replicas < 1) return fail(-1, "n_replicas = %d with a replica list", s.n_replicas);
        if (s.params && s.n_params < 0) return fail(-1, "n_params = %d with a parameter list", s.n_params);
        if (s.scalars & ~scalar_cols)
            return fail(-1, "scalars = 0x%x: only TR_LIKEH, TR_RMSE_TR, TR_RMSE_TE, TR_ACC_TR and TR_ACC_TE are quantities "
                            "(not TR_ACCEPT, TR_LOGALPHA or TR_SRC)", (unsigned)s.scalars);
    }
    if (s.n_lags < 0) return fail(-1, "n_lags = %d must be >= 0", s.n_lags);
    if (s.n_lags > 0 && !s.rho) return fail(-1, "n_lags = %d but rho is NULL", s.n_lags);
    if (s.rho && s.n_lags == 0) return fail(-1, "rho requested with n_lags = 0");
    if (int rc = check_handle(h, "ptnn_convergence")) return rc;
    const int P = h->P, cap = h->cap;
    // the selection: chains, draws per chain, the column of every quantity
    std::vector<int32_t> reps;
    std::vector<int> qcol;
    int C = 0, n = 0;
    if (host_src) {
        C = s.n_chains; n = s.n_draws;
        for (int q = 0; q < s.n_quantities; ++q) qcol.push_back(q);
    } else {
        if (int rc = select_trace_rows(h, s.replicas, s.n_replicas, s.step0, s.nsteps, s.thin, &reps, &n)) return rc;
        C = (int)reps.size();
        if (n < 4) return fail(-1, "%d draws per chain selected: the split chains need at least 4", n);
        if (s.params) {
            for (int k = 0; k < s.n_params; ++k) {
                if (s.params[k] < 0 || s.params[k] >= P) return fail(-1, "parameter %d out of range [0, %d)", s.params[k], P);
                qcol.push_back(s.params[k]);
            }
        } else {
            for (int p = 0; p < P; ++p) qcol.push_back(p);
        }
        for (int c = 0; c < TR_COUNT; ++c)
            if (s.scalars & (1 << c)) qcol.push_back(-1 - c);
        if (qcol.empty()) return fail(-1, "no quantity selected");
    }
    const int hl = n / 2, Q = (int)qcol.size();
    if (s.n_lags > hl) return fail(-1, "n_lags = %d exceeds the split-chain length %d", s.n_lags, hl);

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    int* d_reps = nullptr;
    float* d_draws = nullptr;
    ConvGather ga{};
    if (host_src) {
        const size_t nd = (size_t)C * n * Q;
        HIP_TRY(mem.upload(&d_draws, s.draws, nd, st));
        ga.host = 1; ga.draws = d_draws; ga.Qh = Q;
    } else {
        HIP_TRY(mem.upload(&d_reps, reps.data(), reps.size(), st));
        ga.host = 0; ga.pos_w = h->d_pos_w; ga.scal = h->d_scal; ga.replicas = d_reps; ga.cap = cap; ga.PW = h->PW;
        ga.step0 = s.step0; ga.thin = s.thin; ga.compact = h->plan.compact ? 1 : 0;
    }
    return conv_drive(h, mem, ga, qcol, C, n, s.n_lags, s.mean, s.var, s.r_hat, s.ess, s.trunc_lag, s.ess_chain, s.rho);
}

// ---- predictive accuracy (ptnn_dev_elpd.hpp) ----
static_assert(PTNN_ELPD_TAIL_CAP == ELPD_TAIL_CAP, "ptnn.h tail capacity");

int ptnn_elpd(ptnn_handle* h, const ptnn_elpd_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_elpd_spec")) return rc;
    const ptnn_elpd_spec& s = *spec;
    const bool ll_src = s.loglik != nullptr, host_src = s.w != nullptr;
    SampleSource src = source_of(s, ll_src || host_src, s.eta);
    const RowSource rows{s.x_source, s.x, s.n_rows, "x_source", "PTNN_PREDICT_X", "x", "n_rows"};
    if (ll_src && host_src) return fail(-1, "give host vectors w or a host loglik, not both");
    if (!(s.r_eff > 0.0) || !std::isfinite(s.r_eff)) return fail(-1, "r_eff = %g must be a finite number > 0", s.r_eff);
    if (!src.host && s.nsteps < 1)
        return fail(-1, "no source: nsteps = %d trace rows, and neither host vectors w nor a host loglik", s.nsteps);
    if (int rc = check_source(src, "samples")) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    if (!ll_src)
        if (int rc = check_rows(rows)) return rc;
    if (ll_src && s.loglik_out) return fail(-1, "loglik_out: the log-likelihood is the input of this source");
    // the sample count of the host sources
    if (src.host)
        if (int rc = count_samples(nullptr, src)) return rc;
    if (ll_src)
        for (long long k = 0; k < src.n_items * s.n_rows; ++k)
            if (!std::isfinite(s.loglik[k])) return fail(-1, "loglik[%lld, %lld] = %g is not finite", k / s.n_rows, k % s.n_rows, s.loglik[k]);
    if (int rc = check_handle(h, "ptnn_elpd")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    if (host_src && reg && !s.eta) return fail(-1, "a regression's host vectors need eta = log tau^2 (one per vector)");
    if (!ll_src)
        if (int rc = fit_rows(h, rows)) return rc;
    if (!ll_src && s.x_source == PTNN_PREDICT_X_HOST && !reg)
        for (int n = 0; n < s.n_rows; ++n) {
            const float yv = s.x[(size_t)n * (I + 1) + I];
            if (!(yv >= 0.0f) || yv >= (float)O || yv != std::floor(yv))
                return fail(-1, "class label %g in row %d is not an integer in [0, %d)", (double)yv, n, O);
        }
    if (!src.host)
        if (int rc = count_samples(h, src)) return rc;
    const long long n_items = src.n_items, S = src.M;
    if (S < 2) return fail(-1, "the selection holds %lld samples: p_waic (a variance, ddof 1) needs at least 2", S);
    if (int rc = sample_limit(src)) return rc;
    const long long M = (long long)std::ceil(std::min(0.2 * (double)S, 3.0 * std::sqrt((double)S / s.r_eff)));
    if (M > ELPD_TAIL_CAP)
        return fail(-1, "%lld samples with r_eff = %g need a PSIS tail of M = %lld > %d samples: select fewer samples (thin=, chains=) "
                        "or give a larger r_eff", S, s.r_eff, M, ELPD_TAIL_CAP);
    if (s.n_samples) *s.n_samples = S;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const int n_rows = s.n_rows;
    double *d_lppd = nullptr, *d_pwaic = nullptr, *d_loo = nullptr, *d_khat = nullptr;
    long long* d_tail = nullptr;
    HIP_TRY(mem.alloc(&d_lppd, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_pwaic, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_loo, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_khat, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_tail, (size_t)n_rows));
    ElpdRed ra{};
    ra.O = O; ra.S = S; ra.M = (int)M;
    ra.lppd = d_lppd; ra.p_waic = d_pwaic; ra.elpd_loo = d_loo; ra.khat = d_khat; ra.tail_len = d_tail;
    auto copy_out = [&]() -> int {
        HIP_TRY(fetch(s.lppd, d_lppd, (size_t)n_rows, st));
        HIP_TRY(fetch(s.p_waic, d_pwaic, (size_t)n_rows, st));
        HIP_TRY(fetch(s.elpd_loo, d_loo, (size_t)n_rows, st));
        HIP_TRY(fetch(s.khat, d_khat, (size_t)n_rows, st));
        HIP_TRY(fetch((long long*)s.tail_len, d_tail, (size_t)n_rows, st));
        return wait_stream(h);
    };

    if (ll_src) {
        // source 3: every host sample is its own entry (repeats need no merging: the reduction depends on the multiset only)
        double* d_ll = nullptr;
        int* d_cnt = nullptr;
        HIP_TRY(mem.upload(&d_ll, s.loglik, (size_t)n_items * n_rows, st));
        std::vector<int32_t> ones(s.multiplicity ? 0 : (size_t)n_items, 1);
        HIP_TRY(mem.upload(&d_cnt, s.multiplicity ? s.multiplicity : ones.data(), (size_t)n_items, st));
        if (!s.multiplicity)
            if (int rc = wait_stream(h)) return rc;          // `ones` dies at the end of this block
        ra.mode = ELPD_HOST; ra.ll = d_ll; ra.ll_stride = n_rows; ra.cnt = d_cnt; ra.U = (int)n_items; ra.row0 = 0;
        hipLaunchKernelGGL(elpd_reduce_kernel, dim3((unsigned)n_rows), dim3(ELPD_THREADS), 0, st, ra);
        HIP_TRY(hipGetLastError());
        if (s.n_distinct) *s.n_distinct = n_items;
        return copy_out();
    }

    // data rows and targets
    const float* d_x = nullptr;
    int xs = 0;
    if (int rc = upload_rows(h, mem, rows, I + 1, &d_x, &xs)) return rc;
    // stage a: items -> distinct (w, eta) samples
    Distinct d;
    if (int rc = distinct_samples(h, mem, src, true, true, &d)) return rc;
    const int U = d.U;
    if (s.n_distinct) *s.n_distinct = U;
    // stage b + c in blocks of rows: fx scratch U x (rows x O) floats (+ U x rows doubles for loglik_out) under the budget
    const long long rows_blk = row_block(scratch_budget("PTNN_ELPD_SCRATCH_BYTES"),
                                         (size_t)U * (sizeof(float) * O + (s.loglik_out ? sizeof(double) : 0)), n_rows);
    float* d_fx = nullptr;
    double* d_llb = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * O * U));
    if (s.loglik_out) HIP_TRY(mem.alloc(&d_llb, (size_t)rows_blk * U));
    ForwardPlan fwd;
    if (int rc = fwd.init(h, "predictive accuracy")) return rc;
    std::vector<int> item_run;
    if (s.loglik_out) if (int rc = item_runs(h, d, n_items, &item_run)) return rc;
    ra.mode = reg ? ELPD_REG : ELPD_CLS; ra.fx = d_fx; ra.eta = d.run_eta; ra.y = d_x + I; ra.ys = xs; ra.cnt = d.run_cnt; ra.U = U;
    ra.ll_out = d_llb;
    for (long long r0 = 0; r0 < n_rows; r0 += rows_blk) {
        const int nr = (int)std::min<long long>(rows_blk, n_rows - r0);
        if (int rc = fwd.launch(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
        ra.row0 = (int)r0;
        hipLaunchKernelGGL(elpd_reduce_kernel, dim3((unsigned)nr), dim3(ELPD_THREADS), 0, st, ra);
        HIP_TRY(hipGetLastError());
        if (s.loglik_out) {
            const long long n_ll = (long long)nr * U;
            hipLaunchKernelGGL(elpd_loglik_kernel, dim3((unsigned)((n_ll + ELPD_THREADS - 1) / ELPD_THREADS)), dim3(ELPD_THREADS), 0, st, ra, nr);
            HIP_TRY(hipGetLastError());
            if (int rc = scatter_samples(h, (const double*)d_llb, nr, U, item_run, src.weights(), s.loglik_out, (size_t)n_rows, (size_t)r0)) return rc;
        }
    }
    return copy_out();
}

// ---- recursive forecasts (ptnn_dev_forecast.hpp) ----
int ptnn_forecast(ptnn_handle* h, const ptnn_forecast_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_forecast_spec")) return rc;
    const ptnn_forecast_spec& s = *spec;
    const bool host_src = s.w != nullptr, noise = s.noise != 0;
    SampleSource src = source_of(s, host_src, s.eta);
    const RowSource rows{s.origin_source, s.origins, s.n_origins, "origin_source", "PTNN_FORECAST_ORIGIN", "origins", "n_origins"};
    if (int rc = check_source(src, "vectors")) return rc;
    if (int rc = check_rows(rows)) return rc;
    if (s.n_origins < 1) return fail(-1, "n_origins = %d must be >= 1", s.n_origins);
    if (s.horizon < 1) return fail(-1, "horizon = %d must be >= 1", s.horizon);
    const long long ncols = (long long)s.n_origins * s.horizon;
    if (ncols > 0x7fffffffLL) return fail(-1, "%d origins x horizon %d = %lld columns: at most 2^31 - 1 per call", s.n_origins, s.horizon, ncols);
    if (int rc = check_ranks(s.n_ranks, s.ranks, s.order_stats)) return rc;
    if (noise && host_src && !s.eta) return fail(-1, "noise: host vectors need eta = log tau^2 (one per vector)");
    if (int rc = check_handle(h, "ptnn_forecast")) return rc;
    if (h->cfg.task != PTNN_TASK_REG || h->cfg.n_out != 1)
        return fail(-1, "forecasting needs a regression net with n_out == 1 (a one-step map of one series); this handle is a %s "
                        "net with n_out = %d", h->cfg.task == PTNN_TASK_REG ? "regression" : "classification", h->cfg.n_out);
    const int I = h->cfg.n_in, P = h->P, hz = s.horizon;
    if (int rc = fit_rows(h, rows)) return rc;
    if (int rc = count_samples(h, src)) return rc;
    const long long M = src.M;
    if (M < 1) return fail(-1, "the selection holds no sample");
    if (int rc = sample_limit(src)) return rc;
    if (int rc = check_rank_values(s.n_ranks, s.ranks, M)) return rc;
    if (s.n_samples) *s.n_samples = M;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    // origins
    const float* d_x = nullptr;
    int xs = 0;
    if (int rc = upload_rows(h, mem, rows, I, &d_x, &xs)) return rc;
    // stage a: items -> trajectories (noise off: distinct vectors; noise on: every occurrence, host multiplicities expanded)
    std::vector<float> w_exp, eta_exp;
    if (noise && host_src && s.multiplicity) {
        w_exp.reserve((size_t)M * P);
        eta_exp.reserve((size_t)M);
        for (int64_t k = 0; k < s.n_w; ++k)
            for (int c = 0; c < s.multiplicity[k]; ++c) {
                w_exp.insert(w_exp.end(), s.w + (size_t)k * P, s.w + (size_t)(k + 1) * P);
                eta_exp.push_back(s.eta[k]);
            }
        src.w = w_exp.data(); src.eta = eta_exp.data(); src.multiplicity = nullptr;
        src.n_items = M;
    }
    Distinct d;
    if (int rc = distinct_samples(h, mem, src, noise, !noise, &d)) return rc;
    const int U = d.U;
    if (s.n_trajectories) *s.n_trajectories = U;
    // outputs on the device for every column
    double* d_mean = nullptr; float* d_ostat = nullptr; long long* d_ranks = nullptr;
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    if (s.n_ranks) {
        HIP_TRY(mem.alloc(&d_ostat, (size_t)s.n_ranks * ncols));
        HIP_TRY(mem.upload(&d_ranks, (const long long*)s.ranks, (size_t)s.n_ranks, st));
    }
    // stage b + c in blocks of origins and horizon steps: fx 4 U ob hb bytes, + 4 U I bytes of carried windows when the horizon
    // is split (only with one origin per block: the columns of a block are then always contiguous)
    const size_t budget = scratch_budget("PTNN_FORECAST_SCRATCH_BYTES");
    const size_t traj_bytes = (size_t)U * sizeof(float);
    long long ob = 1, hb = hz;
    if (budget >= traj_bytes * hz) {
        ob = std::max(1LL, std::min<long long>((long long)(budget / (traj_bytes * hz)), s.n_origins));
    } else {
        const long long fit = (long long)(budget / traj_bytes) - I;
        hb = std::max(1LL, std::min<long long>(fit, hz));
    }
    ob = std::min<long long>(ob, 65535LL * WAVE);        // grid.y of the split layout
    const bool split_h = hb < hz;
    float *d_fx = nullptr, *d_win = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)ob * hb * U));
    if (split_h) HIP_TRY(mem.alloc(&d_win, (size_t)U * I));
    // the layout: a function of the shape alone (P), never of the budget
    const int layout = P <= FC_LANE_MAX_P ? FC_LANE : FC_SPLIT;
    const size_t lds = layout == FC_LANE ? (size_t)(FC_THREADS / WAVE) * P * WAVE * sizeof(float)
                                         : (size_t)(round_up4(P) + 2 * (FC_THREADS / WAVE) * WAVE) * sizeof(float);
    if (lds > 152 * 1024) return fail(-3, "forecast: a %d-parameter vector does not fit in LDS", P);
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(h->shape->forecast_fwd), lds)) return rc;
    // samples: the trajectory of every selected row, chain-major
    std::vector<int> item_run;
    if (s.samples) if (int rc = item_runs(h, d, src.n_items, &item_run)) return rc;
    ForecastFwd fa{};
    fa.base = d.base; fa.run_off = d.run_off; fa.eta = d.run_eta; fa.x = d_x; fa.xs = xs; fa.horizon = hz; fa.win = d_win;
    fa.H = h->cfg.n_hidden; fa.P = P; fa.U = U; fa.layout = layout; fa.noise = noise ? 1 : 0;
    fa.seed_lo = (uint32_t)(s.seed & 0xffffffffu); fa.seed_hi = (uint32_t)(s.seed >> 32); fa.fx = d_fx;
    for (long long r0 = 0; r0 < s.n_origins; r0 += ob) {
        const int nr = (int)std::min<long long>(ob, s.n_origins - r0);
        for (long long k0 = 0; k0 < hz; k0 += hb) {
            const int nk = (int)std::min<long long>(hb, hz - k0);
            fa.r0 = (int)r0; fa.nr = nr; fa.k0 = (int)k0; fa.hb = nk;
            dim3 grid;
            if (layout == FC_LANE) {
                const long long gx = (U + FC_THREADS - 1) / FC_THREADS;
                grid = dim3((unsigned)gx, (unsigned)std::max(1LL, std::min<long long>((512 + gx - 1) / gx, nr)));
            } else {
                grid = dim3((unsigned)U, (unsigned)((nr + WAVE - 1) / WAVE));
            }
            hipLaunchKernelGGL(h->shape->forecast_fwd, grid, dim3(FC_THREADS), lds, st, fa);
            HIP_TRY(hipGetLastError());
            const long long col0 = r0 * hz + k0;             // the block's columns are contiguous (see above)
            PredictRed ra{d_fx, d.run_cnt, U, 1, (int)col0, (int)ncols, M, s.n_ranks, d_ranks, d_mean, d_ostat, nullptr};
            hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)(nr * nk)), dim3(PRED_THREADS), 0, st, ra);
            HIP_TRY(hipGetLastError());
            if (s.samples)
                if (int rc = scatter_samples(h, d_fx, nr * nk, U, item_run, src.weights(), s.samples, (size_t)ncols, (size_t)col0)) return rc;
        }
    }
    HIP_TRY(fetch(s.mean, d_mean, (size_t)ncols, st));
    HIP_TRY(fetch(s.order_stats, d_ostat, (size_t)s.n_ranks * ncols, st));
    return wait_stream(h);
}

// ---- log evidence (ptnn_dev_evidence.hpp) ----
static_assert(PTNN_EVIDENCE_MAX_A == EVID_MAX_A, "ptnn.h prior exponents");

int ptnn_evidence(ptnn_handle* h, const ptnn_evidence_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_evidence_spec")) return rc;
    const ptnn_evidence_spec& s = *spec;
    const bool u_src = s.u != nullptr, host_src = s.w != nullptr;
    // host vectors [K][n][P] as one list of K n items (their [K, n] multiplicities are applied to U, below), or one rung per chain
    SampleSource src{host_src, s.w, nullptr, (int64_t)s.n_rungs * s.n_per_rung, nullptr, s.replicas, s.n_replicas, s.step0, s.nsteps, s.thin};
    if (u_src && host_src) return fail(-1, "give host vectors w or a host U, not both");
    if (u_src || host_src) {
        if (s.n_rungs < 1) return fail(-1, "n_rungs = %d must be >= 1", s.n_rungs);
        if (s.n_per_rung < 1) return fail(-1, "n_per_rung = %lld must be >= 1", (long long)s.n_per_rung);
    } else {
        if (s.nsteps < 1) return fail(-1, "no source: nsteps = %d trace rows, and neither host vectors w nor a host U", s.nsteps);
        if (int rc = check_source(src, "vectors")) return rc;
    }
    if (s.n_prior < 0) return fail(-1, "n_prior = %lld must be >= 0", (long long)s.n_prior);
    if (s.n_prior > 0x7fffffffLL) return fail(-1, "n_prior = %lld: at most 2^31 - 1 prior draws per call", (long long)s.n_prior);
    if (s.n_prior > 0 && (s.n_a < 1 || s.n_a > EVID_MAX_A || !s.a))
        return fail(-1, "n_prior = %lld prior draws need 1 to %d exponents a (n_a = %d)", (long long)s.n_prior, EVID_MAX_A, s.n_a);
    if (s.n_prior > 0)
        for (int j = 0; j < s.n_a; ++j)
            if (!std::isfinite(s.a[j])) return fail(-1, "a[%d] = %g is not finite", j, s.a[j]);
    if (s.n_prior == 0 && s.u_prior_out) return fail(-1, "u_prior_out requested with n_prior = 0");
    if (u_src && s.u_out) return fail(-1, "u_out: U is the input of this source");
    if (u_src && s.n_distinct) *s.n_distinct = 0;
    // host sources: items, their multiplicities, the draws of every rung
    std::vector<long long> off;                        // [K + 1] expanded draws of rung k at [off[k], off[k + 1])
    std::vector<int32_t> item_of;                      // expanded draw -> item (multiplicities only)
    if (u_src || host_src) {
        const long long K = s.n_rungs, n = s.n_per_rung;
        if (K * n > 0x7fffffffLL) return fail(-1, "%lld host rows: at most 2^31 - 1 per call", K * n);
        src.n_items = K * n;
        off.assign((size_t)K + 1, 0);
        for (long long k = 0; k < K; ++k) {
            long long c = 0;
            for (long long i = 0; i < n; ++i) {
                const long long it = k * n + i;
                const int mu = s.multiplicity ? s.multiplicity[it] : 1;
                if (mu < 0) return fail(-1, "multiplicity[%lld, %lld] = %d is negative", k, i, mu);
                c += mu;
                if (s.multiplicity) for (int r = 0; r < mu; ++r) item_of.push_back((int32_t)it);
                if (u_src && mu > 0 && !std::isfinite(s.u[it])) return fail(-1, "u[%lld, %lld] = %g is not finite", k, i, s.u[it]);
            }
            off[(size_t)k + 1] = off[(size_t)k] + c;
            if (off[(size_t)k + 1] > 0x7fffffffLL) return fail(-1, "more than 2^31 - 1 expanded draws");
        }
    }
    if (int rc = check_handle(h, "ptnn_evidence")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out, P = h->P, N = h->Ntr;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    // the trace selection: one rung per chain
    if (!u_src && !host_src) {
        if (int rc = count_samples(h, src)) return rc;
        if (src.n_items > 0x7fffffffLL) return fail(-1, "%lld trace rows: at most 2^31 - 1 per call", src.n_items);
        off.assign(src.reps.size() + 1, 0);
        for (size_t k = 0; k < src.reps.size(); ++k) off[k + 1] = off[k] + src.m;
    }
    const long long n_items = src.n_items;
    const int K = (int)off.size() - 1;
    for (int k = 0; k < K; ++k)
        if (off[(size_t)k + 1] - off[(size_t)k] < 4)
            return fail(-1, "rung %d holds %lld draws: the split ESS needs at least 4 per rung", k, off[(size_t)k + 1] - off[(size_t)k]);
    if (s.d)
        for (int k = 0; k < K; ++k)
            if (!std::isfinite(s.d[k])) return fail(-1, "d[%d] = %g is not finite", k, s.d[k]);
    const long long n_draws = off[(size_t)K];
    if (s.n_draws)
        for (int k = 0; k < K; ++k) s.n_draws[k] = off[(size_t)k + 1] - off[(size_t)k];

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const size_t budget = scratch_budget("PTNN_EVIDENCE_SCRATCH_BYTES");
    // the forward pass of predict_fwd on the training rows
    ForwardPlan fwd;
    if (int rc = fwd.init(h, "log evidence")) return rc;
    const float* d_x = h->d_data;                      // training rows
    const int xs = h->IPY;
    int* d_sse0 = nullptr;                             // weight vectors with SSE = 0 (evid_finish_kernel)
    HIP_TRY(mem.alloc(&d_sse0, 1));
    HIP_TRY(hipMemsetAsync(d_sse0, 0, sizeof(int), st));
    // U (and b) of `nv` vectors at base + run_off[u]: rows in blocks of rows_blk, fx scratch `fx` of rows_blk x O x nv floats
    auto eval_u = [&](const float* base, const long long* run_off, int nv, long long rows_blk, float* fx, double* acc, double* u_out,
                      double* b_out) -> int {
        HIP_TRY(hipMemsetAsync(acc, 0, (size_t)nv * sizeof(double), st));
        const unsigned ub = (unsigned)((nv + EVID_THREADS - 1) / EVID_THREADS);
        for (long long r0 = 0; r0 < N; r0 += rows_blk) {
            const int nr = (int)std::min<long long>(rows_blk, N - r0);
            if (int rc = fwd.launch(h, base, run_off, d_x, xs, (int)r0, nr, nv, fx)) return rc;
            EvidRows ra{fx, d_x + (size_t)r0 * xs + I, xs, nr, O, nv, reg ? 1 : 0, acc};
            hipLaunchKernelGGL(evid_rows_kernel, dim3(ub), dim3(EVID_THREADS), 0, st, ra);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(evid_finish_kernel, dim3(ub), dim3(EVID_THREADS), 0, st, nv, reg ? 1 : 0, N, (const double*)acc, u_out, b_out, d_sse0);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    auto rows_for = [&](long long nv, size_t avail) { return row_block(avail, (size_t)nv * O * sizeof(float), N); };
    auto sse_check = [&]() -> int {
        int e = 0;
        HIP_TRY(hipMemcpyAsync(&e, d_sse0, sizeof e, hipMemcpyDeviceToHost, st));
        if (int rc = wait_stream(h)) return rc;
        if (e) return fail(-1, "%d weight vectors fit the %d training rows exactly (SSE = 0): U = -(N / 2) log SSE is infinite", e, N);
        return 0;
    };

    // ---- the rungs: U of every draw
    double* d_udraw = nullptr;
    if (K > 0) HIP_TRY(mem.alloc(&d_udraw, (size_t)n_draws));
    int* d_item_of = nullptr;
    if (!item_of.empty()) HIP_TRY(mem.upload(&d_item_of, item_of.data(), item_of.size(), st));
    const unsigned draw_blocks = (unsigned)((n_draws + EVID_THREADS - 1) / EVID_THREADS);
    if (u_src) {
        double* d_u = nullptr;
        HIP_TRY(mem.upload(&d_u, s.u, (size_t)n_items, st));
        hipLaunchKernelGGL(evid_expand_kernel, dim3(draw_blocks), dim3(EVID_THREADS), 0, st, n_draws, (const int*)d_item_of,
                           (const int*)nullptr, (const double*)d_u, d_udraw);
        HIP_TRY(hipGetLastError());
    } else {
        // stage a: items -> distinct vectors
        Distinct d;
        if (int rc = distinct_samples(h, mem, src, false, true, &d)) return rc;
        const int U = d.U;
        if (s.n_distinct) *s.n_distinct = U;
        // stages b, c: U of every distinct vector, rows in blocks under the budget
        const long long rows_blk = rows_for(U, budget);
        float* d_fx = nullptr;
        double *d_acc = nullptr, *d_udist = nullptr;
        HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * O * U));
        HIP_TRY(mem.alloc(&d_acc, (size_t)U));
        HIP_TRY(mem.alloc(&d_udist, (size_t)U));
        if (int rc = eval_u(d.base, d.run_off, U, rows_blk, d_fx, d_acc, d_udist, nullptr)) return rc;
        hipLaunchKernelGGL(evid_expand_kernel, dim3(draw_blocks), dim3(EVID_THREADS), 0, st, n_draws, (const int*)d_item_of,
                           (const int*)d.item_run, (const double*)d_udist, d_udraw);
        HIP_TRY(hipGetLastError());
        if (int rc = sse_check()) return rc;
    }
    // stage d: per-rung moments and stones
    long long* d_off = nullptr;
    double *d_mean = nullptr, *d_var = nullptr, *d_d = nullptr, *d_ls = nullptr, *d_rv = nullptr;
    HIP_TRY(mem.upload(&d_off, off.data(), off.size(), st));
    HIP_TRY(mem.alloc(&d_mean, (size_t)K));
    HIP_TRY(mem.alloc(&d_var, (size_t)K));
    if (s.d) {
        HIP_TRY(mem.upload(&d_d, s.d, (size_t)K, st));
        HIP_TRY(mem.alloc(&d_ls, (size_t)K));
        HIP_TRY(mem.alloc(&d_rv, (size_t)K));
    }
    EvidRung rg{d_udraw, d_off, d_d, d_mean, d_var, d_ls, d_rv};
    hipLaunchKernelGGL(evid_rung_kernel, dim3((unsigned)K), dim3(EVID_THREADS), 0, st, rg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fetch(s.u_mean, d_mean, (size_t)K, st));
    HIP_TRY(fetch(s.u_var, d_var, (size_t)K, st));
    HIP_TRY(fetch(s.d ? s.log_stone : nullptr, d_ls, (size_t)K, st));
    HIP_TRY(fetch(s.d ? s.stone_relvar : nullptr, d_rv, (size_t)K, st));
    HIP_TRY(fetch(s.u_out, d_udraw, (size_t)n_draws, st));
    if (int rc = wait_stream(h)) return rc;
    // the split ESS of every rung's U draws (one chain each), by the convergence kernels: rungs of equal length in one pass
    if (s.u_ess) {
        std::vector<char> done((size_t)K, 0);
        for (int k0 = 0; k0 < K; ++k0) {
            if (done[(size_t)k0]) continue;
            const long long nk = off[(size_t)k0 + 1] - off[(size_t)k0];
            std::vector<int> rung, qcol;
            for (int k = k0; k < K; ++k)
                if (!done[(size_t)k] && off[(size_t)k + 1] - off[(size_t)k] == nk) { rung.push_back(k); done[(size_t)k] = 1; }
            const int Q = (int)rung.size();
            for (int q = 0; q < Q; ++q) qcol.push_back(q);
            DeviceScratch cm;
            int* d_rung = nullptr;
            float* d_draws = nullptr;
            HIP_TRY(cm.alloc(&d_rung, (size_t)Q));
            HIP_TRY(hipMemcpyAsync(d_rung, rung.data(), (size_t)Q * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_TRY(cm.alloc(&d_draws, (size_t)Q * nk));
            hipLaunchKernelGGL(evid_conv_kernel, dim3((unsigned)(((long long)Q * nk + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st,
                               Q, (int)nk, (const long long*)d_off, (const int*)d_rung, (const double*)d_udraw, d_draws);
            HIP_TRY(hipGetLastError());
            ConvGather ga{};
            ga.host = 1; ga.draws = d_draws; ga.Qh = Q;
            std::vector<double> ess((size_t)Q);
            if (int rc = conv_drive(h, cm, ga, qcol, 1, (int)nk, 0, nullptr, nullptr, nullptr, ess.data(), nullptr, nullptr, nullptr)) return rc;
            for (int q = 0; q < Q; ++q) s.u_ess[rung[(size_t)q]] = ess[(size_t)q];
        }
    }
    if (s.n_prior == 0) return 0;

    // ---- stage e: prior draws in blocks of nb vectors (vector + forward scratch of every training row under the budget)
    const long long NP = s.n_prior;
    const size_t per_draw = (size_t)P * sizeof(float) + 4 * sizeof(double) + (size_t)std::min<long long>(N, 65535LL * WAVE) * O * sizeof(float);
    const long long nb = std::max(1LL, std::min<long long>((long long)(budget / per_draw), NP));
    const size_t fixed = (size_t)nb * ((size_t)P * sizeof(float) + 4 * sizeof(double));
    const long long rows_blk = rows_for(nb, budget > fixed ? budget - fixed : 0);
    double *d_pu = nullptr, *d_pb = nullptr, *d_acc = nullptr, *d_a = nullptr;
    float *d_pw = nullptr, *d_fx = nullptr;
    long long* d_poff = nullptr;
    HIP_TRY(mem.alloc(&d_pu, (size_t)NP));
    HIP_TRY(mem.alloc(&d_pb, (size_t)NP));
    HIP_TRY(mem.alloc(&d_pw, (size_t)nb * P));
    HIP_TRY(mem.alloc(&d_poff, (size_t)nb));
    HIP_TRY(mem.alloc(&d_acc, (size_t)nb));
    HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * O * nb));
    const float sigma = (float)std::sqrt((double)h->cfg.sigma_squared);
    const uint32_t slo = (uint32_t)(s.seed & 0xffffffffu), shi = (uint32_t)(s.seed >> 32);
    const int nq = (P + 3) / 4;
    for (long long d0 = 0; d0 < NP; d0 += nb) {
        const int b = (int)std::min<long long>(nb, NP - d0);
        hipLaunchKernelGGL(evid_prior_kernel, dim3((unsigned)(((long long)b * nq + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st,
                           d0, b, P, sigma, slo, shi, d_pw, d_poff);
        HIP_TRY(hipGetLastError());
        if (int rc = eval_u(d_pw, d_poff, b, rows_blk, d_fx, d_acc, d_pu + d0, d_pb + d0)) return rc;
    }
    HIP_TRY(mem.alloc(&d_a, (size_t)s.n_a));
    HIP_TRY(hipMemcpyAsync(d_a, s.a, (size_t)s.n_a * sizeof(double), hipMemcpyHostToDevice, st));
    double* d_pr = nullptr;
    HIP_TRY(mem.alloc(&d_pr, (size_t)4 * s.n_a));
    EvidPriorRed pr{d_pu, d_pb, NP, d_a, d_pr, d_pr + s.n_a, d_pr + 2 * s.n_a, d_pr + 3 * s.n_a};
    hipLaunchKernelGGL(evid_prior_reduce_kernel, dim3((unsigned)s.n_a), dim3(EVID_THREADS), 0, st, pr);
    HIP_TRY(hipGetLastError());
    std::vector<double> prh((size_t)4 * s.n_a);
    HIP_TRY(hipMemcpyAsync(prh.data(), d_pr, prh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (s.u_prior_out) HIP_TRY(hipMemcpyAsync(s.u_prior_out, d_pu, (size_t)NP * sizeof(double), hipMemcpyDeviceToHost, st));
    if (int rc = sse_check()) return rc;
    double* outs[4] = {s.prior_log_mean_exp, s.prior_kish_ess, s.prior_u_mean, s.prior_u_var};
    for (int o = 0; o < 4; ++o)
        if (outs[o]) std::copy(prh.begin() + (size_t)o * s.n_a, prh.begin() + (size_t)(o + 1) * s.n_a, outs[o]);
    return 0;
}

// ---- calibration (ptnn_dev_calibration.hpp) ----
static_assert(PTNN_CALIB_MAX_LEVELS == CALIB_MAX_LEVELS && PTNN_CALIB_MAX_DISTINCT == CALIB_MAX_DISTINCT, "ptnn.h calibration limits");

int ptnn_calibration(ptnn_handle* h, const ptnn_calibration_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_calibration_spec")) return rc;
    const ptnn_calibration_spec& s = *spec;
    const bool host_src = s.w != nullptr;
    SampleSource src = source_of(s, host_src, s.eta);
    const RowSource rows{s.x_source, s.x, s.n_rows, "x_source", "PTNN_PREDICT_X", "x", "n_rows"};
    if (!src.host && s.nsteps < 1) return fail(-1, "no source: nsteps = %d trace rows and no host vectors w", s.nsteps);
    if (int rc = check_source(src, "samples")) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    if (int rc = check_rows(rows)) return rc;
    if (s.n_levels < 0 || s.n_levels > CALIB_MAX_LEVELS) return fail(-1, "n_levels = %d outside [0, %d]", s.n_levels, CALIB_MAX_LEVELS);
    if (s.n_levels > 0 && (!s.levels_p || !s.levels_z || !s.quantiles))
        return fail(-1, "n_levels = %d needs levels_p, levels_z and quantiles", s.n_levels);
    if (s.quantiles && s.n_levels == 0) return fail(-1, "quantiles requested without levels");
    for (int k = 0; k < s.n_levels; ++k)
        if (!(s.levels_p[k] > 0.0 && s.levels_p[k] < 1.0) || !std::isfinite(s.levels_z[k]))
            return fail(-1, "levels_p[%d] = %g (levels_z %g): a quantile level lies in (0, 1)", k, s.levels_p[k], s.levels_z[k]);
    if (s.crps && !s.pair_term) return fail(-1, "crps requested without pair_term");
    if (src.host)
        if (int rc = count_samples(nullptr, src)) return rc;
    if (int rc = check_handle(h, "ptnn_calibration")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    const bool reg_out = s.pit || s.crps || s.pred_mean || s.pred_sd || s.quantiles || s.pair_term;
    if (reg_out && (!reg || O != 1))
        return fail(-1, "pit, crps, pred_mean, pred_sd and quantiles need a regression net with n_out == 1; this handle is a %s net "
                        "with n_out = %d", reg ? "regression" : "classification", O);
    if (s.p_mean && reg) return fail(-1, "p_mean: a regression has no class probabilities");
    if (host_src && reg && !s.eta) return fail(-1, "a regression's host vectors need eta = log tau^2 (one per vector)");
    if (int rc = fit_rows(h, rows)) return rc;
    if (!src.host)
        if (int rc = count_samples(h, src)) return rc;
    const long long S = src.M;
    if (S < 1) return fail(-1, "the selection holds no sample");
    if (int rc = sample_limit(src)) return rc;
    if (s.n_samples) *s.n_samples = S;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const int n_rows = s.n_rows;
    const float* d_x = nullptr;
    int xs = 0;
    if (int rc = upload_rows(h, mem, rows, I + 1, &d_x, &xs)) return rc;
    // stage a: items -> distinct (w, eta) samples (a classification's: distinct w, as ptnn_predict's)
    Distinct d;
    if (int rc = distinct_samples(h, mem, src, reg, true, &d)) return rc;
    const int U = d.U;
    if (s.n_distinct) *s.n_distinct = U;
    if (s.pair_term && U > CALIB_MAX_DISTINCT)
        return fail(-1, "%d distinct samples: the pair term of the CRPS takes at most %d (U^2 / 2 terms per data row); select fewer "
                        "samples (thin=, chains=) or leave the CRPS out (crps=False)", U, CALIB_MAX_DISTINCT);
    const long long rows_blk = row_block(scratch_budget("PTNN_CALIB_SCRATCH_BYTES"), (size_t)U * sizeof(float) * O, n_rows);
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * O * U));
    ForwardPlan fwd;
    if (int rc = fwd.init(h, "calibration")) return rc;

    if (!reg) {
        double* d_mean = nullptr;
        HIP_TRY(mem.alloc(&d_mean, (size_t)n_rows * O));
        for (long long r0 = 0; r0 < n_rows; r0 += rows_blk) {
            const int nr = (int)std::min<long long>(rows_blk, n_rows - r0);
            if (int rc = fwd.launch(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
            PredictRed ra{d_fx, d.run_cnt, U, O, (int)r0 * O, n_rows * O, S, 0, nullptr, d_mean, nullptr, nullptr};
            hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)(nr * O)), dim3(PRED_THREADS), 0, st, ra);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(fetch(s.p_mean, d_mean, (size_t)n_rows * O, st));
        return wait_stream(h);
    }

    double *d_tau2 = nullptr, *d_tau = nullptr, *d_itau = nullptr;
    double *d_pit = nullptr, *d_crps = nullptr, *d_mean = nullptr, *d_sd = nullptr, *d_q = nullptr, *d_t1 = nullptr, *d_bound = nullptr;
    unsigned long long* d_limbs = nullptr;
    HIP_TRY(mem.alloc(&d_tau2, (size_t)U));
    HIP_TRY(mem.alloc(&d_tau, (size_t)U));
    HIP_TRY(mem.alloc(&d_itau, (size_t)U));
    HIP_TRY(mem.alloc(&d_pit, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_mean, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_sd, (size_t)n_rows));
    if (s.n_levels) HIP_TRY(mem.alloc(&d_q, (size_t)s.n_levels * n_rows));
    if (s.pair_term) {
        HIP_TRY(mem.alloc(&d_crps, (size_t)n_rows));
        HIP_TRY(mem.alloc(&d_t1, (size_t)n_rows));
        HIP_TRY(mem.alloc(&d_bound, (size_t)n_rows));
        HIP_TRY(mem.alloc(&d_limbs, (size_t)n_rows * 4));
        HIP_TRY(hipMemsetAsync(d_limbs, 0, (size_t)n_rows * 4 * sizeof(unsigned long long), st));
    }
    hipLaunchKernelGGL(calib_tau_kernel, dim3((unsigned)((U + CALIB_THREADS - 1) / CALIB_THREADS)), dim3(CALIB_THREADS), 0, st, U,
                       (const float*)d.run_eta, d_tau2, d_tau, d_itau);
    HIP_TRY(hipGetLastError());
    CalibRow ra{};
    ra.fx = d_fx; ra.tau2 = d_tau2; ra.tau = d_tau; ra.itau = d_itau; ra.cnt = d.run_cnt; ra.y = d_x + I; ra.ys = xs; ra.U = U;
    ra.n_rows = n_rows; ra.S = S; ra.n_levels = s.n_levels; ra.pair = s.pair_term ? 1 : 0;
    for (int k = 0; k < s.n_levels; ++k) { ra.p[k] = s.levels_p[k]; ra.z[k] = s.levels_z[k]; }
    ra.pit = d_pit; ra.pred_mean = d_mean; ra.pred_sd = d_sd; ra.quantiles = d_q; ra.term1 = d_t1; ra.pair_bound = d_bound;
    const int n_tiles = (U + CALIB_THREADS - 1) / CALIB_THREADS;
    CalibPair pa{d_fx, d_tau2, d.run_cnt, d_bound, U, 0, 0, n_tiles, d_limbs};
    const unsigned n_tri = (unsigned)((long long)n_tiles * (n_tiles + 1) / 2);
    for (long long r0 = 0; r0 < n_rows; r0 += rows_blk) {
        const int nr = (int)std::min<long long>(rows_blk, n_rows - r0);
        if (int rc = fwd.launch(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
        ra.row0 = (int)r0;
        hipLaunchKernelGGL(calib_row_kernel, dim3((unsigned)nr), dim3(CALIB_THREADS), 0, st, ra);
        HIP_TRY(hipGetLastError());
        // the pair term of this block's rows, at most 65535 rows (grid.y) per launch
        for (int q0 = 0; s.pair_term && q0 < nr; q0 += 65535) {
            pa.row0 = (int)r0; pa.r0 = q0;
            hipLaunchKernelGGL(calib_pair_kernel, dim3(n_tri, (unsigned)std::min(65535, nr - q0)), dim3(CALIB_THREADS), 0, st, pa);
            HIP_TRY(hipGetLastError());
        }
    }
    if (s.pair_term) {
        hipLaunchKernelGGL(calib_finish_kernel, dim3((unsigned)((n_rows + CALIB_THREADS - 1) / CALIB_THREADS)), dim3(CALIB_THREADS), 0, st,
                           n_rows, (const unsigned long long*)d_limbs, (const double*)d_t1, (const double*)d_bound, S, d_crps);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(fetch(s.pit, d_pit, (size_t)n_rows, st));
    HIP_TRY(fetch(s.pred_mean, d_mean, (size_t)n_rows, st));
    HIP_TRY(fetch(s.pred_sd, d_sd, (size_t)n_rows, st));
    HIP_TRY(fetch(s.quantiles, d_q, (size_t)s.n_levels * n_rows, st));
    HIP_TRY(fetch(s.crps, d_crps, (size_t)n_rows, st));
    return wait_stream(h);
}

static int run_model(ptnn_handle* h, int mode, const float* w_in, const float* tau_sq, int n, float* out, size_t out_floats,
                     int a0, int a1) {
    if (!h) return fail(-1, "null handle");
    if (!h->have_data) return fail(-1, "ptnn_set_data has not been called");
    if (n < 1) return fail(-1, "n must be >= 1");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    float *d_w = nullptr, *d_tau = nullptr, *d_out = nullptr;
    const int P = h->P;
    if (w_in) {
        HIP_TRY(hipMalloc(&d_w, (size_t)n * P * sizeof(float)));
        HIP_TRY(hipMemcpy(d_w, w_in, (size_t)n * P * sizeof(float), hipMemcpyHostToDevice));
    }
    if (tau_sq) {
        HIP_TRY(hipMalloc(&d_tau, (size_t)n * sizeof(float)));
        HIP_TRY(hipMemcpy(d_tau, tau_sq, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMalloc(&d_out, out_floats * sizeof(float)));
    HIP_TRY(hipMemsetAsync(d_out, 0, out_floats * sizeof(float), h->stream));
    const SegParams p = h->seg_params();
    // mode 4 (ptnn_time_tree_round): ONE input row, but 9 blocks -- blocks 0 and 8 share an XCD under the round-robin dispatch
    hipLaunchKernelGGL(h->plan.wide() ? h->shape->model_wide : h->shape->model, dim3(mode == 4 ? 9 : n), dim3(h->plan.model_threads), h->plan.model_lds, h->stream, p,
                       mode, d_w, d_tau, d_out, a0, a1);
    HIP_TRY(hipGetLastError());
    if (int rc = wait_stream(h)) return rc;
    HIP_TRY(hipMemcpy(out, d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost));
    if (d_w) (void)hipFree(d_w);
    if (d_tau) (void)hipFree(d_tau);
    (void)hipFree(d_out);
    return 0;
}

int ptnn_evaluate(ptnn_handle* h, const float* w, const float* tau_sq, int n, float* out) {
    if (!w || !out) return fail(-1, "null argument");
    if (h && h->cfg.task == PTNN_TASK_REG && !tau_sq) return fail(-1, "regression needs tau_sq");
    return run_model(h, 0, w, tau_sq, n, out, (size_t)n * 8, 0, 0);
}

int ptnn_langevin_gradient(ptnn_handle* h, const float* w_in, int n, float* w_out) {
    if (!w_in || !w_out) return fail(-1, "null argument");
    return run_model(h, 1, w_in, nullptr, n, w_out, (size_t)n * (h ? h->P : 0), 0, 0);
}

int ptnn_time_sgd_epoch(ptnn_handle* h, const float* w, int reps, double* ms_per_epoch) {
    if (!h || !w || !ms_per_epoch || reps < 1) return fail(-1, "bad argument");
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    if (int rc = run_model(h, 3, w, nullptr, 1, out, 4, reps, 0)) return rc;
    int khz = 0;
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device_id));
    if (khz <= 0) return fail(-2, "the device reports no wall clock rate");
    auto ticks = [&](int k) {
        unsigned lo, hi;
        std::memcpy(&lo, &out[k], 4); std::memcpy(&hi, &out[k + 1], 4);
        return (double)(((unsigned long long)hi << 32) | lo);
    };
    ms_per_epoch[0] = ticks(0) / (double)khz / (double)reps;
    // wide nets (n_hidden > 64): [1] = a PAIR of epochs through one row loop (sgd_sweep_wide_pair); narrow nets: 0
    ms_per_epoch[1] = h->plan.wide() ? ticks(2) / (double)khz / (double)reps : 0.0;
    return 0;
}

int ptnn_time_tree_round(ptnn_handle* h, const float* w, int reps, int xcd_local, double* ms) {
    if (!h || !w || !ms || reps < 1) return fail(-1, "bad argument");
    if (h->plan.wide()) return fail(-3, "the prefetching tree runs nets of up to 64 hidden units");
    float out[64] = {0.f};
    if (int rc = run_model(h, 4, w, nullptr, 1, out, 64, reps, xcd_local ? 1 : 0)) return rc;
    int khz = 0;
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device_id));
    if (khz <= 0) return fail(-2, "the device reports no wall clock rate");
    if (out[4] != 1.0f) return fail(-2, "the granule round trips between two work-groups timed out");
    auto ticks = [&](int k) {
        unsigned lo, hi;
        std::memcpy(&lo, &out[k], 4); std::memcpy(&hi, &out[k + 1], 4);
        return (double)(((unsigned long long)hi << 32) | lo);
    };
    ms[0] = ticks(0) / (double)khz / (double)reps;             // one forward pass + likelihood + prior sums of a whole work-group
    ms[1] = ticks(2) / (double)khz / (double)reps / 2.0;       // one granule, one way (half a round trip)
    ms[2] = (double)out[5];                                    // 1: the round trips went through the XCD's L2
    return 0;
}

int ptnn_tape(ptnn_handle* h, int replica, int step, float* noise, float* scal) {
    if (!h || !noise || !scal) return fail(-1, "null argument");
    // narrow nets return {noise[P], scal[3]}; the wide kernel writes whole float4s: {noise[PS], scal[3]}
    const size_t off = h->plan.wide() ? (size_t)h->PS : (size_t)h->P;
    std::vector<float> buf(off + 3);
    if (int rc = run_model(h, 2, nullptr, nullptr, 1, buf.data(), buf.size(), replica, step)) return rc;
    std::memcpy(noise, buf.data(), h->P * sizeof(float));
    std::memcpy(scal, buf.data() + off, 3 * sizeof(float));
    return 0;
}

int ptnn_describe(ptnn_handle* h, char* buf, int nbytes) {
    if (!h || !buf || nbytes < 1) return fail(-1, "bad argument");
    if (!h->have_data) return fail(-1, "ptnn_set_data has not been called (the schedule depends on the data set)");
    const LaunchPlan& pl = h->plan;
    const void* fn = reinterpret_cast<const void*>(segment_function(h->shape, pl.kind));
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, pl.threads, pl.seg_lds));
    hipFuncAttributes fa{};
    HIP_TRY(hipFuncGetAttributes(&fa, fn));
    const int slots = pl.kind == SEG_COOP ? 1
                    : pl.kind == SEG_SPEC ? pl.groups * (pl.threads / WAVE)
                    : pl.kind == SEG_TREE ? tree_depth(pl.groups)                              // the steps committed per round
                    : pl.wide() ? (pl.groups > 1 && h->cfg.use_langevin ? 8 : pl.groups)
                    : pack_slots(pl.pk_nred) * pl.groups;
    const int n = std::snprintf(buf, (size_t)nbytes,
                                "{\"kernel\": \"ptnn::%s<%d,%d,%d>\", \"schedule\": \"%s\", \"grid_blocks\": %d, \"block_threads\": %d, "
                                "\"lds_bytes\": %zu, \"groups_per_replica\": %d, \"slots_per_round\": %d, \"num_cus\": %d, "
                                "\"blocks_per_cu\": %d, \"vgprs\": %d, \"scratch_bytes\": %zu, \"forward_mfma\": %d, \"exchange\": \"%s\", \"lds_resident_state\": %d, \"compact_traces\": %d, \"launches\": \"%s\"}",
                                g_seg[pl.kind].name, h->cfg.task, h->cfg.n_in, h->cfg.n_out,
                                pl.wide() && pl.groups > 1 ? "speculative-wide" : g_seg[pl.kind].label,
                                pl.grid(h->cfg.n_replicas_local), pl.threads, pl.seg_lds, pl.groups, slots, h->num_cus, per_cu, fa.numRegs, (size_t)fa.localSizeBytes,
                                pl.fw_mfma ? pl.fw_mfma : ((pl.wide() && h->cfg.n_hidden % 32 == 0) ? 1 : 0),
                                h->comm.kind == COMM_NONE ? "none" : (h->cfg.label_swap ? "labels" : (resolved_xchg_mode(h) == PTNN_XCHG_GATHER ? "gather" : "boundary")),
                                pl.kind == SEG_WIDE_RES ? 1 : 0, pl.compact ? 1 : 0,
                                (pl.persistent && h->comm.kind == COMM_NONE) ? "one per ptnn_run (swap rounds inside)" : "one per swap interval");
    if (n < 0 || n >= nbytes) return fail(-1, "buffer of %d bytes is too small for the description", nbytes);
    return n;
}

int ptnn_kernel_time(ptnn_handle* h, int reset, int64_t* launches, double* total_ms) {
    if (!h) return fail(-1, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = wait_stream(h)) return rc;
    collect_timing(h);
    if (launches) *launches = h->timed_launches;
    if (total_ms) *total_ms = h->timed_ms;
    if (reset) { h->timed_launches = 0; h->timed_ms = 0.0; }
    return 0;
}

int ptnn_debug_stamps(ptnn_handle* h, uint64_t* out16) {   // 160 entries: 16 phase sums + 64 x (cycles, rounds)
    if (!h || !out16) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = wait_stream(h)) return rc;
    HIP_TRY(hipMemcpy(out16, h->d_stamps, 160 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(h->d_stamps, 0, 160 * sizeof(unsigned long long)));
    const unsigned long long big = ~0ull;
    HIP_TRY(hipMemcpy(h->d_stamps + 12, &big, sizeof big, hipMemcpyHostToDevice));
    return 0;
}

// exactly one floating conversion: % [flags] [width] [.precision] (e|E|f|F|g|G)
static bool float_format_ok(const char* fmt) {
    const size_t fl = std::strlen(fmt);
    bool ok = fl >= 2 && fl < 16 && fmt[0] == '%' && std::strchr("eEfFgG", fmt[fl - 1]) != nullptr;
    for (size_t k = 1; ok && k + 1 < fl; ++k) ok = std::strchr("0123456789.+- #", fmt[k]) != nullptr;
    // width and precision stay far inside the 400-byte slot ptnn_savetxt formats a value into
    for (size_t k = 1; ok && k + 1 < fl;) {
        if (fmt[k] >= '0' && fmt[k] <= '9') {
            long v = 0;
            while (k + 1 < fl && fmt[k] >= '0' && fmt[k] <= '9') v = v * 10 + (fmt[k++] - '0');
            ok = v <= 40;
        } else ++k;
    }
    return ok;
}

int ptnn_text_round(double* values, int64_t n, const char* fmt) {
    if (!values || !fmt || n < 0) return fail(-1, "bad argument");
    if (!float_format_ok(fmt)) return fail(-1, "unsupported format '%s'", fmt);
    const ptnn_text::Format f = ptnn_text::parse_format(fmt);
    for (int64_t k = 0; k < n; ++k) values[k] = ptnn_text::round_trip(values[k], f);
    return 0;
}

int ptnn_text_round_f32(const float* in, double* out, int64_t n, const char* fmt) {
    if (!in || !out || !fmt || n < 0) return fail(-1, "bad argument");
    if (!float_format_ok(fmt)) return fail(-1, "unsupported format '%s'", fmt);
    const ptnn_text::Format f = ptnn_text::parse_format(fmt);
    for (int64_t k = 0; k < n; ++k) out[k] = ptnn_text::round_trip((double)in[k], f);
    return 0;
}

}  // extern "C" (the row writer below is a template)

// rows [0, rows) of a matrix as np.savetxt writes them; value(r, c) yields the double to print, same_as_prev(r) whether row r
// repeats row r - 1 bit for bit (its text is then copied, not formatted again)
template <class Value, class SameAsPrev>
static int write_text_rows(const char* path, int64_t rows, int64_t cols, const char* fmt, bool append, Value value, SameAsPrev same_as_prev) {
    if (!float_format_ok(fmt)) return fail(-1, "unsupported format '%s'", fmt);
    const ptnn_text::Format f = ptnn_text::parse_format(fmt);
    FILE* fp = std::fopen(path, append ? "a" : "w");
    if (!fp) return fail(-4, "cannot open %s for writing", path);
    std::setvbuf(fp, nullptr, _IONBF, 0);                      // the block below is the buffer
    const size_t line_cap = (size_t)cols * 401 + 2;
    // no larger than the file can get, and not value-initialised: most of a run's files are a few KB
    const size_t buf_size = std::max<size_t>(std::min<size_t>(4u << 20, (size_t)std::max<int64_t>(rows, 1) * line_cap), 2 * line_cap);
    const std::unique_ptr<char[]> buf_mem(new char[buf_size]), line_mem(new char[line_cap]);
    struct Span { char* p; size_t n; char* data() const { return p; } size_t size() const { return n; } };
    const Span buf{buf_mem.get(), buf_size}, line{line_mem.get(), line_cap};
    size_t used = 0, line_len = 0;
    for (int64_t r = 0; r < rows; ++r) {
        if (r == 0 || !same_as_prev(r)) {
            char* o = line.data();
            for (int64_t c = 0; c < cols; ++c) {
                if (c) *o++ = ' ';
                o = ptnn_text::put_value(o, value(r, c), f);
            }
            *o++ = '\n';
            line_len = (size_t)(o - line.data());
        }
        if (buf.size() - used < line_len) {
            if (std::fwrite(buf.data(), 1, used, fp) != used) { std::fclose(fp); return fail(-4, "write to %s failed", path); }
            used = 0;
        }
        std::memcpy(buf.data() + used, line.data(), line_len);
        used += line_len;
    }
    const bool wrote = std::fwrite(buf.data(), 1, used, fp) == used;
    if (std::fclose(fp) != 0 || !wrote) return fail(-4, "write to %s failed", path);
    return 0;
}

extern "C" {

int ptnn_savetxt(const char* path, const double* data, int64_t rows, int64_t cols, const char* fmt) {
    if (!path || !data || !fmt) return fail(-1, "null argument");
    if (rows < 0 || cols < 1) return fail(-1, "bad shape %lld x %lld", (long long)rows, (long long)cols);
    return write_text_rows(path, rows, cols, fmt, false, [&](int64_t r, int64_t c) { return data[r * cols + c]; },
                           [&](int64_t r) { return std::memcmp(data + r * cols, data + (r - 1) * cols, (size_t)cols * sizeof(double)) == 0; });
}

int ptnn_savetxt_f32(const char* path, const float* data, int64_t rows, int64_t cols, int64_t row_stride, const char* fmt, int append) {
    if (!path || !data || !fmt) return fail(-1, "null argument");
    if (rows < 0 || cols < 1 || row_stride < cols) return fail(-1, "bad shape %lld x %lld (row stride %lld)", (long long)rows, (long long)cols, (long long)row_stride);
    return write_text_rows(path, rows, cols, fmt, append != 0, [&](int64_t r, int64_t c) { return (double)data[r * row_stride + c]; },
                           [&](int64_t r) { return std::memcmp(data + r * row_stride, data + (r - 1) * row_stride, (size_t)cols * sizeof(float)) == 0; });
}

int ptnn_savetxt_f32_batch(int n_files, const char* const* paths, const float* const* data, const int64_t* rows, const int64_t* cols,
                           const int64_t* row_stride, const char* const* fmts, int append, int threads) {
    if (n_files < 0 || (n_files && (!paths || !data || !rows || !cols || !row_stride || !fmts))) return fail(-1, "null argument");
    const int T = std::max(1, std::min(threads, n_files));
    std::atomic<int> next{0}, bad{-1};
    std::mutex mu;
    std::string why;
    auto work = [&]() {
        for (int k = next.fetch_add(1); k < n_files; k = next.fetch_add(1)) {
            if (ptnn_savetxt_f32(paths[k], data[k], rows[k], cols[k], row_stride[k], fmts[k], append) < 0) {
                std::lock_guard<std::mutex> lock(mu);
                if (bad.load() < 0) { bad.store(k); why = g_err; }     // g_err is per thread: carry the first cause to the caller's
            }
        }
    };
    if (T == 1) work();
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(work);
        for (auto& x : th) x.join();
    }
    if (bad.load() >= 0) return fail(-4, "%s", why.c_str());
    return 0;
}

int ptnn_posterior_matrix(const float* pos_w, int64_t n_chains, int64_t n_rows, int64_t n_param, int64_t row_floats, int64_t first_row, double* out, int threads) {
    // out[p][c * m + t] = pos_w[c][first_row + t][p], m = n_rows - first_row: the (P, R (S - b)) float64 matrix show_results
    // returns (REG:795-797, 848: np.loadtxt of every chain's pos_w file, burn-in cut, chains side by side, transposed)
    if (!pos_w || !out || n_chains < 1 || n_param < 1 || row_floats < n_param || first_row < 0 || first_row > n_rows) return fail(-1, "bad argument");
    const int64_t m = n_rows - first_row;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n_chains));
    auto work = [&](int t) {
        for (int64_t c = t; c < n_chains; c += T) {
            const float* src = pos_w + (c * n_rows + first_row) * row_floats;
            // blocks of rows: the block's source (bt x P floats) stays in cache while it is read P times with stride P
            for (int64_t t0 = 0; t0 < m; t0 += 256) {
                const int64_t bt = std::min<int64_t>(256, m - t0);
                for (int64_t p = 0; p < n_param; ++p) {
                    double* dst = out + p * (n_chains * m) + c * m + t0;
                    const float* s = src + t0 * row_floats + p;
                    for (int64_t k = 0; k < bt; ++k) dst[k] = (double)s[k * row_floats];
                }
            }
        }
    };
    if (T == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(work, t);
        for (auto& x : th) x.join();
    }
    return 0;
}

}  // extern "C"
