// ptnn.hip -- host side of libptnn.so, the sampler and the communicators: the C ABI of include/ptnn.h over the gfx950 kernels of
// ptnn_device.hpp.  (Analysis calls: ptnn_analysis.hip; checkpoint / resume: ptnn_checkpoint.hip; text output: ptnn_text.hip.)
// Replaces, for the hot path only, what the reference does with one forked ptReplica process per chain plus the
// parent's swap loop (REG = multicore-pt-regression/pt_timeseries_regression.py:223-485, 659-771;
// CLS = multicore-pt-classification/pt_classification.py:232-494, 668-776).
#include "ptnn_shapes.hpp"
namespace ptnn {
#include "ptnn_dev_swap.hpp"                 // xchg_pack_kernel, chain_reset_kernel, swap_kernel
}  // namespace ptnn
#include "ptnn_host.hpp"

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

thread_local std::string ptnn::g_err;

int ptnn::fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// one table per shape, each defined in its own translation unit (ptnn_shape.hip)
#define X_DECL(T, I, O) extern "C" const ptnn::Shape ptnn_shape_##T##_##I##_##O;
PTNN_SHAPES(X_DECL)
#undef X_DECL
// ... and one entry per fixed-width packed kernel, each in a translation unit of its own too (ptnn_shape.hip with -DPTNN_HC)
#define X_DECL(T, I, O, H) extern "C" const ptnn::PackFixed ptnn_pack_fixed_##T##_##I##_##O##_##H;
PTNN_PACK_FIXED(X_DECL)
#undef X_DECL
#define X_DECL(T, I, O, H) extern "C" const ptnn::PackFixed ptnn_packm_fixed_##T##_##I##_##O##_##H;
PTNN_PACKM_FIXED(X_DECL)
#undef X_DECL

namespace {

#define X_ENTRY(T, I, O) &ptnn_shape_##T##_##I##_##O,
const Shape* const g_shapes[] = {PTNN_SHAPES(X_ENTRY)};
#undef X_ENTRY
#define X_ENTRY(T, I, O, H) &ptnn_pack_fixed_##T##_##I##_##O##_##H,
const PackFixed* const g_pack_fixed[] = {PTNN_PACK_FIXED(X_ENTRY) nullptr};     // (the list may be empty: a diagnostic build of one shape)
#undef X_ENTRY
#define X_ENTRY(T, I, O, H) &ptnn_packm_fixed_##T##_##I##_##O##_##H,
const PackFixed* const g_packm_fixed[] = {PTNN_PACKM_FIXED(X_ENTRY) nullptr};
#undef X_ENTRY
constexpr int MAX_HIDDEN = MAX_WAVES * WAVE;    // wide nets: one thread per hidden unit

const Shape* find_shape(int task, int I, int O) {
    for (const Shape* s : g_shapes)
        if (s->task == task && s->I == I && s->O == O) return s;
    return nullptr;
}

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

}  // namespace

int LaunchPlan::grid(int replicas) const { return replicas * (g_seg[kind].per_group ? groups : 1); }

SegParams ptnn_handle::seg_params() const {
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

namespace {

inline int tree_depth(int groups) { int d = 0; while ((1 << (d + 1)) - 1 <= groups) ++d; return d; }   // groups = 2^d - 1

// Q10: REG hands off after step i when i % si == 0 and i != 0 (REG:427); CLS when (i+1) % si == 0 (CLS:438)
inline bool swap_trigger(const ptnn_config& c, int i) {
    if (c.task == PTNN_TASK_REG) return (i % c.swap_interval == 0) && i != 0;
    return ((i + 1) % c.swap_interval) == 0;
}

seg_fn segment_function(const Shape* sh, SegKind k) { return sh->*g_seg[k].fn; }

// the shape's packed kernel (multi: over several CUs) with the hidden width H compiled in, or null (PTNN_PACK_FIXED, PTNN_PACKM_FIXED)
seg_fn pack_fixed_function(const Shape* sh, int H, bool multi) {
    for (const PackFixed* const* f = multi ? g_packm_fixed : g_pack_fixed; *f; ++f)
        if ((*f)->task == sh->task && (*f)->I == sh->I && (*f)->O == sh->O && (*f)->H == H) return (*f)->pack;
    return nullptr;
}
// the kernel a plan launches
seg_fn plan_function(const Shape* sh, const LaunchPlan& plan) {
    const bool packed = plan.kind == SEG_PACK || plan.kind == SEG_PACKM;
    return (packed && plan.pack_hc > 0) ? pack_fixed_function(sh, plan.pack_hc, plan.kind == SEG_PACKM) : segment_function(sh, plan.kind);
}

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

}  // namespace

int ptnn::ladder_adapt_alloc(ptnn_handle* h, const ptnn_ladder_adapt_spec& spec) {
    ladder_adapt_release(h);
    const size_t R = h->cfg.n_replicas_global;
    HIP_TRY(hipMalloc(&h->d_lad_hist, (size_t)(spec.rounds + 1) * R * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_lad_s, 2 * (R - 1) * sizeof(double)));
    HIP_TRY(hipMalloc(&h->d_lad_acc, (size_t)h->max_rounds * (R - 1) * sizeof(float)));
    h->adapt = spec; h->have_adapt = true;
    return 0;
}

namespace {

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

// Do the in-launch swap rounds of this handle take the pipelined path now?  The plan says whether the kernel and the configuration
// allow it; what can change after planning is asked here: a communicator (its rounds run between launches) and ladder adaptation
// (it needs the whole round's statistics in one place).
bool swap_pipelined(const ptnn_handle* h) {
    return h->plan.persistent && h->plan.swap_pipeline && h->comm.kind == COMM_NONE && !h->have_adapt;
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
    pp.delay_replica = -1;
    if (swap_inside && swap_pipelined(h)) {
        // the ring of posted rows and the two counters per replica of the pipelined rounds (swap_handoff)
        const int R = h->cfg.n_replicas_global;
        const int row = swap_ring_row_floats(h->PS);
        if (R > h->swap_ring_replicas) {
            for (void* q : {(void*)h->d_swap_ring, (void*)h->d_swap_tags})
                if (q) HIP_TRY(hipFree(q));
            h->d_swap_ring = nullptr; h->d_swap_tags = nullptr; h->swap_ring_replicas = 0;
            HIP_TRY(hipMalloc(&h->d_swap_ring, (size_t)SWAP_RING_DEPTH * R * (row + 1) * sizeof(float)));     // the rows, then the posted scalars
            HIP_TRY(hipMalloc(&h->d_swap_tags, (size_t)2 * R * sizeof(unsigned)));
            h->swap_ring_replicas = R;
        }
        HIP_TRY(hipMemsetAsync(h->d_swap_tags, 0, (size_t)2 * R * sizeof(unsigned), h->stream));
        pp.pipeline = 1; pp.ring_row = row; pp.ring = h->d_swap_ring; pp.ring_L = h->d_swap_ring + (size_t)SWAP_RING_DEPTH * R * row; pp.ready = h->d_swap_tags; pp.taken = h->d_swap_tags + R;
        if (h->plan.delay_replica >= 0 && h->plan.delay_us > 0) {
            int khz = 0;
            HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device_id));
            if (khz > 0) { pp.delay_replica = h->plan.delay_replica; pp.delay_ticks = (unsigned)((long long)h->plan.delay_us * khz / 1000); }
        }
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
    hipLaunchKernelGGL(plan_function(h->shape, h->plan), dim3(grid), dim3(h->plan.threads), h->plan.seg_lds, h->stream, p, pp, begin);
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

}  // namespace

// The dynamic-LDS ceiling of a kernel is a property of the function, shared by every handle of the process: only ever raise
// it, so that a handle created later with a smaller data set does not pull it below what an earlier one launches with.
int ptnn::raise_lds_limit(const void* func, size_t bytes) {
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

// Whether a work-group of `fn` can have `bytes` of LDS: within LDS_MAX, and the runtime grants the ceiling (just below 160 KiB it
// refuses; the refusal's error is cleared).  For the plans that have something smaller to go on with.
static bool lds_accepted(seg_fn fn, size_t bytes) {
    return bytes <= LDS_MAX && ptnn::raise_lds_limit(reinterpret_cast<const void*>(fn), bytes) == 0;
}

// Wait for everything queued on the handle's stream.  With an RCCL communicator attached the wait is bounded: a collective
// whose peer never arrives would otherwise block the host for ever (the reference's parent at least polls is_alive() every
// round, REG:721-727).  "No progress" = the stream is busy and the device has not completed a swap round (swap_kernel stores the
// round count into a pinned host word) for comm_timeout_s() seconds; a long segment between two rounds is far below that.
int ptnn::wait_stream(ptnn_handle* h) {
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
int ptnn::finish_stream(ptnn_handle* h) {
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

namespace {

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
    // The kernel with this hidden width compiled in where the shape has one (one CU: 4-5-1, 5-5-1; several: 4-10-1), unless
    // $PTNN_PACK_FIXED_H=0 asks for the run-time-width kernels (the comparison path of the tests and of an A/B run).  The lengths such a
    // kernel forms at compile time are ptnn_dims.hpp's, like the handle's: checked below, since the kernel would not notice.
    const char* const fixed_env = std::getenv("PTNN_PACK_FIXED_H");
    auto fixed = [&](bool multi) { return !(fixed_env && fixed_env[0] == '0') && pack_fixed_function(h.shape, H, multi) != nullptr; };
    {
        const int Pc = dims_P(c.n_in, H, c.n_out);
        if ((fixed(false) || fixed(true)) &&
            (h.P != Pc || h.PS != dims_PS(Pc) || h.PW != dims_PW(Pc) || h.FWS != dims_FWS(c.n_in, c.n_out) || h.IPY != dims_IPY(c.n_in) ||
             plan.pk_nred != pack_nred(H)))
            return fail(-3, "the handle's row lengths (P %d, PS %d, PW %d, FWS %d, IPY %d) are not the ones compiled into the fixed-width "
                            "packed kernel of %d hidden units", h.P, h.PS, h.PW, h.FWS, h.IPY, H);
    }
    const seg_fn packm_fn = fixed(true) ? pack_fixed_function(h.shape, H, true) : segment_function(h.shape, SEG_PACKM);
    int G = 1;
    const size_t pkm = pack_multi_lds_floats(Nall, h.IPY, h.PS, H, h.FWS, pack_slots(plan.pk_nred)) * sizeof(float);
    if (fits && pkm <= LDS_MAX && c.use_langevin && !c.shared_device && (sched == PTNN_SCHED_PACKED || c.schedule == PTNN_SCHED_AUTO) &&
        c.waves_per_replica == 0) {
        const int want = c.groups_per_replica;
        if (want == 2 || want == 4) G = want;                       // (8-lane groups: on request only -- 16 slots on one CU already)
        else if (want == 0 && plan.pk_nred == 4) { if (Rl * 4 <= h.num_cus) G = 4; else if (Rl * 2 <= h.num_cus) G = 2; }
        // The runtime refuses a dynamic-LDS ceiling just below 160 KiB (6-16-18 with 65 rows: 159.9 KiB over several CUs, next to
        // the kernel's 256 B of static LDS): ask it.
        // A refused automatic choice goes on with one CU per replica, a refused request is an error.
        if (G > 1 && !lds_accepted(packm_fn, pkm)) {
            if (want == 2 || want == 4)
                return fail(-3, "the packed round over %d CUs needs %zu B of LDS, which the runtime does not grant one work-group", want, pkm);
            G = 1;
        }
    }
    const bool pays = (H <= 8) || G > 1 || Rl * 4 > h.num_cus;
    if (sched != PTNN_SCHED_PACKED &&
        !(c.schedule == PTNN_SCHED_AUTO && sched == PTNN_SCHED_SPECULATIVE && fits && pays && c.use_langevin && c.waves_per_replica == 0 &&
          (c.groups_per_replica == 0 || G > 1)))
        return 0;
    const seg_fn pack_fn = fixed(false) ? pack_fixed_function(h.shape, H, false) : segment_function(h.shape, SEG_PACK);
    if (G == 1 && !lds_accepted(pack_fn, pk)) {
        if (sched == PTNN_SCHED_PACKED) return fail(-3, "the packed schedule needs %zu B of LDS, which the runtime does not grant one work-group", pk);
        return 0;
    }
    plan.kind = G > 1 ? SEG_PACKM : SEG_PACK;
    plan.pack_hc = fixed(G > 1) ? H : 0;
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
    const seg_fn spec = segment_function(h.shape, SEG_SPEC);
    auto fits = [&](int k) { return lds_accepted(spec, lds(k)); };
    int k = nw ? nw : (G > 1 ? 4 : 8);
    while (k > 1 && !fits(k)) k >>= 1;
    if (nw && k != nw) {
        if (c.schedule == PTNN_SCHED_AUTO) k = 0;      // auto: fall back to the cooperative schedule
        else return fail(-3, "speculative schedule with %d waves needs more than 160 KiB of LDS", nw);
    }
    if (k * G > MAX_SLOTS) return fail(-1, "waves x groups must not exceed %d", MAX_SLOTS);
    if (k == 0 || !fits(k)) return 0;
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
    const void* fn = reinterpret_cast<const void*>(plan_function(h.shape, plan));
    if (int rc = raise_lds_limit(fn, plan.seg_lds)) return rc;
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, plan.threads, plan.seg_lds));
    plan.persistent = (long long)plan.grid(c.n_replicas_local) <= (long long)per_cu * h.num_cus;
    // Pipelined swap rounds (swap_handoff): the one-CU packed kernel, the reference's cascade, the chains themselves moving, the whole
    // ladder on this device.  The cooperative and the wide kernels share the loop but keep the grid barrier: they have not been
    // measured on the new path.  $PTNN_SWAP_PIPELINE=0: the barrier everywhere (the A/B switch).
    const char* pe = std::getenv("PTNN_SWAP_PIPELINE");
    plan.swap_pipeline = plan.persistent && !(pe && pe[0] == '0') && plan.kind == SEG_PACK && plan.grid(1) == 1 && c.swap_rule == 0 &&
                         !c.label_swap && c.n_replicas_local == R;
    // $PTNN_SWAP_DELAY="r:t" (tests): replica r idles t microseconds before it posts.  t is capped at SWAP_DELAY_MAX_US = 5000: a
    // waiter gives up after SPIN_LIMIT = 2^22 polls of at least 0.5 us each (a sleep and a round trip to L2), i.e. not before two
    // seconds, and the SWAP_RING_DEPTH + 2 = 6 delayed rounds a waiter can at most sit out in one wait come to 30 ms.
    if (const char* de = std::getenv("PTNN_SWAP_DELAY")) {
        constexpr int SWAP_DELAY_MAX_US = 5000;
        int r = -1, t = 0;
        if (std::sscanf(de, "%d:%d", &r, &t) == 2 && r >= 0 && r < R && t > 0) { plan.delay_replica = r; plan.delay_us = std::min(t, SWAP_DELAY_MAX_US); }
    }
    return 0;
}

// The launch plan of a handle for a data set of Nall rows: a function of the config, the data shape and the device ($PTNN_PERSISTENT
// and $PTNN_PACK_FIXED_H aside).  Queries the runtime (occupancy, dynamic-LDS ceilings), never writes to the handle; 0 or the refusal.
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
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(plan_function(h.shape, plan)), plan.seg_lds)) return rc;
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
    packed.assign((size_t)(Nall + 2 + 4) * IPY, 0.0f);             // two zero rows: look-ahead of the SGD sweep (the kernels copy these
                                                                   // Nall + 2 rows into LDS); four more for sweep_rows_reg41, whose scalar loads fetch
                                                                   // the global image in pairs of rows up to row Ntr + 5
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

}  // namespace

int ptnn::check_ready(ptnn_handle* h) {
    if (!h) return fail(-1, "null handle");
    if (!h->have_data) return fail(-1, "ptnn_set_data has not been called");
    if (!h->have_state) return fail(-1, "ptnn_set_state has not been called");
    return 0;
}

namespace {
// everything of ptnn_create that can fail after the handle exists: the caller destroys the handle on a non-zero return
int create_buffers(ptnn_handle* h, const ptnn_config* cfg, const Shape* sh, const hipDeviceProp_t& prop) {
    h->cfg = *cfg;
    h->shape = sh;
    h->num_cus = prop.multiProcessorCount;
    if (const char* ts = std::getenv("PTNN_TIMING_STRIDE")) h->timing_stride = std::atoi(ts);
    const int I = cfg->n_in, H = cfg->n_hidden, O = cfg->n_out;
    h->P = dims_P(I, H, O);
    h->PS = dims_PS(h->P);                                 // ptnn_dims.hpp: the formulas a fixed-width kernel evaluates at compile time
    h->PW = dims_PW(h->P);
    h->IPY = dims_IPY(I);
    h->FWS = dims_FWS(I, O);
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
                    h->d_L_handoff, h->d_L_final, h->d_L_raw, h->d_prior_post, h->d_temps_global, h->d_pos_w, h->d_scal, h->d_src, h->d_label[0], h->d_label[1], h->d_slot_of[0], h->d_slot_of[1], h->d_src_log, h->d_counters, h->d_error, h->d_xslots, h->d_xw, h->d_xverdict, h->d_xswap, h->d_stamps, h->d_wide_scratch, h->d_xt, h->d_xs, h->d_barrier, h->d_swap_ring, h->d_swap_tags};
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
    const void* fn = reinterpret_cast<const void*>(plan_function(h->shape, pl));
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    char width[16] = "";                                   // a compiled-in hidden width is the kernel's fourth template argument
    if ((pl.kind == SEG_PACK || pl.kind == SEG_PACKM) && pl.pack_hc > 0) std::snprintf(width, sizeof width, ",%d", pl.pack_hc);
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, pl.threads, pl.seg_lds));
    hipFuncAttributes fa{};
    HIP_TRY(hipFuncGetAttributes(&fa, fn));
    const int slots = pl.kind == SEG_COOP ? 1
                    : pl.kind == SEG_SPEC ? pl.groups * (pl.threads / WAVE)
                    : pl.kind == SEG_TREE ? tree_depth(pl.groups)                              // the steps committed per round
                    : pl.wide() ? (pl.groups > 1 && h->cfg.use_langevin ? 8 : pl.groups)
                    : pack_slots(pl.pk_nred) * pl.groups;
    // how a swap round is run: inside the launch -- pipelined, at the grid barrier, or by the kernel's own granule exchange (tree,
    // packed over several CUs) -- or by swap_kernel / the communicator between two launches
    const bool inside = pl.persistent && h->comm.kind == COMM_NONE;
    const bool pipelined = swap_pipelined(h);
    const char* const swap_rounds = !inside ? "between launches" : pipelined ? "pipelined (ring 4)"
                                    : (pl.kind == SEG_TREE || pl.kind == SEG_PACKM) ? "in-kernel exchange" : "grid barrier";
    static_assert(SWAP_RING_DEPTH == 4, "describe() spells the ring depth out");
    const int n = std::snprintf(buf, (size_t)nbytes,
                                "{\"kernel\": \"ptnn::%s<%d,%d,%d%s>\", \"schedule\": \"%s\", \"grid_blocks\": %d, \"block_threads\": %d, "
                                "\"lds_bytes\": %zu, \"groups_per_replica\": %d, \"slots_per_round\": %d, \"num_cus\": %d, "
                                "\"blocks_per_cu\": %d, \"vgprs\": %d, \"scratch_bytes\": %zu, \"forward_mfma\": %d, \"exchange\": \"%s\", \"lds_resident_state\": %d, \"compact_traces\": %d, \"launches\": \"%s\", \"swap_rounds\": \"%s\", \"swap_ring_depth\": %d}",
                                g_seg[pl.kind].name, h->cfg.task, h->cfg.n_in, h->cfg.n_out, width,
                                pl.wide() && pl.groups > 1 ? "speculative-wide" : g_seg[pl.kind].label,
                                pl.grid(h->cfg.n_replicas_local), pl.threads, pl.seg_lds, pl.groups, slots, h->num_cus, per_cu, fa.numRegs, (size_t)fa.localSizeBytes,
                                pl.fw_mfma ? pl.fw_mfma : ((pl.wide() && h->cfg.n_hidden % 32 == 0) ? 1 : 0),
                                h->comm.kind == COMM_NONE ? "none" : (h->cfg.label_swap ? "labels" : (resolved_xchg_mode(h) == PTNN_XCHG_GATHER ? "gather" : "boundary")),
                                pl.kind == SEG_WIDE_RES ? 1 : 0, pl.compact ? 1 : 0,
                                (pl.persistent && h->comm.kind == COMM_NONE) ? "one per ptnn_run (swap rounds inside)" : "one per swap interval",
                                swap_rounds, pipelined ? (int)SWAP_RING_DEPTH : 0);
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

}  // extern "C"
