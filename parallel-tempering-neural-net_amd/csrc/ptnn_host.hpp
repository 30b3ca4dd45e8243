// ptnn_host.hpp -- what the host translation units of libptnn.so share (ptnn.hip, ptnn_analysis.hip, ptnn_checkpoint.hip,
// ptnn_text.hip): the error text, the handle, and the few functions of ptnn.hip that the others call.  Internal: never installed,
// not included by ptnn_shape.hip, and nothing declared here is visible outside the library.  It includes no device code (Shape
// and SegParams are only named), so the text side can use it without the kernels.
#pragma once
#include "ptnn_comm.hpp"
#include "ptnn_dims.hpp"
#include "../../include/ptnn.h"

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

namespace ptnn {

struct Shape;           // ptnn_shapes.hpp
struct SegParams;       // ptnn_device.hpp

extern thread_local std::string g_err;      // the text behind ptnn_last_error; one object for the whole library (ptnn.hip)

int fail(int code, const char* fmt, ...);   // sets g_err, returns code

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            (void)hipGetLastError(); /* reported here: must not surface again at the next launch check */   \
            return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
        }                                                                                                  \
    } while (0)

constexpr size_t LDS_MAX = 160 * 1024;          // LDS of one work-group
constexpr size_t LDS_CEILING = 152 * 1024;      // largest dynamic-LDS ceiling the runtime accepts (just below LDS_MAX it refuses)

enum SegKind { SEG_COOP, SEG_SPEC, SEG_PACK, SEG_PACKM, SEG_TREE, SEG_WIDE, SEG_WIDE_RES, SEG_KINDS };   // the segment kernels

// What ptnn_set_data decided: the segment kernel, its launch shape and the buffers it needs (plan_launch)
struct LaunchPlan {
    SegKind kind = SEG_COOP;
    int threads = 64, model_threads = 64;       // segment kernel; model_kernel / model_wide_kernel (ptnn_evaluate and friends)
    size_t seg_lds = 0, model_lds = 0;
    int groups = 1;                 // work-groups (CUs) per replica; tree: 2^depth - 1
    int pk_nred = 3;                // packed schedules: lane-group width 2^3 (H <= 8) or 2^4 hidden units
    int pack_hc = 0;                // packed schedules: the hidden width compiled into the kernel taken (0: the run-time-width kernel)
    int fw_mfma = 0;                // forward pass on the matrix cores: 1 exact fp32, 2 split bf16 operands
    bool xy_global = false;         // split forward pass: no room for the row-major data image in LDS, its rare readers go to global memory
    bool tree_ahead = false;        // tree: room in LDS for two sets of tapes
    bool compact = false;           // wide nets with all trace rows resident: rejected steps record a row index, no pos_w row
    int blocks_per_cu = 0;          // occupancy of the segment kernel as the runtime reports it (0 = not queried)
    bool persistent = false;        // all work-groups of the grid are resident: ptnn_run queues ONE launch, swap rounds inside
    bool swap_pipeline = false;     // ... and those rounds are pipelined (replica k waits for 0 .. k+1, no grid barrier): plan_persistent
    int delay_replica = -1;         // $PTNN_SWAP_DELAY="r:t" (tests): replica r idles delay_us microseconds before it posts a pipelined round
    int delay_us = 0;
    // bytes of the buffers the plan needs (0 = none): multi-group exchange slots / rows / verdicts, in-launch swap granules, wide scratch
    size_t xslots = 0, xw = 0, xverdict = 0, xswap = 0, wide_scratch = 0;
    bool wide() const { return kind == SEG_WIDE || kind == SEG_WIDE_RES; }
    int grid(int replicas) const;   // ptnn.hip (the kernel table says which kinds have `groups` work-groups per replica)
};

}  // namespace ptnn

struct ptnn_handle {
    ptnn_config cfg{};
    const ptnn::Shape* shape = nullptr;
    hipStream_t stream = nullptr;
    int P = 0, PS = 0, PW = 0, IPY = 0, FWS = 0, Ntr = 0, Nte = 0;
    ptnn::LaunchPlan plan;
    unsigned* d_barrier = nullptr;  // grid barrier of the persistent launch: one slot per work-group
    int barrier_slots = 0;
    float* d_swap_ring = nullptr;   // pipelined swap rounds: [SWAP_RING_DEPTH][R][ring row] posted rows ...
    unsigned* d_swap_tags = nullptr;    // ... and ready[R] | taken[R], zeroed before every launch
    int swap_ring_replicas = 0;
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
    ptnn::Comm comm;
    std::vector<ptnn::RowMsg> route;
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

    ptnn::SegParams seg_params() const;     // ptnn.hip
};

// the functions of ptnn.hip that the other host translation units call
namespace ptnn {

int check_ready(ptnn_handle* h);                            // data and state are set
int wait_stream(ptnn_handle* h);                            // everything queued on the handle's stream has run (bounded with RCCL)
int finish_stream(ptnn_handle* h);                          // wait_stream + the device's error flag
int raise_lds_limit(const void* func, size_t bytes);        // the dynamic-LDS ceiling of a kernel, only ever raised
int ladder_adapt_alloc(ptnn_handle* h, const ptnn_ladder_adapt_spec& spec);     // ptnn_checkpoint_load restores an adaptation

}  // namespace ptnn

#pragma GCC visibility pop
