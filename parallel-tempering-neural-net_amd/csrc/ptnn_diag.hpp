// ptnn_diag.hpp -- DIAGNOSTIC BUILD ONLY (-DPTNN_STAMPS; profiles/tools/build_stamps.sh).  Never part of the product: ptnn_device.hpp
// includes this file only when PTNN_STAMPS is defined, otherwise STAMP / STAMP_SUB / STAMP_MH / FW_DBG / PTNN_DIAG expand to nothing.
//
// In-kernel cycle stamps: wave 0 of the first work-group of replica 0 adds up shader-clock cycles per phase of a round and writes
// the sums to SegParams::stamps at the end of the launch (ptnn_debug_stamps reads and resets them; profiles/tools/stamps*.py print
// them).  The hook bodies below are pasted into the kernels by name (PTNN_DIAG(name)) and use the local names of the place they
// are pasted into (tid, lane, wave, p, r, grp, ...).
#pragma once

#define PTNN_DIAG(name) PTNN_DIAG_##name

#define STAMP(slot)                                                                          \
    do {                                                                                     \
        if (stamp_on) {                                                                      \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                      \
            __builtin_amdgcn_s_waitcnt(0xC07F);                                              \
            stamp_acc[slot] += t_ - stamp_last; stamp_last = t_;                             \
        }                                                                                    \
    } while (0)

// A point inside a phase: the cycles from the phase's start (the last STAMP) up to here, every LDS read before it landed.  It does
// not move the phase's start, so the phase table reads the same with and without such points.
#define STAMP_SUB(slot)                                                                      \
    do {                                                                                     \
        if (stamp_on) {                                                                      \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                      \
            __builtin_amdgcn_s_waitcnt(0xC07F);                                              \
            stamp_sub[slot] += t_ - stamp_last;                                              \
        }                                                                                    \
    } while (0)

// The two points inside Metropolis-Hastings, behind a switch of their own (-DPTNN_STAMPS_MH, e.g. EXTRA=-DPTNN_STAMPS_MH
// build_stamps.sh): each drains the LDS queue in the middle of the phase, and the two cost it about 0.6 k cycles of 1.5 k, so a
// plain -DPTNN_STAMPS build stamps the phase as it runs.  Point 0: what the verdict reads that does not wait for the epochs has
// landed -- the slot's scalars sl_, the step's tape scalars sc_, w_cur w_ (l_: the lane within its 16-lane row) -- point 1: the
// verdict is computed.
#ifdef PTNN_STAMPS_MH
#define STAMP_MH(slot) STAMP_SUB(slot)
#define STAMP_MH_OPERANDS(sl_, sc_, w_, l_)                                                  \
    do {                                                                                     \
        if (stamp_on) {                                                                      \
            const float a_ = (sl_)[SL_LIKPROP] + (sl_)[SL_PRIORPROP] + (sl_)[SL_LG] + (sl_)[SL_D2] + (sl_)[SL_ADAPT] + (sc_)[1] + \
                             (w_)[l_] + (w_)[16 + (l_)];                                     \
            asm volatile("" :: "v"(a_));                                                     \
        }                                                                                    \
        STAMP_SUB(0);                                                                        \
    } while (0)
#else
#define STAMP_MH(slot) do { } while (0)
#define STAMP_MH_OPERANDS(sl_, sc_, w_, l_) do { } while (0)
#endif

// cycles of the phases of eval_rows_mfma_coop / eval_rows_mfma_split (block 0, wave 0)
static __device__ unsigned long long fw_dbg[8];
#define FW_DBG(q_) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                        fw_dbg[q_] += t_ - fw_t; fw_t = t_; } } while (0)

#define PTNN_DIAG_fw_begin \
    unsigned long long fw_t = __builtin_amdgcn_s_memtime();

#define PTNN_DIAG_coop_begin \
    const bool stamp_on = (blockIdx.x == 0 && tid < WAVE); \
    unsigned long long stamp_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long stamp_last = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F); \
    const unsigned long long stamp_t0 = stamp_last;

#define PTNN_DIAG_coop_flush \
    if (stamp_on && (tid & 63) == 0 && p.stamps) { \
        for (int q_ = 0; q_ < 9; ++q_) atomicAdd(p.stamps + q_, stamp_acc[q_]); \
        atomicAdd(p.stamps + 9, (unsigned long long)n_steps); \
        atomicAdd(p.stamps + 10, __builtin_amdgcn_s_memtime() - stamp_t0); \
        if (tid == 0) for (int q_ = 0; q_ < 8; ++q_) { atomicAdd(p.stamps + 150 + q_, fw_dbg[q_]); fw_dbg[q_] = 0; } \
    }

#define PTNN_DIAG_spec_entry \
    const unsigned long long stamp_entry = __builtin_amdgcn_s_memrealtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F);

#define PTNN_DIAG_spec_begin \
    const bool stamp_on = (blockIdx.x == 0 && wave == 0); \
    unsigned long long stamp_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long stamp_last = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F); \
    unsigned long long stamp_rounds = 0; \
    const unsigned long long stamp_t0 = stamp_last; \
    const unsigned long long stamp_rt0 = __builtin_amdgcn_s_memrealtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F);

#define PTNN_DIAG_count_round \
    stamp_rounds += 1;

#define PTNN_DIAG_spec_flush \
    if (stamp_on && lane == 0 && p.stamps) { \
        for (int q_ = 0; q_ < 9; ++q_) atomicAdd(p.stamps + q_, stamp_acc[q_]); \
        atomicAdd(p.stamps + 9, stamp_rounds); \
        atomicAdd(p.stamps + 10, __builtin_amdgcn_s_memtime() - stamp_t0); \
        atomicAdd(p.stamps + 11, __builtin_amdgcn_s_memrealtime() - stamp_rt0); \
    } \
    if (tid == 0 && p.stamps) { \
        const unsigned long long now = __builtin_amdgcn_s_memrealtime(); \
        atomicMin(p.stamps + 12, stamp_entry); \
        atomicMax(p.stamps + 13, stamp_rt0 - stamp_entry); \
        atomicMax(p.stamps + 14, now - stamp_rt0); \
        atomicMax(p.stamps + 15, now); \
    } \
    if (grp == 0 && tid == 0 && p.stamps && r < 64) { \
        atomicAdd(p.stamps + 16 + 2 * r, __builtin_amdgcn_s_memtime() - stamp_t0); \
        atomicAdd(p.stamps + 17 + 2 * r, stamp_rounds); \
    }

#define PTNN_DIAG_pack_begin \
    const bool stamp_on = (blockIdx.x == 0 && wave == 0); \
    unsigned long long stamp_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long stamp_sub[7] = {0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long stamp_last = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F); \
    unsigned long long stamp_rounds = 0, stamp_eval = 0, stamp_arrive = 0; \
    const unsigned long long stamp_t0 = stamp_last;

#define PTNN_DIAG_pack_eval_begin \
    const unsigned long long ev_t0 = __builtin_amdgcn_s_memtime();

// Arrival at the barrier behind the forward passes: wave 0 (sweep) and the first forward wave each add up the clock they arrive at
// (sums wrap; their difference does not), so (sum of wave 0) - (sum of the forward wave) over the rounds is the time the forward
// wave waits there for the sweep waves: the slack a shorter sweep path can use.
#define PTNN_DIAG_pack_eval_end \
    { \
        const unsigned long long ev_t1 = __builtin_amdgcn_s_memtime(); \
        if (ev_i == 0) stamp_eval += ev_t1 - ev_t0; \
        if (blockIdx.x == 0 && (ev_i == 0 || wave == 0)) stamp_arrive += ev_t1; \
    }

// The two points around the hand-scheduled row loop of the packed sweep (sgd_sweep<PROP>): cycles from the phase's start (STAMP(2))
// to the first instruction of the asm block and to the first one behind it.  Each drains the LDS queue, like every STAMP_SUB.
#define PTNN_DIAG_sweep_fields \
    bool diag_on = false; unsigned long long diag_last = 0; unsigned long long* diag_sub = nullptr;
#define PTNN_DIAG_pack_sweep_args \
    pp.diag_on = stamp_on; pp.diag_last = stamp_last; pp.diag_sub = stamp_sub + 5;
#define PTNN_DIAG_SWEEP_POINT(q_) \
    if constexpr (PROP) { \
        if (pp->diag_on) { \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
            __builtin_amdgcn_s_waitcnt(0xC07F); \
            pp->diag_sub[q_] += t_ - pp->diag_last; \
        } \
    }
#define PTNN_DIAG_sweep_asm_begin PTNN_DIAG_SWEEP_POINT(0)
#define PTNN_DIAG_sweep_asm_end PTNN_DIAG_SWEEP_POINT(1)

#define PTNN_DIAG_pack_flush \
    if (stamp_on && lane == 0 && p.stamps) { \
        for (int q_ = 0; q_ < 9; ++q_) atomicAdd(p.stamps + q_, stamp_acc[q_]); \
        atomicAdd(p.stamps + 9, stamp_rounds); \
        atomicAdd(p.stamps + 10, __builtin_amdgcn_s_memtime() - stamp_t0); \
    } \
    if (stamp_on && lane == 0 && p.stamps) for (int q_ = 0; q_ < 5; ++q_) atomicAdd(p.stamps + 144 + q_, stamp_sub[q_]); \
    if (stamp_on && lane == 0 && p.stamps) {                /* 150 ..: the cooperative kernel's fw_dbg, which this kernel never writes */ \
        atomicAdd(p.stamps + 150, stamp_sub[5]); atomicAdd(p.stamps + 151, stamp_sub[6]); atomicAdd(p.stamps + 152, stamp_arrive); \
    } \
    if (blockIdx.x == 0 && ev_i == 0 && lane == 0 && p.stamps) { atomicAdd(p.stamps + 11, stamp_eval); atomicAdd(p.stamps + 153, stamp_arrive); } \
    if (tid == 0 && p.stamps && r < 64) { \
        atomicAdd(p.stamps + 16 + 2 * r, __builtin_amdgcn_s_memtime() - stamp_t0); \
        atomicAdd(p.stamps + 17 + 2 * r, stamp_rounds); \
    }

// The boundary between two swap intervals of the pipelined rounds (swap_handoff and the packed body around it), thread 0 of
// replica 0: cycles from the end of the body's round loop to the release of `ready` (0: write-back, post, drain), on to the end of
// the poll (1: the wait for replicas 0 and 1), to the release of `taken` (2: uniforms, cascade, take, drain), to the barrier behind
// staging and the state load of the re-entered body (3) and to the head of its round loop (4: the tape ring); [5] counts the
// boundaries, [6] is the last stamp, [7] says that a hand-off lies behind the entry.  Flushed with the body's other stamps into
// stamps[154 .. 159]; profiles/tools/stamps_pack.py prints them.
static __device__ unsigned long long bd_dbg[8];
#define PTNN_BD_POINT(q_) \
    if (blockIdx.x == 0 && threadIdx.x == 0) { \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_s_waitcnt(0xC07F); \
        if ((q_) >= 0) bd_dbg[(q_) < 0 ? 0 : (q_)] += t_ - bd_dbg[6]; \
        bd_dbg[6] = t_; \
    }
#define PTNN_DIAG_bd_loop_end PTNN_BD_POINT(-1)
#define PTNN_DIAG_bd_ready PTNN_BD_POINT(0)
#define PTNN_DIAG_bd_polled PTNN_BD_POINT(1)
#define PTNN_DIAG_bd_taken PTNN_BD_POINT(2) if (blockIdx.x == 0 && threadIdx.x == 0) { bd_dbg[5] += 1; bd_dbg[7] = 1; }
#define PTNN_DIAG_bd_staged if (blockIdx.x == 0 && threadIdx.x == 0 && bd_dbg[7]) { PTNN_BD_POINT(3) }
#define PTNN_DIAG_bd_loop_head if (blockIdx.x == 0 && threadIdx.x == 0 && bd_dbg[7]) { PTNN_BD_POINT(4) bd_dbg[7] = 0; }
#define PTNN_DIAG_bd_flush \
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.stamps) \
        for (int q_ = 0; q_ < 6; ++q_) { atomicAdd(p.stamps + 154 + q_, bd_dbg[q_]); bd_dbg[q_] = 0; }

#define PTNN_DIAG_tree_begin \
    const bool stamp_on = (lb == 0 && tid < WAVE); \
    unsigned long long stamp_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long stamp_last = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_s_waitcnt(0xC07F); \
    const unsigned long long stamp_t0 = stamp_last; \
    unsigned long long stamp_rounds = 0;

#define PTNN_DIAG_tree_flush \
    if (stamp_on && tid == 0) { \
        for (int q_ = 0; q_ < 9; ++q_) atomicAdd(p.stamps + q_, stamp_acc[q_]); \
        atomicAdd(p.stamps + 9, stamp_rounds); \
        atomicAdd(p.stamps + 10, __builtin_amdgcn_s_memtime() - stamp_t0); \
    }
