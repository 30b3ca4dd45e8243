/*
 * ptnn.h -- C ABI of libptnn.so: the MI355X (gfx950) parallel-tempering Bayesian-FNN sampler.
 *
 * The reference (sydney-machine-learning/parallel-tempering-neural-net) has no FFI: its seam is the Python
 * class ParallelTempering (REG = multicore-pt-regression/pt_timeseries_regression.py:487-875,
 * CLS = multicore-pt-classification/pt_classification.py:497-897).  This header is the boundary a maintainer
 * binds with ctypes to replace what that class does by forking one ptReplica process per chain; every entry
 * point names the reference code it stands in for.  INTEGRATION.md shows the binding.
 *
 * Conventions: plain C, no C++ or torch types; return 0 = OK, negative = error (text via ptnn_last_error());
 * the caller owns every host buffer (C-contiguous float32 / int32, alive for the call only); the library owns
 * device memory and its stream; a handle is not thread-safe (one host thread per handle, one handle per GPU);
 * calls are synchronous unless their comment says "asynchronous".
 */
#ifndef PTNN_H
#define PTNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTNN_ABI_VERSION 4

#define PTNN_TASK_REG 0 /* Gaussian likelihood + eta = log tau^2 (REG) */
#define PTNN_TASK_CLS 1 /* multinomial likelihood on softmax-of-sigmoid outputs (CLS) */

#define PTNN_SCHED_AUTO 0
#define PTNN_SCHED_COOPERATIVE 1
#define PTNN_SCHED_SPECULATIVE 2
#define PTNN_SCHED_PACKED 3      /* speculative, all slots of a round on one CU (n_hidden <= 8) */
#define PTNN_SCHED_TREE 4        /* prefetching: 2^D - 1 work-groups evaluate every outcome of the next D decisions (random-walk classification) */

typedef struct ptnn_handle ptnn_handle;

/* Everything ParallelTempering.__init__ / initialize_chains / ptReplica.__init__ fix for a run
 * (REG:489-527, 639-650, 140-176; CLS:499-535, 648-659, 159-193). */
typedef struct ptnn_config {
    int32_t struct_bytes;         /* = sizeof(ptnn_config): ABI guard */
    int32_t device_id;            /* HIP device ordinal */
    int32_t task;                 /* PTNN_TASK_REG | PTNN_TASK_CLS */
    int32_t n_in, n_hidden, n_out;/* topology [I, H, O] (REG:30) */
    int32_t n_replicas_local;     /* replicas (temperatures) this handle owns */
    int32_t n_replicas_global;    /* replicas in the whole ladder (== local on one GPU) */
    int32_t first_global_replica; /* global index of local replica 0 (contiguous block of the ladder) */
    int32_t n_samples;            /* S = NumSamples per replica = int(NumSample/num_chains) (REG:506) */
    int32_t swap_interval;        /* REG:496; hand-off trigger differs per task (REG:427 vs CLS:438) */
    int32_t pt_switch_step;       /* step i at which adapttemp drops to 1 (REG:320), or -1 if 0.6*S is not integral */
    int32_t use_langevin;         /* use_langevin_gradients (REG:329) */
    int32_t waves_per_replica;    /* 0 = auto; 1,2,4,8: wavefronts per work-group */
    int32_t schedule;             /* 0 = auto, 1 = cooperative (all waves share one MH step), 2 = speculative
                                   * (wave v pre-computes step i+v; identical chain), 3 = packed
                                   * speculative (n_hidden <= 8: 16 slots on one CU, SGD epochs in lane groups), 4 = prefetching
                                   * tree (random-walk classification runs: groups_per_replica = 2^D - 1 work-groups evaluate the
                                   * proposals of all outcomes of the next D accept/reject decisions, D steps per round; identical
                                   * chain; chosen automatically when replicas x 3 work-groups fit the GPU) */
    int32_t groups_per_replica;   /* speculative schedule: work-groups (CUs) cooperating on one replica; 0 = auto
                                   * (as many of 1, 2, 4 as keeps replicas x groups <= number of CUs).  Tree schedule: 3, 7, 15
                                   * or 31 (0 = auto: the deepest tree that is resident).  Wide nets (n_hidden > 64):
                                   * 1, 2 or 4 work-groups speculating over windows of steps (0 = auto: 4 or 2 where resident).
                                   * Packed schedule: 1, 2 or 4 CUs, each running a packed round over its slots of one window
                                   * (0 = auto: 4 or 2 where resident for 9 <= n_hidden <= 16, whose lane groups leave 8 slots per
                                   * CU; 1 for n_hidden <= 8, which has its 16 slots on one CU) */
    int32_t trace_capacity;       /* rows per replica kept on the device (ring); 0 = all n_samples rows.  With a smaller
                                   * value the caller drains with ptnn_get_traces at least every trace_capacity steps */
    int32_t forward_bf16;         /* forward pass on the matrix cores (cooperative schedule with 24 <= n_hidden <= 64; wide nets with
                                   * n_hidden % 32 == 0).  0 (default) = fp32 accuracy: where the split images fit, every fp32 operand
                                   * is split into three bf16 terms and the six leading partial products run on
                                   * v_mfma_f32_32x32x16_bf16 (errors of the size of fp32 rounding; not bit-identical to the VALU
                                   * schedules), else the exact v_mfma_f32_32x32x2_f32.  1 = operands ROUNDED to bf16 (wide nets only;
                                   * the precision study of BASELINE config 5, changes 0.3 % of the decisions).  2 = always the exact
                                   * fp32 instruction (k-ordered fma chains, bit-identical to the VALU schedules) */
    int32_t swap_rule;            /* 0 = the reference's cascade (REG:659-690, default); 1 = even/odd Metropolis exchange
                                   * min(1, exp((1/T_k - 1/T_k+1)(L_k+1 - L_k))) on untempered log-likelihoods, the moved state
                                   * brings its likelihood and prior along, no phantom round (not in the reference) */
    int32_t shared_noise;         /* 0 = every (replica, step) has its own Philox counter (default); 1 = all replicas read the
                                   * step tape of replica 0 (proposal noise, Langevin coin, MH uniform, eta noise): what the
                                   * reference's forked chains do, which all inherit one numpy / random state (REG:709-712,
                                   * SURVEY Q14).  Initial weights and swap uniforms are not shared (the parent draws them). */
    int32_t label_swap;           /* 0 = a swap round moves (w, eta) between the temperature slots, as the reference does (default);
                                   * 1 = label swapping (not in the reference): the chains stay in place and the
                                   * TEMPERATURES move -- a round only rewrites the slot <-> temperature maps, so nothing but the R
                                   * posted scalars crosses a GPU boundary (zero payload).  A chain keeps its own likelihood (re-tempered
                                   * for its new temperature) and prior: no stale values (Q12 does not apply).  Works with both swap
                                   * rules; needs ptnn_set_ladder.  Trace rows are recorded per chain slot: ptnn_get_labels / the swap log
                                   * say which temperature a slot held when (the Python host stitches the per-temperature files). */
    int32_t shared_device;        /* 1 = other handles or processes run on this GPU at the same time (several blocks of one ladder
                                   * rehearsing the N > 1 path on one device): automatic choices then avoid every schedule whose
                                   * work-groups wait for each other -- several work-groups per replica, the persistent launch --
                                   * because their residency cannot be guaranteed (a non-resident partner is a bounded spin and
                                   * error -5).  Explicit schedule / groups_per_replica requests are still honoured.  0 = the GPU is
                                   * this handle's alone (default). */
    int32_t reserved_;            /* keeps the floats 8-byte aligned with the seed; set 0 */
    float l_prob;                 /* langevin_prob (REG:174); CLS fixes 0.5 (CLS:192) */
    float learn_rate;             /* SGD step of langevin_gradient (REG:33) */
    float step_w;                 /* 0.025 (REG:258) */
    float step_eta;               /* 0.2   (REG:260) */
    float sigma_squared;          /* 25    (REG:273) */
    float nu_1, nu_2;             /* 0, 0  (REG:274-275) */
    uint64_t seed;                /* Philox4x32-10 key; streams are documented in DESIGN.md */
} ptnn_config;

int ptnn_abi_version(void);
/* thread-local, valid until the next failing call on this thread */
const char *ptnn_last_error(void);
/* 1 if a kernel is compiled for (task, n_in, n_out); n_hidden may be anything in [1, 512] (<= 64: one wave per SGD
 * sweep, speculative or cooperative schedule; 65..512: one thread per hidden unit, cooperative schedule) */
int ptnn_supports(int task, int n_in, int n_hidden, int n_out);

/* replaces ParallelTempering.__init__ + the construction of the ptReplica objects (REG:489, 650) */
int ptnn_create(const ptnn_config *cfg, ptnn_handle **out);
int ptnn_destroy(ptnn_handle *h);

/* traindata / testdata (REG:491-492): row-major [n, ncols] float32, columns [x_0..x_{I-1}, y, ...]; copied to HBM */
int ptnn_set_data(ptnn_handle *h, const float *train, int ntr, const float *test, int nte, int ncols);

/* w0 [R_local, P] (REG:649) and temperatures [R_local] (REG:615-636).  Also runs the chain start-up on the device:
 * eta0 = log var(fx_train(w0) - y) for REG (REG:270), initial prior and tempered likelihood (REG:280-285). */
int ptnn_set_state(ptnn_handle *h, const float *w0, const float *temperatures);

/* all R_global temperatures (needed by swap_rule 1 only) */
int ptnn_set_ladder(ptnn_handle *h, const float *temperatures_global);

/* Ladder adaptation during burn-in (swap_rule 1 only; Vousden, Farr & Mandel 2016 with fixed endpoints).
 * Swap round t < rounds moves the log-gaps s_k = log(T_k+1 - T_k) by kappa(t) (a_k(t) - mean_k a_k(t)), kappa(t) = kappa0 t0 / (t + t0),
 * a_k(t) = min(1, exp((1/T_k - 1/T_k+1)(L_k+1 - L_k))) the acceptance of EVERY adjacent pair under the round's ladder, then
 * rescales the gaps so that T_0 = 1 and T_R-1 = the ladder's last temperature stay where they are.  The new ladder is used
 * from the next interval on; from round `rounds` on it is frozen.  Every rule-1 round records its a_k(t).
 * Call after ptnn_set_ladder (which drops a spec set before it) and before the first step; ptnn_set_state restarts the
 * adaptation from the initial ladder.  Refused: swap_rule != 1, no ladder, a ladder that does not start at exactly 1 or is not
 * strictly increasing, rounds outside [0, swap rounds of the run], a last adapted round that hands off after pt_switch_step,
 * kappa0 or t0 not finite and > 0, a call after steps have run.  Checkpoints carry the spec, the log-gaps and both records. */
typedef struct ptnn_ladder_adapt_spec {
    int32_t struct_bytes;  /* = sizeof(ptnn_ladder_adapt_spec): ABI guard */
    int32_t rounds;        /* A: swap rounds that move the ladder; 0 = fixed ladder, acceptances recorded only */
    double kappa0, t0;     /* kappa(t) = kappa0 * t0 / (t + t0) */
} ptnn_ladder_adapt_spec;
int ptnn_set_ladder_adaptation(ptnn_handle *h, const ptnn_ladder_adapt_spec *spec);
/* ladders [A+1][R_global] (row t = the ladder of round t's test, row A the frozen one; rows of rounds not run yet are NaN),
 * accept [rounds recorded][R_global-1] = a_k(t), room for n_samples / swap_interval + 2 rows; either may be NULL.
 * *rounds_recorded = the rounds run so far.  The arrays are those of this handle (every block of a ladder holds the same). */
int ptnn_get_ladder_history(ptnn_handle *h, float *ladders, float *accept, int32_t *rounds_recorded);
/* the adaptation this handle runs (after ptnn_checkpoint_load: the checkpoint's): 1 and *spec filled, or 0 without one.
 * Size the buffers of ptnn_get_ladder_history from spec->rounds.  A checkpoint whose spec differs from the one set on the handle,
 * or that has none while the handle has one, is refused by ptnn_checkpoint_load. */
int ptnn_get_ladder_adaptation(ptnn_handle *h, ptnn_ladder_adapt_spec *spec);

/* Advances every local replica by up to n_steps MH steps (ptReplica.run loop body, REG:313-437) and performs the
 * swap rounds that fall inside (ParallelTempering.swap_procedure + round loop, REG:659-690, 719-752), including the
 * phantom last round when the chain end is reached.  n_steps < 0 = run to the end.  A handle that owns only a
 * block of the ladder (n_replicas_local < n_replicas_global) needs a communicator (ptnn_comm_init / ptnn_comm_init_host)
 * and every rank calls ptnn_run with the same n_steps: the swap rounds then exchange through it.  Asynchronous: returns
 * once the work is queued (the "boundary" exchange waits once per swap round for the permutation); ptnn_sync waits.
 * Without a communicator, and when every work-group of the grid is resident (ptnn_describe: "launches"), the whole call is ONE
 * kernel launch: the intervals and the swap rounds between them run inside it (grid barriers); otherwise one launch per swap
 * interval plus one for the round.  The chains are identical either way. */
int ptnn_run(ptnn_handle *h, int n_steps);
int ptnn_sync(ptnn_handle *h);
/* number of MH steps queued so far (0 .. S-1) */
int ptnn_steps_done(ptnn_handle *h);

/* ---- sharded ladder: one handle per GPU, each owning a contiguous, equally sized block of the temperature ladder ----
 * Replaces the reference's star topology (every replica ships [w, eta, L, T] to the parent through a multiprocessing.Queue
 * each round and blocks on an Event, REG:427-437 <-> 694-759).  Replicas are independent for a swap interval, so the only
 * exchange step is the swap round; every rank computes the identical cascade (uniforms are Philox(seed; round, pair)), hence
 * identical chains for every GPU count.  Two exchanges (ptnn_comm_set_mode):
 *   PTNN_XCHG_GATHER    one in-place all-gather per round of the exchange rows {(w, eta), cached langevin_gradient, L} of all
 *                       replicas (R_global x (8 P + 16) bytes), cascade + row copy on the device, NO host wait: pack kernel,
 *                       collective and swap kernel are queued on the handle's stream behind the segment kernel.
 *   PTNN_XCHG_BOUNDARY  all-gather of the R_global posted scalars L (4 R bytes), cascade on the device, permutation to the
 *                       host (one wait), then ONE grouped send/recv of the rows that cross a GPU boundary: per GPU at most one
 *                       (w, eta) row arrives from below (the carried state; its source may be several GPUs down: xGMI is a
 *                       full mesh, it goes there directly), at most one from the GPU above, and at most one leaves each way
 *                        -- 4 (P + 1) bytes each.  swap_rule 0 only.
 *   PTNN_XCHG_AUTO      GATHER while the gathered buffer is <= 4 MiB (every BASELINE net but the 32-512-1 one), else BOUNDARY.
 */
#define PTNN_XCHG_AUTO 0
#define PTNN_XCHG_GATHER 1
#define PTNN_XCHG_BOUNDARY 2

/* RCCL transport (xGMI on one node).  Rank 0 obtains a unique id (ncclGetUniqueId; 128 bytes) and hands it to every rank by
 * whatever rendezvous launched them; every rank then calls ptnn_comm_init(h, id, 128, rank, nranks) with
 * rank == first_global_replica / n_replicas_local (ncclCommInitRank on the handle's device: collective, blocks until all
 * ranks have joined).  librccl.so is loaded on the first call (dlopen; $PTNN_RCCL_LIBRARY overrides the path), so single-GPU
 * users never load it.  Collectives run on the handle's own stream.
 * Nothing here blocks for ever (the reference's parent polls is_alive() each round, REG:721-727): loading the library,
 * ncclGetUniqueId and ncclCommInitRank run on a helper thread that is abandoned after $PTNN_COMM_TIMEOUT_S seconds (default 120),
 * and every wait behind a collective (ptnn_sync, the getters, the boundary exchange's per-round wait) gives up when the stream
 * is busy but the device has completed no swap round for that long; all of them return -7 with the stage that stalled.
 * The library never changes the environment.  The ladder is sharded inside one node, so the bootstrap needs neither a routable
 * interface nor a verbs probe: callers that own their process export NCCL_SOCKET_IFNAME=lo and NCCL_IB_DISABLE=1 before their
 * first thread starts (the Python host does: distributed.single_node_rccl_env). */
int ptnn_comm_unique_id(void *id_out, int nbytes);
int ptnn_comm_init(ptnn_handle *h, const void *unique_id, int nbytes, int rank, int nranks);
/* One bounded RCCL round trip among `devices` (distinct) from the calling process: unique id, ncclCommInitRank on a thread per
 * device, a 4-byte all-gather, destroy; *seconds = how long it took.  Run it in a fresh CHILD process before the long-lived
 * process touches RCCL: a bring-up that fails or stalls half-way can keep the process it happened in from exiting.  0 = RCCL
 * works among these devices; -7 = it does not (ptnn_last_error names the stage). */
int ptnn_comm_probe(const int32_t *devices, int n, double *seconds);
/* what is attached to the handle: transport (0 none, 1 RCCL, 2 host-staged), this rank, the number of ranks -- for RCCL as the
 * communicator itself reports it (ncclCommCount), not as the caller passed it in -- and the handle's device */
int ptnn_comm_info(ptnn_handle *h, int32_t *transport, int32_t *rank, int32_t *nranks, int32_t *device);
/* the last stage a communicator bring-up / exchange entered in this process, as text ("ncclCommInitRank(rank 0 of 1, device 0)
 * (entered 0.4 s ago)"); $PTNN_COMM_TRACE=1 prints every stage to stderr as it is entered.  Returns the length written. */
int ptnn_comm_last_stage(char *buf, int nbytes);

/* Host-staged transport: the library stages through pinned host memory and calls back.  For fabrics other than RCCL and
 * for tests (RCCL refuses two ranks on one device; a one-GPU box rehearses the N > 1 path with this).
 *   all_gather(ctx, buf, bytes_per_rank): buf holds nranks blocks, this rank's block is filled; fill the others. 0 = OK.
 *   send_recv(ctx, n, peer[n], is_send[n], buf[n], bytes): n messages of `bytes` bytes each, in an order both ends of
 *     every pair agree on (ascending global destination slot); complete all of them before returning.  0 = OK. */
typedef int (*ptnn_all_gather_fn)(void *ctx, void *buf, int64_t bytes_per_rank);
typedef int (*ptnn_send_recv_fn)(void *ctx, int n, const int32_t *peer, const int32_t *is_send, void *const *buf, int64_t bytes);
int ptnn_comm_init_host(ptnn_handle *h, int rank, int nranks, ptnn_all_gather_fn all_gather, ptnn_send_recv_fn send_recv, void *ctx);

int ptnn_comm_set_mode(ptnn_handle *h, int mode);
/* what crossed GPU boundaries so far: payload bytes this rank sent and received, swap rounds exchanged, the mode in use */
int ptnn_comm_stats(ptnn_handle *h, int64_t *bytes_sent, int64_t *bytes_received, int64_t *rounds, int32_t *mode);
/* releases the communicator (ncclCommDestroy); ptnn_destroy does it too */
int ptnn_comm_finalize(ptnn_handle *h);

/* Pure host function (no GPU): which rows rank `rank` receives and sends for the permutation src[R_global] of one round
 * (slot k receives the state of slot src[k]) when every rank owns n_local consecutive slots.  Messages are listed in ascending
 * global destination slot.  msg[4 * m + {0,1,2,3}] = {is_send, peer rank, local row (destination row of a receive, source row
 * of a send), global destination slot}.  Returns the number of messages (<= max_msgs) or negative. */
int ptnn_route(const int32_t *src, int n_global, int n_local, int rank, int32_t *msg, int max_msgs);

/* ---- the pieces of one swap round, for callers that drive the exchange themselves ---- */
/* queue MH steps up to and including the next hand-off step (or the chain end); returns in *handoff 1 when a swap
 * round is due after it, 2 when the due round is the phantom end-of-chain round, 0 otherwise.  Asynchronous. */
int ptnn_run_segment(ptnn_handle *h, int *handoff);
/* device address of the posted scalars L[R_global] (REG:430 / CLS:439); the local block is filled by the segment,
 * the caller all-gathers the rest in place */
int ptnn_swap_L_ptr(ptnn_handle *h, int phantom, void **dev_ptr);
/* overwrite L[R_global] from the host (host-staged transports, tests) */
int ptnn_swap_set_L(ptnn_handle *h, int phantom, const float *L_host);
/* run the cascade on L[R_global] (identical on every rank: uniforms are Philox(seed; round, pair)); writes
 * src[R_global] to the host: slot k receives the (w, eta) of slot src[k] */
int ptnn_swap_cascade(ptnn_handle *h, int phantom, int32_t *src_host);
/* device addresses of the (w, eta) row of a local replica in the current (send) and next (receive) state buffers;
 * row length ptnn_state_row_floats() floats */
int ptnn_swap_row_ptr(ptnn_handle *h, int local_replica, void **cur_row, void **next_row);
int ptnn_state_row_floats(ptnn_handle *h);
/* copy the rows whose source is local, flip the buffers, count the round.  Rows with remote sources must have been
 * received into next_row before this call. */
int ptnn_swap_apply(ptnn_handle *h, const int32_t *src_host, int phantom);

/* Gathered exchange (the default of the sharded-ladder driver; replaces the Queue traffic of REG:427-437 <-> 730-752 with ONE
 * collective per swap round): ptnn_swap_pack writes, for every local replica, the exchange row
 *   { (w, eta) row | cached langevin_gradient row | its valid flag | posted L | swap_rule 1: untempered L, prior | pad }
 * into this rank's block of the buffer ptnn_xchg_ptr returns ([n_replicas_global][row_floats], same layout on every rank);
 * the caller all-gathers the buffer in place; ptnn_swap_apply_gathered then runs the cascade on the gathered L values and
 * copies every local slot's source row out of the buffer, wherever that replica ran, flips the buffers and counts the round. */
int ptnn_xchg_ptr(ptnn_handle *h, void **base, int *row_floats);
int ptnn_swap_pack(ptnn_handle *h, int phantom);
int ptnn_swap_apply_gathered(ptnn_handle *h, int phantom);

/* ---- posterior predictive (the reference's drafts: fx_mu = fx.mean(axis=0) and np.percentile bands over the samples'
 * network outputs, multicore-pt-classification/Misc_code/ldpt_classifier_multi.py:788-794; its run_chains() commented the
 * per-sample outputs out, REG:244-245, 410-419, 785-837) ----
 * Network outputs (REG: sigmoid output, REG:51-55; CLS: softmax of it, CLS:108-110) of a set of weight vectors on a set of input
 * rows, reduced on the device.  The selected rows are collapsed into DISTINCT vectors with multiplicities (a rejected MH step
 * repeats the previous vector, REG:417: runs of bitwise-equal consecutive rows of one chain, or of the TR_SRC row index with
 * compact traces), each evaluated once.  Source: the handle's trace -- rows step0, step0 + thin, ... < step0 + nsteps of the local
 * replicas listed (NULL = all, in order), same residency rules as ptnn_get_traces -- or, when w != NULL, n_w host vectors w [n_w, P]
 * with optional multiplicities (NULL = 1 each; consecutive equal vectors merge as trace rows do).  M = the selected rows,
 * repeats included (the sum of the multiplicities), at most 2^31 - 1.
 * Inputs: x_source PTNN_PREDICT_X_HOST with x [n_rows, n_in] float32, or the handle's own train / test rows (n_rows must then be
 * that set's size).  Outputs, any may be NULL: mean [n_rows, n_out] (the weighted mean, accumulated in double); order_stats
 * [n_ranks, n_rows, n_out] = the exact fp32 value of 0-based rank ranks[k] in the expanded multiset of M values (no interpolation;
 * n_ranks <= 16, 0 <= rank < M); vote [n_rows, n_out] (classification only) = the share of the M samples whose argmax class --
 * of the returned probabilities, first index on a tie -- is that class; samples [M, n_rows, n_out] = every selected row's outputs,
 * chain-major (the reference's fx_train_all / fx_test_all layout, REG:785-788); n_samples = M, n_distinct = distinct vectors.
 * Runs on the handle's stream behind everything queued (a failed run surfaces as at ptnn_sync) and returns when done; columns are
 * processed in blocks whose scratch stays under $PTNN_PREDICT_SCRATCH_BYTES (read per call, default 1 GiB) and of at most
 * 65535 x 64 rows, which changes no result.  Touches no chain state, tape, counter or trace row.  Not with a communicator
 * attached (one GPU only). */
#define PTNN_PREDICT_X_HOST 0
#define PTNN_PREDICT_X_TRAIN 1
#define PTNN_PREDICT_X_TEST 2
#define PTNN_PREDICT_MAX_RANKS 16

typedef struct ptnn_predict_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_predict_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* inputs */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* order statistics */
    const int64_t *ranks;         /* [n_ranks] */
    int32_t n_ranks;
    int32_t reserved_;            /* set 0 */
    /* outputs */
    double *mean;
    float *order_stats;
    double *vote;
    float *samples;
    int64_t *n_samples, *n_distinct;
} ptnn_predict_spec;

int ptnn_predict(ptnn_handle *h, const ptnn_predict_spec *spec);

/* ---- convergence diagnostics (nothing in the reference: it reports no R-hat, effective sample size or Monte Carlo error) ----
 * Classic split-R-hat and split-ESS (Gelman et al., BDA3 11.4-11.5; Geyer's initial monotone sequence as in the Stan Reference
 * Manual; not rank-normalised), with the index arithmetic of DESIGN.md section 12.  A quantity is a weight or a scalar trace
 * column; its C selected chains of n >= 4 draws each are split into their first and last h = n / 2 draws (an odd n drops the
 * middle draw): M = 2C split chains.  Draws are fp32, every mean, product and sum is double.
 * Source: the handle's trace -- rows step0, step0 + thin, ... < step0 + nsteps of the local replicas listed (NULL = all, in
 * order), the residency, checkpoint and ring rules and error texts of ptnn_predict; compact traces resolve the vector through its
 * TR_SRC row -- or, when draws != NULL, host draws [n_chains, n_draws, n_quantities].  Quantities of the trace source: the weights
 * params[n_params] (NULL = all P; a list with n_params = 0 = none), then the scalar columns whose bit (1 << PTNN_TR_*) is set in
 * `scalars`, in PTNN_TR_ order (LIKEH, RMSE_TR, RMSE_TE, ACC_TR, ACC_TE; regression: ACC_TR holds eta = log tau^2, see
 * ptnn_get_trace_rows).  Outputs, any may be NULL, quantity-major in that order: mean [Q] and var [Q] (every selected draw pooled,
 * ddof 1); r_hat [Q] (NaN where every draw is equal, +inf where every split chain is constant but they differ); ess [Q] (NaN where
 * every draw is equal); trunc_lag [Q] (max_t of the pair loop); ess_chain [C, Q] (the same estimator on each chain alone, M = 2);
 * rho [n_lags, Q] (the raw combined autocorrelation rho_t for t < n_lags <= h, before the positivity and monotone edits).
 * Runs on the handle's stream behind everything queued and returns when done; quantities are processed in blocks whose scratch
 * stays under $PTNN_CONVERGENCE_SCRATCH_BYTES (read per call, default 1 GiB), which changes no result.  Touches no chain state,
 * tape, counter or trace row.  Not with a communicator attached (one GPU only).  The rank-normalised family (bulk and tail
 * R-hat and ESS, rank histograms) is the call of its own below, ptnn_rank_convergence. */
#define PTNN_TR_LIKEH 0
#define PTNN_TR_RMSE_TR 1
#define PTNN_TR_RMSE_TE 2
#define PTNN_TR_ACC_TR 3
#define PTNN_TR_ACC_TE 4
#define PTNN_TR_ACCEPT 5
#define PTNN_TR_LOGALPHA 6
#define PTNN_TR_SRC 7

typedef struct ptnn_convergence_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_convergence_spec): ABI guard */
    /* source 1: the trace (used when draws == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    const int32_t *params;        /* weight indices, or NULL = all P */
    int32_t n_params;             /* entries of params (ignored when NULL) */
    int32_t scalars;              /* bit mask over PTNN_TR_LIKEH .. PTNN_TR_ACC_TE */
    /* source 2: host draws */
    const float *draws;           /* [n_chains, n_draws, n_quantities] or NULL */
    int32_t n_chains, n_draws, n_quantities;
    int32_t n_lags;               /* rows of rho (0 = none) */
    /* outputs */
    double *mean, *var, *r_hat, *ess;
    int32_t *trunc_lag;
    double *ess_chain;            /* [C, Q] */
    double *rho;                  /* [n_lags, Q] */
} ptnn_convergence_spec;

int ptnn_convergence(ptnn_handle *h, const ptnn_convergence_spec *spec);

/* ---- rank-normalised convergence diagnostics (nothing in the reference) ----
 * The rank-normalised split-R-hat, bulk / tail / quantile ESS and per-chain rank histograms of Vehtari, Gelman, Simpson, Carpenter
 * & Buerkner (2021), beside the classic figures above; DESIGN.md section 23 states every formula.  Sources, quantities, their
 * order, the rules and the error texts are those of ptnn_convergence.  Of each of the C chains of n >= 4 draws the first and last
 * h = n / 2 are kept and the S' = 2 C h kept draws of a quantity are pooled.  r is a draw's 1-based rank among them, ties (compared
 * by value, -0 = +0) sharing the mean of the ranks they cover; z = Phi^-1((r - 3/8) / (S' + 1/4)) in double (Wichura's AS241,
 * PPND16).  r_hat_bulk and ess_bulk are the split-R-hat and split-ESS of ptnn_convergence with the 2C split chains of z in place of
 * the draws; r_hat_tail is that R-hat of the z-scores of f = |x - med|, med = (x_(S'/2-1) + x_(S'/2)) / 2 of the pooled order
 * statistics (0-based).  For a probability p the indicator I = [x <= x_(lo)], lo = floor((S' - 1) p), is a 0 / 1 series whose
 * split-ESS is ess_quantile; ess_tail is the smaller of those at 0.05 and 0.95 (NaN if either is), ess_median the one at 0.5, and
 * probs[n_probs <= PTNN_RANK_MAX_PROBS] in (0, 1) names further ones.  rank_hist counts, per chain and quantity, the kept draws in
 * bin ((2r - 2) n_bins) / (2 S') (integers), 2 <= n_bins <= PTNN_RANK_MAX_BINS: a chain's bins sum to 2h.  ess_bulk_chain and
 * ess_tail_chain are ess_bulk and ess_tail of each chain alone, with ranks, median and quantiles over that chain's own 2h kept
 * draws.  A quantity whose draws are all equal has NaN everywhere; one whose split chains are constant but differ has R-hat = +inf;
 * a constant indicator has a NaN ESS; a quantity with a draw that is not finite has NaN for every figure and z, and zero counts.
 * Outputs, any may be NULL (what is NULL is not computed), quantity-major: r_hat_bulk, r_hat_tail, ess_bulk, ess_tail, ess_median
 * [Q]; ess_quantile [n_probs, Q]; ess_bulk_chain, ess_tail_chain [C, Q]; rank_hist [C, n_bins, Q]; z [C, 2h, Q], the bulk z-scores
 * in the order of the kept draws.  Runs on the handle's stream behind everything queued and returns when done; quantities are
 * processed in blocks whose scratch stays under $PTNN_CONVERGENCE_SCRATCH_BYTES (read per call, default 1 GiB), which changes no
 * result.  At most 65535 chains and 2^29 pooled kept draws per quantity (more is refused).  Touches no chain state, tape, counter
 * or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_RANK_MAX_PROBS 16
#define PTNN_RANK_MAX_BINS 64

typedef struct ptnn_rank_convergence_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_rank_convergence_spec): ABI guard */
    /* source 1: the trace (used when draws == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    const int32_t *params;        /* weight indices, or NULL = all P */
    int32_t n_params;             /* entries of params (ignored when NULL) */
    int32_t scalars;              /* bit mask over PTNN_TR_LIKEH .. PTNN_TR_ACC_TE */
    /* source 2: host draws */
    const float *draws;           /* [n_chains, n_draws, n_quantities] or NULL */
    int32_t n_chains, n_draws, n_quantities;
    int32_t n_probs;              /* entries of probs */
    const double *probs;          /* further quantile probabilities, each in (0, 1) */
    int32_t n_bins;               /* bins of rank_hist */
    int32_t reserved_;            /* set 0 */
    /* outputs */
    double *r_hat_bulk, *r_hat_tail, *ess_bulk, *ess_tail, *ess_median;
    double *ess_quantile;         /* [n_probs, Q] */
    double *ess_bulk_chain, *ess_tail_chain;   /* [C, Q] */
    int64_t *rank_hist;           /* [C, n_bins, Q] */
    double *z;                    /* [C, 2h, Q] */
} ptnn_rank_convergence_spec;

int ptnn_rank_convergence(ptnn_handle *h, const ptnn_rank_convergence_spec *spec);

/* ---- predictive accuracy (nothing in the reference: it compares topologies by RMSE / accuracy only, result.txt) ----
 * Per data row n: the log pointwise predictive density lppd_n, the WAIC penalty p_waic_n (sample variance of the pointwise
 * log-likelihood, ddof 1), and the PSIS-LOO estimate elpd_loo_n with its Pareto shape khat_n (Vehtari, Gelman & Gabry 2017;
 * Pareto smoothing with the Zhang & Stephens 2009 fit and its weakly informative prior), over the expanded multiset of S samples
 * (a sample with multiplicity c counts c times); DESIGN.md section 13 states every formula.  The pointwise log-likelihood is
 * untempered: regression ll = -log(2 pi tau^2) / 2 - (y - f)^2 / (2 tau^2) with tau^2 = exp(eta) (REG:200-204), classification
 * ll = log p_y of the softmax outputs (CLS:209-222); f / p are the fp32 outputs of ptnn_predict's forward pass, everything after
 * it is double.
 * Sources: (1) the handle's trace, selected as ptnn_predict selects it (same rules and error texts); a regression takes eta from
 * the TR_ACC_TR slot of the row that holds the vector (TR_SRC with compact traces), and a row before its chain's first accepted
 * MH step (no eta recorded yet) is refused.  (2) host vectors w [n_w, P] with eta [n_w] (regression; ignored for classification)
 * and optional multiplicities.  (3) a host pointwise log-likelihood loglik [n_w, n_rows] (finite doubles) with optional
 * multiplicities: no forward pass.  Consecutive samples equal in w and eta bits are one distinct sample; the results depend on
 * the multiset only (bitwise: trace, host vectors, expanded or (distinct, multiplicity), any block size).
 * Data (sources 1, 2): x_source _TRAIN / _TEST (the handle's rows and targets) or _HOST with x [n_rows, n_in + 1] (last column
 * the target; classification: an integer label in [0, n_out)).  r_eff > 0: the relative efficiency of the PSIS tail length
 * M = ceil(min(0.2 S, 3 sqrt(S / r_eff))), at most PTNN_ELPD_TAIL_CAP.  Outputs, any may be NULL: lppd, p_waic, elpd_loo, khat
 * [n_rows] (khat = +inf where the tail holds <= 4 samples, no smoothing); tail_len [n_rows] (expanded tail count T);
 * loglik_out [S, n_rows] (the pointwise log-likelihood, expanded, chain-major as ptnn_predict's samples; sources 1, 2);
 * n_samples = S; n_distinct = distinct samples.
 * Runs on the handle's stream behind everything queued and returns when done; rows are processed in blocks whose scratch stays
 * under $PTNN_ELPD_SCRATCH_BYTES (read per call, default 1 GiB) and of at most 65535 x 64 rows, which changes no result.
 * Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_ELPD_TAIL_CAP 4096

typedef struct ptnn_elpd_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_elpd_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and loglik == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    /* source 3: host pointwise log-likelihood */
    const double *loglik;         /* [n_w, n_rows] or NULL */
    const int32_t *multiplicity;  /* sources 2, 3: [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* data (sources 1, 2) */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in + 1] (host rows only) */
    double r_eff;                 /* > 0; 1 = independent draws */
    /* outputs */
    double *lppd, *p_waic, *elpd_loo, *khat;
    int64_t *tail_len;
    double *loglik_out;
    int64_t *n_samples, *n_distinct;
} ptnn_elpd_spec;

int ptnn_elpd(ptnn_handle *h, const ptnn_elpd_spec *spec);

/* ---- leave-future-out cross-validation of ordered rows (nothing in the reference: it compares by RMSE only) ----
 * The question PSIS-LOO cannot answer for a time series: how well are rows i .. i + block - 1 predicted from rows 0 .. i - 1
 * only (Buerkner, Gabry & Vehtari 2020)?  The data are n_rows ordered rows; the S samples (expanded multiset, as ptnn_elpd) are
 * conditioned on rows [0, n_fit), 0 < n_fit <= n_rows -- the caller's statement.  With ll[s, n] the pointwise log-likelihood of
 * ptnn_elpd and C[s, j] = the sum of ll[s, r] over r < j (double, ascending row order), an origin i (0 < i, i + block <= n_rows)
 * has the log ratio lr_s = C[s, i] - C[s, n_fit] (rows added when i > n_fit, removed when i < n_fit) and the target
 * t_s = C[s, i + block] - C[s, i]: the joint log density of the next `block` rows, each given its own observed inputs (block
 * one-step predictions scored jointly, not a recursive block-step forecast).  (lw, khat, T) = the Pareto smoothing of
 * ptnn_elpd applied to lr (same r_eff rule, cut, tail rule and cap) and elpd_lfo_i = logsumexp(lw + t); DESIGN.md section 18.
 * An origin i == n_fit has every lr = 0: the weights are uniform, elpd_lfo_i = log mean exp t, khat = +inf, T = 0.
 * Sources: the three of ptnn_elpd, selected, merged and refused alike -- (1) the trace, (2) host vectors w [n_w, P] with eta
 * [n_w] (regression) and optional multiplicities, (3) a host loglik [n_w, n_rows] (finite doubles; no forward pass).  The
 * results depend on the multiset of samples only (bitwise: trace, host vectors, expanded or (distinct, multiplicity), any
 * scratch budget, the origins of one call or one call each).  Data (sources 1, 2): as ptnn_elpd, rows in time order.
 * origins [n_origins]: any order, repeats allowed.  Outputs, any may be NULL: elpd_lfo, khat [n_origins] (khat = +inf where
 * the tail holds <= 4 samples, no smoothing), tail_len [n_origins], loglik_out [S, n_rows] (sources 1, 2, as ptnn_elpd's),
 * n_samples = S, n_distinct.
 * Runs on the handle's stream behind everything queued and returns when done; the sums of the columns the origins need and the
 * forward outputs of a block of rows stay under $PTNN_LFO_SCRATCH_BYTES (read per call, default 1 GiB; half each, at least one
 * origin and one row), the origins going in several passes if need be, which changes no result.  Touches no chain state, tape,
 * counter or trace row.  Not with a communicator attached (one GPU only). */
typedef struct ptnn_lfo_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_lfo_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and loglik == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    /* source 3: host pointwise log-likelihood */
    const double *loglik;         /* [n_w, n_rows] or NULL */
    const int32_t *multiplicity;  /* sources 2, 3: [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* data (sources 1, 2), in time order */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in + 1] (host rows only) */
    /* the fit and the origins */
    int32_t n_fit;                /* the samples have seen rows [0, n_fit), 0 < n_fit <= n_rows */
    int32_t block;                /* rows scored per origin, >= 1 */
    const int32_t *origins;       /* [n_origins], 0 < i and i + block <= n_rows */
    int32_t n_origins;
    double r_eff;                 /* > 0; 1 = independent draws */
    /* outputs */
    double *elpd_lfo, *khat;
    int64_t *tail_len;
    double *loglik_out;
    int64_t *n_samples, *n_distinct;
} ptnn_lfo_spec;

int ptnn_lfo(ptnn_handle *h, const ptnn_lfo_spec *spec);

/* ---- recursive multi-step forecasts (nothing in the reference: it scores one-step predictions of the test rows only) ----
 * A regression net with n_out == 1 fitted to windows of one series is the one-step map x[t+1] = f_w(x[t-I+1 .. t]), I = n_in.
 * From an origin window (I inputs) step k = 1 .. horizon of a trajectory is y_k = f_w(window_{k-1}) -- exactly ptnn_predict's
 * forward pass, sigmoid output (REG:51-55) -- plus, with noise on, exp(eta_w / 2) z_k (tau^2 = exp(eta), the REG likelihood's
 * observation variance, REG:200-204); window_k = (window_{k-1}[1:], y_k), the noisy y_k when noise is on.
 * Sample set: selected as ptnn_predict selects it -- the handle's trace (same rules and error texts) or host vectors w [n_w, P]
 * with optional multiplicities; M = the selected rows, repeats included.  Noise off: trajectories depend on w only, one per
 * distinct vector (merged as ptnn_predict merges them), weighted by its multiplicity; seed is ignored.  Noise on: every selected
 * occurrence is its own trajectory, index i = its position in the chain-major selection (c * m + j; host vectors: after
 * expanding the multiplicities), with z_k = box_muller of philox4x32_10(k / 4, i, origin, 4, seed), component k % 4 (0-based k;
 * philox.py: normals(horizon, i, origin, STREAM_FORECAST, seed)[k]); eta comes from the TR_ACC_TR slot of the row that holds the
 * vector (trace; a row before its chain's first accepted MH step has none and is refused) or from eta [n_w] (host vectors).
 * Origins: origin_source PTNN_FORECAST_ORIGIN_HOST with origins [n_origins, n_in] float32, or the handle's train / test inputs
 * (n_origins must be that set's size).  Outputs, any may be NULL, column c = origin * horizon + k: mean [n_origins, horizon]
 * (weighted, accumulated in double); order_stats [n_ranks, n_origins, horizon] (exact fp32 values of 0-based ranks of the
 * expanded multiset of M values, n_ranks <= 16); samples [M, n_origins, horizon] (chain-major, as ptnn_predict's samples);
 * n_samples = M; n_trajectories = trajectories per origin.  With noise off and horizon step 1 every output equals ptnn_predict's
 * on the origin rows, bitwise.
 * Refused: a classification task or n_out != 1, horizon < 1, more than 2^31 - 1 columns, n_ranks > 16, host vectors without eta
 * or trace rows without a recorded eta when noise is on, an attached communicator.
 * Runs on the handle's stream behind everything queued and returns when done; origins and horizon steps are processed in
 * blocks whose scratch stays under $PTNN_FORECAST_SCRATCH_BYTES (read per call, default 1 GiB), the windows carried from one
 * horizon block to the next, which changes no result.  Touches no chain state, tape, counter or trace row. */
#define PTNN_FORECAST_ORIGIN_HOST 0
#define PTNN_FORECAST_ORIGIN_TRAIN 1
#define PTNN_FORECAST_ORIGIN_TEST 2

typedef struct ptnn_forecast_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_forecast_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    const float *eta;             /* [n_w] log tau^2 (noise on) */
    int64_t n_w;
    /* origins */
    int32_t origin_source;        /* PTNN_FORECAST_ORIGIN_HOST | _TRAIN | _TEST */
    int32_t n_origins;
    const float *origins;         /* [n_origins, n_in] (host origins only) */
    int32_t horizon;              /* >= 1 */
    int32_t noise;                /* 0 / 1 */
    uint64_t seed;                /* noise on only */
    /* order statistics */
    const int64_t *ranks;         /* [n_ranks] */
    int32_t n_ranks;
    int32_t reserved_;            /* set 0 */
    /* outputs */
    double *mean;
    float *order_stats;
    float *samples;
    int64_t *n_samples, *n_trajectories;
} ptnn_forecast_spec;

int ptnn_forecast(ptnn_handle *h, const ptnn_forecast_spec *spec);

/* ---- log evidence (nothing in the reference: its ladder follows ptemcee's default_beta_ladder, REG:529-536, whose hottest
 * rung "looks like the prior" for ptemcee's thermodynamic-integration estimate, which the reference never computes) ----
 * Per rung k (draws at beta_k = 1 / T_k): statistics of the full-data log-likelihood U(w) over the rung's draws, and the same
 * over draws of the normalised prior N(0, sigma_squared I_P); the host turns them into thermodynamic-integration (TI) and
 * stepping-stone (SS) estimates of log Z (DESIGN.md section 15 states every formula).  Classification: U = sum_n log p_{y_n}
 * (CLS:209-222, the per-row values ptnn_elpd sums), b = 0.  Regression (eta = log tau^2 integrated out of the improper 1 / tau^2
 * prior): U = -(N / 2) log SSE, b = -log SSE, SSE = sum_n (y_n - f_n)^2 over the N training rows; SSE = 0 is refused.  f / p are
 * the fp32 outputs of ptnn_predict's forward pass on the training rows; every sum after it is double, in row order.
 * Sources: (1) the handle's trace, selected as ptnn_predict selects it (same rules and error texts): each listed replica is one
 * rung, its rows step0, step0 + thin, ... its draws.  (2) host vectors w [n_rungs, n_per_rung, P] with optional multiplicities
 * [n_rungs, n_per_rung].  (3) host U [n_rungs, n_per_rung] (finite doubles) with optional multiplicities: no forward pass.
 * A rung's draws are its rows expanded by their multiplicities, in order; every rung needs at least 4 (the split ESS).
 * Per rung, outputs [n_rungs], any may be NULL: u_mean, u_var (ddof 1), u_ess (the split-ESS of ptnn_convergence on the rung's
 * U draws, in fp32, as one chain); with d [n_rungs] given: log_stone = log mean exp(d_k U) (exact maximum) and stone_relvar =
 * var(exp(d_k U), ddof 1) / mean^2; n_draws [n_rungs] the expanded draw counts; u_out [sum n_draws] every draw's U, rung after rung
 * (sources 1, 2); n_distinct = distinct vectors evaluated (sources 1, 2; runs merged as ptnn_predict merges them).
 * Prior (n_prior > 0; needs n_a in [1, PTNN_EVIDENCE_MAX_A]): draw i is w = sigma z, sigma = sqrt(sigma_squared) in fp32, z_k
 * = box_muller of philox4x32_10(k / 4, i, 0, 5, seed), component k % 4 (philox.py: prior_weights(seed, i, P, sigma)); per
 * exponent a_j, outputs [n_a]: prior_log_mean_exp = log mean exp(b + a_j U) (exact maximum), prior_kish_ess = (sum w)^2 /
 * sum w^2, prior_u_mean / prior_u_var = the mean and (population) variance of U weighted by w = exp(b + a_j U); u_prior_out
 * [n_prior] every prior draw's U.
 * Runs on the handle's stream behind everything queued and returns when done; training rows and prior draws are processed in
 * blocks whose scratch stays under $PTNN_EVIDENCE_SCRATCH_BYTES (read per call, default 1 GiB), which changes no result.
 * Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_EVIDENCE_MAX_A 4

typedef struct ptnn_evidence_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_evidence_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and u == NULL); each replica is a rung */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors; source 3: host U */
    const float *w;               /* [n_rungs, n_per_rung, P] or NULL */
    const double *u;              /* [n_rungs, n_per_rung] or NULL */
    const int32_t *multiplicity;  /* sources 2, 3: [n_rungs, n_per_rung] >= 0, or NULL = 1 each */
    int32_t n_rungs;              /* sources 2, 3 */
    int32_t reserved_;            /* set 0 */
    int64_t n_per_rung;           /* sources 2, 3 */
    const double *d;              /* [n_rungs] stone exponents, or NULL */
    /* prior draws */
    int64_t n_prior;              /* 0 = none */
    uint64_t seed;
    const double *a;              /* [n_a] exponents */
    int32_t n_a;
    int32_t reserved2_;           /* set 0 */
    /* outputs */
    double *u_mean, *u_var, *u_ess, *log_stone, *stone_relvar;               /* [n_rungs] */
    int64_t *n_draws;                                                        /* [n_rungs] */
    double *prior_log_mean_exp, *prior_kish_ess, *prior_u_mean, *prior_u_var; /* [n_a] */
    double *u_out;                                                           /* [sum n_draws] */
    double *u_prior_out;                                                     /* [n_prior] */
    int64_t *n_distinct;
} ptnn_evidence_spec;

int ptnn_evidence(ptnn_handle *h, const ptnn_evidence_spec *spec);

/* ---- every rung at once: the multistate Bennett acceptance ratio (MBAR, Shirts & Chodera 2008; nothing in the reference) ----
 * The free energy of every rung and a weight for every draw of every rung, from one fixed point over all draws (DESIGN.md section
 * 32 states every formula).  States k = 0 .. K-1: an optional prior state first (beta = 0, reduced log density l_0 = 0), then the
 * n_rungs rungs in the order given, `betas` [n_rungs] strictly ascending; K <= PTNN_MBAR_MAX_STATES.  Rung k has l_k(n) = b_n +
 * beta_k U_n, U and b as ptnn_evidence defines them (a classification's b = 0).
 * Sources of the rungs, as ptnn_evidence: (1) the trace, each listed replica one rung; (2) host vectors w [n_rungs, n_per_rung,
 * P]; (3) host U [n_rungs, n_per_rung] with optional b of the same shape (NULL = 0): no forward pass.  Sources 2 and 3 take
 * multiplicities [n_rungs, n_per_rung] >= 0.  The prior state is present when n_prior > 0: host u_prior / b_prior [n_prior]
 * (b_prior NULL = 0), else the n_prior Philox draws of ptnn_evidence (same stream, counter and seed).
 * Items: the n_prior prior draws, then the rungs' rows in source order (trace: chain-major in the order of `replicas`, rows step0,
 * step0 + thin, ...); item n has weight c_n = its multiplicity (1 for trace rows and prior draws), and state k counts N_k = its
 * expanded draws (every rung needs 4).  effective != 0: every item of rung k is scaled by ESS_k / n_k and N_k = ESS_k, the split-ESS
 * of the rung's expanded U draws as ptnn_evidence's u_ess (not finite or not positive: 1); the prior draws are independent.
 * Fixed point: f_k = -log sum_n c_n exp(l_k(n) - D_n), D_n = log sum_j N_j exp(f_j + l_j(n)), f_0 pinned to 0 after every sweep,
 * from f = 0; sweeps are queued in batches of 8 and the largest |f_k - previous f_k| of the last sweep is read once per batch: the
 * call stops when it is <= tol or once max_iter sweeps have run (no error: the caller compares *residual with tol).  Every exp is
 * relative to an exact maximum; every sum is double in a fixed order, so that the sources give identical bits for the same draws.
 * Outputs, any may be NULL: f [K]; gram [K, K] = W^T diag(c) W with W_nk = exp(f_k + l_k(n) - D_n); n_eff [K] = N_k; n_iter (the
 * sweeps run, a multiple of 8); residual; u_out, b_out [n_items] every item's U and b; log_weight [n_items] = log(c_n W_n) at
 * target_beta in [betas[0], betas[n_rungs - 1]], whose free energy is formed like a rung's (-inf where c_n = 0); of w =
 * exp(log_weight): weight_sum, kish_ess = (sum w)^2 / sum (w^2 / c) (the Kish ESS of the draws behind the items: item n stands
 * for c_n draws of weight W_n each) and max_weight_share = max w / sum w; n_items = n_prior + the rungs' rows; n_distinct as
 * ptnn_evidence.
 * The map of the items, [n_items] each: item_chain (the local replica of a trace row, the rung's index in `betas` of a host row, -1
 * for a prior draw), item_step (the trace row's step, the host row's index in its rung, the prior draw's number),
 * item_multiplicity (c_n before the ESS scaling); sse = exp(-b), the sum of squared errors of the item's vector (a regression).
 * Systematic resampling (n_resample = m > 0): cum_weight [n_items] the running sum of w in item order; resample_u = the 23-bit
 * uniform of word 0 of philox4x32_10(0, 0, 0, 7, resample_seed); resample_item [m]: draw i takes the first item whose running sum
 * exceeds ((u + i) / m) * cum_weight[n_items - 1]; resample_w [m, P] the weight vector of every draw, a prior draw's as the device
 * formed it (sources 1, 2 and Philox prior draws only).
 * Expectations (mean or var given; sources 1, 2 and Philox prior draws only): the network outputs of every item's vector on the
 * rows x (ptnn_predict's rows and forward pass), per (row, output) column the mean sum_n w_n f_n / sum_n w_n and the population
 * variance sum_n w_n (f_n - mean)^2 / sum_n w_n under w = exp(log_weight), in double, two passes; the items are added in chunks
 * of 256 (the rungs' rows first, then the prior draws), the chunks in order.
 * Runs on the handle's stream behind everything queued and returns when done; scratch of the forward pass stays under
 * $PTNN_EVIDENCE_SCRATCH_BYTES, which changes no result.  Touches no chain state, tape, counter or trace row.  Not with a
 * communicator attached (one GPU only). */
#define PTNN_MBAR_MAX_STATES 512

typedef struct ptnn_mbar_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_mbar_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and u == NULL); each replica is a rung */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors; source 3: host U (and b) */
    const float *w;               /* [n_rungs, n_per_rung, P] or NULL */
    const double *u;              /* [n_rungs, n_per_rung] or NULL */
    const double *b;              /* source 3: [n_rungs, n_per_rung] or NULL = 0 */
    const int32_t *multiplicity;  /* sources 2, 3: [n_rungs, n_per_rung] >= 0, or NULL = 1 each */
    int32_t n_rungs;              /* all sources: entries of betas */
    int32_t effective;            /* != 0: ESS-scaled weights and counts */
    int64_t n_per_rung;           /* sources 2, 3 */
    const double *betas;          /* [n_rungs] strictly ascending, finite, > 0 */
    /* the prior state */
    int64_t n_prior;              /* 0 = no prior state */
    uint64_t seed;                /* of the Philox prior draws */
    const double *u_prior;        /* [n_prior] host U of the prior draws, or NULL = Philox draws */
    const double *b_prior;        /* [n_prior] with u_prior, or NULL = 0 */
    /* fixed point, target, resampling */
    double target_beta, tol;
    int32_t max_iter;
    int32_t reserved_;            /* set 0 */
    int64_t n_resample;
    uint64_t resample_seed;
    /* rows of the expectations (used when mean or var is asked for) */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST, _TRAIN or _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (PTNN_PREDICT_X_HOST) */
    /* outputs */
    double *f, *gram, *n_eff;                                   /* [K], [K, K], [K] */
    int64_t *n_iter;
    double *residual;
    double *u_out, *b_out, *log_weight, *cum_weight;            /* [n_items] */
    double *weight_sum, *kish_ess, *max_weight_share, *resample_u;
    int64_t *resample_item;                                     /* [n_resample] */
    float *resample_w;                                          /* [n_resample, P] */
    double *mean, *var;                                         /* [n_rows, n_out] */
    int32_t *item_chain, *item_multiplicity;                    /* [n_items] */
    int64_t *item_step;                                         /* [n_items] */
    double *sse;                                                /* [n_items], regression */
    int64_t *n_items, *n_distinct;
} ptnn_mbar_spec;

int ptnn_mbar(ptnn_handle *h, const ptnn_mbar_spec *spec);

/* ---- calibration and proper scores of the predictive distribution (nothing in the reference: it reports RMSE / accuracy) ----
 * Regression (n_out == 1): the predictive distribution of y on data row n is the mixture (1/S) sum_s c_s N(f_s, tau_s^2) over
 * the expanded multiset of S samples (a sample with multiplicity c counts c times), tau_s^2 = exp(eta_s); per row, with the
 * row's target y: pit = (1/S) sum c Phi((y - f) / tau); pred_mean = (1/S) sum c f; pred_sd = sqrt((1/S) sum c (tau^2 + (f -
 * pred_mean)^2)); crps = (1/S) sum_s c_s A(y - f_s, tau_s^2) - (1 / (2 S^2)) sum_s sum_t c_s c_t A(f_s - f_t, tau_s^2 + tau_t^2),
 * A(m, v) = m (2 Phi(m / sqrt v) - 1) + 2 sqrt(v) phi(m / sqrt v) (Grimit et al. 2006; the double sum includes s = t);
 * quantiles [k][n] = a root z of (1/S) sum c Phi((z - f) / tau) = levels_p[k], bisected in double from the bracket [min (f + tau
 * levels_z[k]), max (f + tau levels_z[k])] until the midpoint is an end point; levels_z[k] = Phi^-1(levels_p[k]) is the
 * caller's.  Classification: p_mean [n_rows, n_out] = (1/S) sum c p, bitwise ptnn_predict's mean for the same selection.
 * f / p are the fp32 outputs of ptnn_predict's forward pass, everything after it is double; DESIGN.md section 17.
 * Sources: (1) the handle's trace and (2) host vectors w [n_w, P] with eta [n_w] (regression) and optional multiplicities,
 * selected, merged and refused exactly as ptnn_elpd's sources 1 and 2 (same rules and error texts, the rows without a recorded
 * eta included).  Data as ptnn_elpd: x_source _TRAIN / _TEST or _HOST with x [n_rows, n_in + 1] (last column the target).
 * The results depend on the multiset of samples only (bitwise: trace, host vectors, expanded or (distinct, multiplicity), any
 * block size): every sum is an exact integer sum of fixed-point terms.
 * pair_term != 0 computes crps, U^2 / 2 evaluations of A per row over the U distinct samples: refused when U exceeds
 * PTNN_CALIB_MAX_DISTINCT (select fewer samples, or pair_term = 0, which leaves crps untouched and has no such cap).
 * Outputs, any may be NULL: pit, crps, pred_mean, pred_sd [n_rows]; quantiles [n_levels, n_rows]; p_mean [n_rows, n_out];
 * n_samples = S; n_distinct = U.  Refused: pit / crps / pred_mean / pred_sd / quantiles or pair_term on a classification or
 * with n_out != 1, p_mean on a regression, n_levels outside [0, PTNN_CALIB_MAX_LEVELS], a level outside (0, 1), crps without
 * pair_term, quantiles without levels.
 * Runs on the handle's stream behind everything queued and returns when done; rows are processed in blocks whose scratch stays
 * under $PTNN_CALIB_SCRATCH_BYTES (read per call, default 1 GiB) and of at most 65535 x 64 rows, which changes no result.
 * Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_CALIB_MAX_LEVELS 16
#define PTNN_CALIB_MAX_DISTINCT 65536

typedef struct ptnn_calibration_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_calibration_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* data */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in + 1] (host rows only) */
    /* quantile levels (regression) */
    const double *levels_p;       /* [n_levels] in (0, 1) */
    const double *levels_z;       /* [n_levels] Phi^-1(levels_p) */
    int32_t n_levels;             /* <= PTNN_CALIB_MAX_LEVELS */
    int32_t pair_term;            /* 0 / 1: the CRPS with its pair term (regression) */
    /* outputs */
    double *pit, *crps, *pred_mean, *pred_sd;
    double *quantiles;
    double *p_mean;
    int64_t *n_samples, *n_distinct;
} ptnn_calibration_spec;

int ptnn_calibration(ptnn_handle *h, const ptnn_calibration_spec *spec);

/* ---- forecast verification: proper scores of the recursive forecasts by lead time (nothing in the reference) ----
 * Trajectories: exactly ptnn_forecast's -- the same sample selection, trajectory index i, Philox stream, counters and seed, so
 * `samples` is bitwise ptnn_forecast's with the same arguments.  Noise on: every selected occurrence is its own trajectory, c_i
 * = 1; noise off: one trajectory per distinct (w, eta) sample with multiplicity c (merged as ptnn_calibration merges them: equal
 * w and eta bits).  mu_{i,r,k} = the fp32 sigmoid output of trajectory i at origin r, step k, before that step's noise is added
 * (y = mu + exp(eta / 2) z; noise off: mu = y).  The predictive distribution of the series value at step k is the mixture
 * (1/M) sum_i c_i N(mu_{i,r,k}, tau_i^2), tau_i^2 = exp(eta_i) (Rao-Blackwellised over the last step's noise; at k = 1 it is
 * ptnn_calibration's mixture on the origin row).
 * truth [n_origins, horizon] float32, always from the host: NaN = no observation at that column.  Per column with finite truth
 * y, in double, ptnn_calibration's definitions: pit, pred_mean, pred_sd, crps (with pair_term), quantiles [k][column]; and
 * log_score = log (1/M) sum_i c_i N(y; mu_i, tau_i^2) (pointwise terms as ptnn_elpd's ll, exact maximum, fixed-point sum).
 * Columns without truth give NaN in every per-column output.
 * energy != 0: per origin the energy score of the path (Gneiting et al. 2008) over K_r = the steps with finite truth, Y_i the
 * fp32 noisy path restricted to K_r (noise off: the mean path, weighted by c):
 *   es_r = (1/M) sum_i c_i |Y_i - y|_2 - (1 / (2 M^2)) sum_i sum_j c_i c_j |Y_i - Y_j|_2   (i = j included; double),
 * NaN for an origin with empty K_r; with |K_r| = 1 it is the ensemble CRPS of that column.
 * Every output is bitwise independent of the scratch budget, of repeated calls and of the form of the source (trace, host
 * vectors, expanded or with multiplicities): every sum over trajectories is an exact integer sum of fixed-point terms.
 * Outputs, any may be NULL, column c = origin * horizon + k: pit, crps, log_score, pred_mean, pred_sd [n_origins, horizon];
 * quantiles [n_levels, n_origins, horizon]; energy_score [n_origins]; samples and means (mu) [M, n_origins, horizon] float32,
 * chain-major as ptnn_forecast's samples; n_samples = M; n_trajectories = trajectories per origin.
 * Refused: a classification net or n_out != 1; horizon < 1; more than 2^31 - 1 columns; truth NULL, containing +-inf or without
 * a finite entry; n_levels outside [0, PTNN_CALIB_MAX_LEVELS], a level outside (0, 1), levels without quantiles; crps without
 * pair_term; energy_score without energy; noise on without eta (ptnn_forecast's texts); pair_term or energy with more than
 * PTNN_CALIB_MAX_DISTINCT trajectories; energy with horizon > PTNN_FSCORE_MAX_ENERGY_HORIZON or when one origin's whole
 * horizon does not fit the scratch budget; an attached communicator.
 * Runs on the handle's stream behind everything queued and returns when done; scratch stays under $PTNN_FSCORE_SCRATCH_BYTES
 * (read per call, default 1 GiB): with energy a block is whole origins, else origins and horizon steps are blocked as
 * ptnn_forecast blocks them.  Touches no chain state, tape, counter or trace row. */
#define PTNN_FSCORE_MAX_ENERGY_HORIZON 2048

typedef struct ptnn_forecast_score_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_forecast_score_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    const float *eta;             /* [n_w] log tau^2 */
    int64_t n_w;
    /* origins and truth */
    int32_t origin_source;        /* PTNN_FORECAST_ORIGIN_HOST | _TRAIN | _TEST */
    int32_t n_origins;
    const float *origins;         /* [n_origins, n_in] (host origins only) */
    const float *truth;           /* [n_origins, horizon], NaN = no observation */
    int32_t horizon;              /* >= 1 */
    int32_t noise;                /* 0 / 1 */
    uint64_t seed;                /* noise on only */
    /* quantile levels, the pair term of the CRPS, the energy score */
    const double *levels_p;       /* [n_levels] in (0, 1) */
    const double *levels_z;       /* [n_levels] Phi^-1(levels_p) */
    int32_t n_levels;             /* <= PTNN_CALIB_MAX_LEVELS */
    int32_t pair_term;            /* 0 / 1 */
    int32_t energy;               /* 0 / 1 */
    int32_t reserved_;            /* set 0 */
    /* outputs */
    double *pit, *crps, *log_score, *pred_mean, *pred_sd;
    double *quantiles;
    double *energy_score;
    float *samples, *means;
    int64_t *n_samples, *n_trajectories;
} ptnn_forecast_score_spec;

int ptnn_forecast_score(ptnn_handle *h, const ptnn_forecast_score_spec *spec);

/* ---- input sensitivity (nothing in the reference: it reports no importance, sensitivity or saliency of its inputs) ----
 * Which inputs the sampled nets respond to: the Jacobian of the network output with respect to the inputs, per sample and data
 * row, reduced on the device.  With decode(w) = W1 [I,H], W2 [H,O], B1, B2, bias subtracted, sigmoid on both layers (REG:51-55):
 *   z_h = sum_i x_i W1[i,h] - B1[h]    hid_h = sigmoid(z_h)    d_h  = hid_h (1 - hid_h)
 *   a_o = sum_h hid_h W2[h,o] - B2[o]  s_o   = sigmoid(a_o)    ds_o = s_o (1 - s_o)
 *   J[o,i] = ds_o sum_h W2[h,o] d_h W1[i,h]                    regression: g = J
 *   classification (outputs p = softmax(s), CLS:108-110):      g[c,i] = p_c (J[c,i] - sum_o p_o J[o,i])
 * g is fp32 (d and ds as e / (1 + e)^2 with e = exp(-|z|): no cancellation in a saturated unit); every sum after it is double;
 * DESIGN.md section 19.  Sample set: selected as ptnn_predict selects it -- the handle's trace (same rules and error texts) or
 * host vectors w [n_w, P] with optional multiplicities -- collapsed into distinct vectors as ptnn_predict collapses them; every
 * output is over the expanded multiset of M samples.  Inputs: x_source / n_rows / x [n_rows, n_in] as ptnn_predict.
 * Outputs, any may be NULL.  Per row n, output o, input i (index (n * n_out + o) * n_in + i): grad_mean [n_rows, n_out, n_in]
 * (the weighted mean of g, accumulated in double); order_stats [n_ranks, n_rows, n_out, n_in] = the exact fp32 value of 0-based
 * rank ranks[k] among the M values (ptnn_predict's rule, n_ranks <= 16); pos_count, neg_count [n_rows, n_out, n_in] = the samples
 * with g > 0 and g < 0.  Per output o and input i, with a_s[o,i] = (1/n_rows) sum_n |g_s[n,o,i]| and q_s[o,i] = (1/n_rows)
 * sum_n g_s[n,o,i]^2 of sample s (the row sums in double, in ascending row order): abs_mean, sq_mean [n_out, n_in] = the weighted
 * means of a_s and q_s over the samples; abs_order_stats [n_ranks2, n_out, n_in] = the exact rank ranks2[k] of the fp32-rounded
 * a_s among the M samples; sample_abs [M, n_out, n_in] = every selected row's a_s as fp32, chain-major; samples
 * [M, n_rows, n_out, n_in] = every selected row's g, chain-major (ptnn_predict's samples layout); n_samples = M, n_distinct.
 * Refused: n_rows < 1, an empty selection, a rank outside [0, M), n_rows x n_out x n_in > 2^31 - 1 columns, order statistics
 * requested without ranks.  Runs on the handle's stream behind everything queued and returns when done; rows are processed in
 * blocks whose scratch (4 U n_out n_in bytes per row) stays under $PTNN_SENSITIVITY_SCRATCH_BYTES (read per call, default 1 GiB)
 * and of at most 65535 x 64 rows, which changes no result.  Touches no chain state, tape, counter or trace row.  Not with a
 * communicator attached (one GPU only). */
typedef struct ptnn_sensitivity_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_sensitivity_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* inputs */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* order statistics: of g per (row, output, input), and of a_s per (output, input) */
    const int64_t *ranks;         /* [n_ranks] */
    const int64_t *ranks2;        /* [n_ranks2] */
    int32_t n_ranks, n_ranks2;    /* each <= PTNN_PREDICT_MAX_RANKS */
    /* outputs */
    double *grad_mean;
    float *order_stats;
    int64_t *pos_count, *neg_count;
    double *abs_mean, *sq_mean;
    float *abs_order_stats;
    float *sample_abs;
    float *samples;
    int64_t *n_samples, *n_distinct;
} ptnn_sensitivity_spec;

int ptnn_sensitivity(ptnn_handle *h, const ptnn_sensitivity_spec *spec);

/* ---- partial dependence and ICE curves (nothing in the reference: it never varies an input of a fitted net) ----
 * What the sampled nets do as one input goes over a grid of values, the others held at the data rows (partial dependence, Friedman
 * 2001; individual conditional expectation, Goldstein et al. 2015).  f is the output ptnn_predict returns (a regression's sigmoid
 * output, a classification's p = softmax(s)).  For a selected sample s, data row n, selected input a with index j = inputs[a] and
 * grid value v = grid[a, k]:
 *   ICE_s[n, a, k, o] = f_o(w_s; x_n with x_n[j] := v)          fp32: z_h of the row as it is, then z_h + (v - x_j) W1[j,h]
 *   PD_s[a, k, o]     = (1 / n_rows) sum_n ICE_s[n, a, k, o]    row sums in double, ascending row order, carried across row blocks
 *   range_s[a, o]     = max_k PD32_s[a, k, o] - min_k PD32_s[a, k, o]   PD32 = PD_s rounded to fp32; the difference formed in
 *                                                                       double (exact) and rounded to fp32 once
 * DESIGN.md section 25.  Sample set: selected as ptnn_predict selects it -- the handle's trace (same rules and error texts) or host
 * vectors w [n_w, P] with optional multiplicities -- collapsed into distinct vectors as ptnn_predict collapses them; every output
 * is over the expanded multiset of M samples.  Rows: x_source / n_rows / x [n_rows, n_in] as ptnn_predict.  inputs [n_inputs] = the
 * selected input indices in the caller's order, NULL = all of them, 0 .. n_in - 1 (n_inputs is then ignored); A = their number.
 * grid [A, n_grid] = one row of grid values per selected input, 1 <= n_grid <= PTNN_PD_MAX_GRID; repeated and unsorted values
 * are allowed.  ranks / n_ranks apply to ICE, ranks2 / n_ranks2 to PD_s and range_s (each <= PTNN_PREDICT_MAX_RANKS).
 * Outputs, any may be NULL, and an output costs device work only when its pointer is given (without ice_mean, ice_order_stats and
 * samples the reduction over the n_rows A G n_out ICE columns is not launched).  With G = n_grid, O = n_out and ICE column
 * ((n A + a) G + k) O + o: ice_mean [n_rows, A, G, O] (the weighted mean, accumulated in double); ice_order_stats [n_ranks,
 * n_rows, A, G, O] = the exact fp32 value of 0-based rank ranks[k] among the M values (ptnn_predict's rule); pd_mean [A, G, O] =
 * the weighted mean over the samples of the double row means (a fixed order for a given list of distinct vectors);
 * pd_order_stats [n_ranks2, A, G, O] = the exact rank ranks2[k] of PD32_s; range_mean [A, O] = the weighted mean of range_s;
 * range_order_stats [n_ranks2, A, O]; sample_pd [M, A, G, O] = every selected row's PD32_s, chain-major; sample_range [M, A, O];
 * samples [M, n_rows, A, G, O] = every selected row's ICE, chain-major (ptnn_predict's samples layout); n_samples = M, n_distinct.
 * Refused: what ptnn_sensitivity refuses, n_grid outside [1, PTNN_PD_MAX_GRID], grid NULL, inputs with n_inputs < 1, a grid value
 * that is not finite (with inputs == NULL the grid has n_in rows and is looked at with the handle), order statistics requested
 * without ranks; with the handle: an input index outside [0, n_in) or given twice,
 * n_rows x A x G x n_out > 2^31 - 1 columns, an empty selection, a rank outside [0, M).  Runs on the handle's stream behind
 * everything queued and returns when done; rows are processed in blocks whose scratch (4 U A G n_out bytes per row) stays under
 * $PTNN_PD_SCRATCH_BYTES (read per call, default 1 GiB) and of at most 65535 x 64 rows, which changes no result.  Touches no chain
 * state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_PD_MAX_GRID 64

typedef struct ptnn_pd_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_pd_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* rows */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* the selected inputs and their grids */
    const int32_t *inputs;        /* [n_inputs] distinct indices in [0, n_in), or NULL = 0 .. n_in - 1 */
    int32_t n_inputs;             /* entries of inputs (ignored when NULL) */
    int32_t n_grid;               /* G, 1 .. PTNN_PD_MAX_GRID */
    const float *grid;            /* [A, n_grid] finite */
    /* order statistics: of ICE per (row, input, grid value, output), and of PD32_s and range_s */
    const int64_t *ranks;         /* [n_ranks] */
    const int64_t *ranks2;        /* [n_ranks2] */
    int32_t n_ranks, n_ranks2;    /* each <= PTNN_PREDICT_MAX_RANKS */
    /* outputs */
    double *ice_mean;
    float *ice_order_stats;
    double *pd_mean;
    float *pd_order_stats;
    double *range_mean;
    float *range_order_stats;
    float *sample_pd;
    float *sample_range;
    float *samples;
    int64_t *n_samples, *n_distinct;
} ptnn_pd_spec;

int ptnn_partial_dependence(ptnn_handle *h, const ptnn_pd_spec *spec);

/* ---- accumulated local effects, first order and of input pairs (nothing in the reference) ----
 * Partial dependence sets an input to a grid value on every row, which for correlated inputs (the lags of one series) evaluates the
 * net where no data lies.  Accumulated local effects (Apley & Zhu 2020) move an input only across the bin the row already lies
 * in, average the local differences per bin, accumulate and centre them; the second-order effect of a pair of inputs is what the
 * two do together beyond their main effects.  f is the output ptnn_predict returns; s a selected sample, n a row, o an output.
 * First order, input slot a with index j = inputs[a] and edges z_0 .. z_K (K = n_edges - 1), strictly increasing up to some
 * K* >= 1 and constant from there (the tail is padding: zero-width bins that are always empty):
 *   b(n, a)        = the smallest k >= 1 with x_n[j] <= z_k, K* when there is none (x <= z_0: bin 1; x > z_K*: bin K*)
 *   d_s[n, a, o]   = f_o(w_s; x_n with x_j := z_b) - f_o(w_s; x_n with x_j := z_{b-1})   both f in fp32 (z_h of the row as it is, then
 *                    z_h + (z - x_j) W1[j,h]), the difference formed in double and rounded to fp32 once
 *   m_s[a, k, o]   = (sum of d_s over the n_k rows of bin k) / n_k    double, ascending row order, carried across row blocks; 0
 *                    for an empty bin
 *   g_s[a, k, o]   = g_s[a, k-1, o] + m_s[a, k, o], g_s[a, 0, o] = 0;   c_s[a, o] = (sum_k n_k g_s[a, k, o]) / n_rows
 *   ALE_s[a, k, o] = g_s[a, k, o] - c_s[a, o], k = 0 .. K;  ALE32 = that as fp32;  range_s[a, o] = max_k ALE32 - min_k ALE32 (the
 *                    difference formed in double and rounded once)
 * Second order, pair q = (j, l) with edges u_0 .. u_K2 of j and v_0 .. v_K2 of l (K2 = n_edges2 - 1, the same padding rule), the
 * row in cell (k, m) = (b_j(n), b_l(n)), N(k, m) rows per cell, n^j_k = sum_m N(k, m), n^l_m = sum_k N(k, m):
 *   D2_s[n, q, o]  = [f(u_k, v_m) - f(u_{k-1}, v_m)] - [f(u_k, v_{m-1}) - f(u_{k-1}, v_{m-1})]   x_j and x_l substituted; in double
 *                    from the four fp32 values in this order, fp32 once (each f: the input with the larger index substituted
 *                    first, so that the pair (l, j) evaluates the very corners of (j, l))
 *   D_s[k, m]      = (sum of D2_s over the rows of the cell) / N(k, m), 0 for an empty cell (ALEPlot borrows from the nearest
 *                    non-empty cell instead; cell_count tells how much of the surface rests on data)
 *   h_s[k, m]      = h_s[k-1, m] + sum_{m' <= m} D_s[k, m'] (the running sum along m, ascending), h[0, .] = h[., 0] = 0
 *   A_s[k]         = A_s[k-1] + (sum_m N(k, m) (h[k, m] - h[k-1, m])) / n^j_k;   B_s[m] = B_s[m-1] + (sum_k N(k, m) (h[k, m] -
 *                    h[k, m-1])) / n^l_m;   A[0] = B[0] = 0, a term with a zero count is 0
 *   g2_s[k, m]     = (h[k, m] - A[k]) - B[m];   ALE2_s[q, k, m, o] = g2[k, m] - (sum_{k, m >= 1} N(k, m) g2[k, m]) / n_rows, k-major,
 *                    k, m = 0 .. K2;  ALE2_32 = that as fp32
 *   inter_s[q, o]  = sqrt((sum_{k, m >= 1} N(k, m) ALE2_32^2) / n_rows)   as fp32: the count-weighted RMS at the cells' upper corners
 * Every sum is taken in double in ascending order, products and sums rounded separately.  DESIGN.md section 33.
 * Sample set and rows: exactly as ptnn_partial_dependence.  edges [A, n_edges], 2 <= n_edges <= PTNN_ALE_MAX_EDGES: one row per
 * first-order input; inputs [n_inputs] = their indices in the caller's order, NULL = all n_in (n_inputs is then ignored); edges ==
 * NULL: no first-order term (A = 0), allowed with pairs only.  pairs [n_pairs, 2] = (j, l), n_pairs <= PTNN_ALE_MAX_PAIRS, with
 * edges2 [n_pairs, 2, n_edges2], 2 <= n_edges2 <= PTNN_ALE_MAX_EDGES2; n_pairs = 0 is allowed.  ranks / n_ranks apply to the local
 * effects, ranks2 / n_ranks2 to ALE32, range_s, ALE2_32 and inter_s.
 * Outputs, any may be NULL, and an output costs device work only when its pointer is given.  With E = n_edges, E2 = n_edges2, O =
 * n_out, T = A + n_pairs: bin_count [A, E - 1] and cell_count [n_pairs, E2 - 1, E2 - 1] = the rows per bin and cell; over the
 * expanded multiset of M samples the weighted mean (accumulated in double), the exact fp32 order statistics of ranks2 and every
 * selected row's value, chain-major, of ALE32: ale_mean [A, E, O], ale_order_stats [n_ranks2, A, E, O], sample_ale [M, A, E, O]; of
 * range_s: range_mean [A, O], range_order_stats, sample_range; of ALE2_32: ale2_mean [n_pairs, E2, E2, O], ale2_order_stats,
 * sample_ale2; of inter_s: inter_mean [n_pairs, O], inter_order_stats, sample_inter; of the local effects d_s then D2_s, column (n T
 * + t) O + o: local_mean [n_rows, T, O], local_order_stats [n_ranks, n_rows, T, O], samples [M, n_rows, T, O]; n_samples = M,
 * n_distinct.
 * Refused: what ptnn_partial_dependence refuses, n_edges or n_edges2 out of range, no term at all, a non-finite edge, edges not
 * increasing and then constant or with z_1 <= z_0, a pair with j = l or given twice (in either order); with the handle: an index
 * outside [0, n_in), n_rows x T x n_out > 2^31 - 1 columns, bin accumulators past the scratch budget.  Rows are processed in
 * blocks whose scratch (4 U T n_out bytes per row) stays under $PTNN_ALE_SCRATCH_BYTES (read per call, default 1 GiB), which
 * changes no result.  Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_ALE_MAX_EDGES 64
#define PTNN_ALE_MAX_EDGES2 16
#define PTNN_ALE_MAX_PAIRS 16

typedef struct ptnn_ale_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_ale_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* rows */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* first order: the selected inputs and their edges */
    const int32_t *inputs;        /* [n_inputs] distinct indices in [0, n_in), or NULL = 0 .. n_in - 1 */
    int32_t n_inputs;             /* entries of inputs (ignored when NULL) */
    int32_t n_edges;              /* E, 2 .. PTNN_ALE_MAX_EDGES */
    const float *edges;           /* [A, n_edges] finite, increasing then constant; NULL = no first-order term */
    /* second order: the pairs and their edges */
    const int32_t *pairs;         /* [n_pairs, 2] (j, l), j != l */
    int32_t n_pairs;              /* Q, 0 .. PTNN_ALE_MAX_PAIRS */
    int32_t n_edges2;             /* E2, 2 .. PTNN_ALE_MAX_EDGES2 */
    const float *edges2;          /* [n_pairs, 2, n_edges2]: the edges of j, then of l */
    /* order statistics: of the local effects per (row, term, output), and of the curves, surfaces, ranges and interactions */
    const int64_t *ranks;         /* [n_ranks] */
    const int64_t *ranks2;        /* [n_ranks2] */
    int32_t n_ranks, n_ranks2;    /* each <= PTNN_PREDICT_MAX_RANKS */
    /* outputs */
    int64_t *bin_count;
    int64_t *cell_count;
    double *ale_mean;
    float *ale_order_stats;
    double *range_mean;
    float *range_order_stats;
    float *sample_ale;
    float *sample_range;
    double *ale2_mean;
    float *ale2_order_stats;
    double *inter_mean;
    float *inter_order_stats;
    float *sample_ale2;
    float *sample_inter;
    double *local_mean;
    float *local_order_stats;
    float *samples;
    int64_t *n_samples, *n_distinct;
} ptnn_ale_spec;

int ptnn_accumulated_effects(ptnn_handle *h, const ptnn_ale_spec *spec);

/* ---- coalition values: Shapley attributions of the sampled nets (nothing in the reference: it never splits a prediction among
 * its inputs) ----
 * How much of one prediction each input accounts for, against a background sample (Shapley 1953; Strumbelj & Kononenko 2014;
 * Lundberg & Lee 2017: the interventional value function), per sample, so that the attribution gets a posterior band.  f is the
 * output ptnn_predict returns.  For a selected sample s, explained row x_n, background rows b_1 .. b_B and a coalition S given as
 * a 64-bit mask (bit i set: input i is taken from the explained row):
 *   h(x, b, S)_i   = x_i if i in S else b_i                     the hybrid row: exact fp32 values, a select
 *   v_s[n, S, o]   = (1 / B) sum_b f_o(w_s; h(x_n, b, S))       f in fp32; the sum over b in double, in one fixed order
 *   out_s[n, o, t] = sum_c coef[c, t] v_s[n, S_c, o]            c = 0 .. C - 1 in table order, in double, stored as fp32 once
 * The library does not know what a Shapley value is: it gets the coalition table masks [n_coalitions] and coef [n_coalitions,
 * n_terms] and evaluates n_terms linear functionals of the game (the Python front builds the exact and the permutation tables).
 * DESIGN.md section 29.  Sample set and rows: exactly as ptnn_partial_dependence (the two sample sources, x_source / n_rows / x).
 * background [n_background, n_in] host floats.  ranks / n_ranks apply to out, ranks2 / n_ranks2 to a_s.
 * Outputs, any may be NULL, and an output costs device work only when its pointer is given.  With O = n_out, T = n_terms and
 * column (n O + o) T + t: mean [n_rows, O, T] (the weighted mean of out, accumulated in double); order_stats [n_ranks, n_rows, O,
 * T] = the exact fp32 value of 0-based rank ranks[k] among the M values (ptnn_predict's rule); pos_count, neg_count [n_rows, O, T]
 * = the samples with out > 0 and out < 0.  Per (o, t), with a_s[o, t] = (1 / n_rows) sum_n |out_s[n, o, t]| (the row sums in
 * double, ascending row order, carried across row blocks): abs_mean [O, T] = the weighted mean of a_s over the samples;
 * abs_order_stats [n_ranks2, O, T] = the exact rank ranks2[k] of the fp32-rounded a_s; sample_abs [M, O, T] = every selected
 * row's a_s as fp32, chain-major; samples [M, n_rows, O, T] = every selected row's out, chain-major; n_samples = M, n_distinct.
 * Refused: what ptnn_sensitivity refuses; background NULL or a value that is not finite; n_background outside [1,
 * PTNN_SHAP_MAX_BACKGROUND], n_coalitions outside [1, PTNN_SHAP_MAX_COALITIONS], n_terms outside [1, PTNN_SHAP_MAX_TERMS]; masks
 * or coef NULL; a coefficient that is not finite; with the handle: n_terms x n_out > PTNN_SHAP_MAX_ACC, a mask with a bit at or
 * above n_in, n_rows x n_out x n_terms > 2^31 - 1 columns, an empty selection, a rank outside [0, M).  Runs on the handle's
 * stream behind everything queued and returns when done; rows are processed in blocks whose scratch (4 U n_out n_terms bytes per
 * row) stays under $PTNN_SHAP_SCRATCH_BYTES (read per call, default 1 GiB), which changes no result.  Touches no chain state,
 * tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_SHAP_MAX_COALITIONS 4096
#define PTNN_SHAP_MAX_BACKGROUND 256
#define PTNN_SHAP_MAX_TERMS 64
#define PTNN_SHAP_MAX_ACC 256

typedef struct ptnn_shapley_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_shapley_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* the explained rows */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* the background rows and the coalition table */
    const float *background;      /* [n_background, n_in] finite */
    const uint64_t *masks;        /* [n_coalitions] bit i set: input i from the explained row; no bit at or above n_in */
    const double *coef;           /* [n_coalitions, n_terms] finite */
    int32_t n_background;         /* B, 1 .. PTNN_SHAP_MAX_BACKGROUND */
    int32_t n_coalitions;         /* C, 1 .. PTNN_SHAP_MAX_COALITIONS */
    int32_t n_terms;              /* T, 1 .. PTNN_SHAP_MAX_TERMS, T x n_out <= PTNN_SHAP_MAX_ACC */
    int32_t reserved_;            /* set 0 */
    /* order statistics: of out per (row, output, term), and of a_s per (output, term) */
    const int64_t *ranks;         /* [n_ranks] */
    const int64_t *ranks2;        /* [n_ranks2] */
    int32_t n_ranks, n_ranks2;    /* each <= PTNN_PREDICT_MAX_RANKS */
    /* outputs */
    double *mean;
    float *order_stats;
    int64_t *pos_count, *neg_count;
    double *abs_mean;
    float *abs_order_stats;
    float *sample_abs;
    float *samples;
    int64_t *n_samples, *n_distinct;
} ptnn_shapley_spec;

int ptnn_coalition_values(ptnn_handle *h, const ptnn_shapley_spec *spec);

/* ---- posterior predictive checks (nothing in the reference: it never simulates data from the fitted model) ----
 * Does data simulated from the fitted model look like the data?  (BDA3 ch. 6; Gelman, Meng & Stern 1996.)  Every selected
 * occurrence of a sample draws one replicated data set y_rep on the data rows; a test quantity T is evaluated on y_rep and on
 * the targets y, and p = P(T(y_rep, theta) >= T(y, theta)) is counted over the occurrences.  DESIGN.md section 20.
 * Samples: selected, merged and refused exactly as ptnn_calibration's two sources (the trace, or host vectors w [n_w, P] with
 * eta [n_w] for a regression and optional multiplicities; same rules and error texts, the rows without a recorded eta included).
 * Data as ptnn_elpd: x_source _TRAIN / _TEST or _HOST with x [n_rows, n_in + 1] (last column the target); the rows are taken
 * in the order given (for the time-series nets: time).  Every selected occurrence is its own replicate: occurrence i is
 * position i of the chain-major selection, host vectors after expanding the multiplicities (ptnn_forecast's noise-on index);
 * M = occurrences, U = distinct (w, eta).  The forward pass runs once per distinct vector (ptnn_predict's, fp32 f / p);
 * everything after it is double.
 * Draws: Philox stream 6 (philox.py: STREAM_PPC); the draw of occurrence i, row n is component n % 4 of
 * philox4x32_10(n / 4, i, 0, 6, seed).
 * Regression (n_out == 1): z[i,n] = the device's Box-Muller of that block (philox.normals(n_rows, i, 0, 6, seed)[n] up to
 * fp32 rounding); y_rep[i,n] = f + tau z, tau = exp(eta / 2); standardised residuals e[i,n] = (y_n - f[i,n]) / tau_i of the data
 * and z[i,n] of the replicate.  For a series v of N rows with mean m: sd = the population standard deviation;
 * acf_k(v) = sum_{n >= k} (v_n - m)(v_{n-k} - m) / sum_n (v_n - m)^2.  Statistics, in this order:
 *   0-3  mean, sd, min, max                 of y                      | of y_rep[i, .]        (T on the data is the same for every i)
 *   4    chi2                               sum e^2                   | sum z^2
 *   5    max_abs_resid                      max |e|                   | max |z|
 *   6    ljung_box                          N (N + 2) sum_k acf_k(e)^2 / (N - k) over lags[] | the same on z
 *   7+j  resid_acf[lags[j]]                 acf_k(e[i, .])            | acf_k(z[i, .])
 * lags: at most PTNN_PPC_MAX_LAGS distinct lags, each in [1, n_rows - 1].  n_stats = 7 + n_lags.
 * Classification: p = ptnn_predict's fp32 class probabilities widened to double, u = ((x >> 9) + 0.5) 2^-23 of the Philox
 * component; y_rep[i,n] = the smallest class k with sum_{j<=k} p_j > u sum_j p_j (sums in class order; the last class when none
 * does).  Statistics, each with label = y and with label = y_rep[i, .]: 0 deviance = -2 sum_n log p_label; 1 accuracy = the
 * share of rows with label == argmax p (first index on a tie); 2+k class_count[k].  n_stats = 2 + n_out.
 * Reduction over the occurrences, per statistic j: n_defined = the occurrences where both T are finite (the others are left
 * out of everything); n_greater = #{T_rep > T_obs}; n_equal = #{T_rep == T_obs}; mean_obs, mean_rep, var_rep (population),
 * double sums in an order fixed by M.  The caller forms p_value = (n_greater + n_equal / 2) / n_defined.
 * Outputs, any may be NULL: n_defined, n_greater, n_equal, mean_obs, mean_rep, var_rep [n_stats]; t_obs, t_rep [M, n_stats]
 * chain-major; z [M, n_rows] fp32, the exact normal draws (regression); y_rep [M, n_rows] int32 classes (classification);
 * n_samples = M; n_distinct = U.
 * Refused: n_rows < 2; 2^31 or more samples (ptnn_calibration's limit and text); a lag out of range or listed twice; lags or
 * z on a classification; y_rep on a regression; a regression with n_out != 1; a regression with more rows than one wave's
 * LDS holds as doubles (19456).
 * Runs on the handle's stream behind everything queued and returns when done; the distinct vectors are processed in blocks
 * whose scratch (4 n_rows n_out bytes per vector) stays under $PTNN_PPC_SCRATCH_BYTES (read per call, default 1 GiB): every
 * block holds all rows, so all rows of an occurrence are reduced by one wave in one order and no block size changes a bit.
 * Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_PPC_MAX_LAGS 16

typedef struct ptnn_ppc_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_ppc_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* data */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in + 1] (host rows only) */
    /* residual autocorrelation (regression) */
    const int32_t *lags;          /* [n_lags] distinct, each in [1, n_rows - 1] */
    int32_t n_lags;               /* <= PTNN_PPC_MAX_LAGS */
    int32_t reserved_;            /* keeps the seed 8-byte aligned; set 0 */
    uint64_t seed;                /* Philox key of the replicated data */
    /* outputs */
    int64_t *n_defined, *n_greater, *n_equal;
    double *mean_obs, *mean_rep, *var_rep;
    double *t_obs, *t_rep;
    float *z;
    int32_t *y_rep;
    int64_t *n_samples, *n_distinct;
} ptnn_ppc_spec;

int ptnn_ppc(ptnn_handle *h, const ptnn_ppc_spec *spec);

/* ---- power-scaling sensitivity (nothing in the reference: its prior constants are fixed and never questioned) ----
 * How much do the conclusions depend on the prior, and do prior and data pull against each other?  (Kallioinen, Paananen,
 * Buerkner & Vehtari 2023.)  The prior, or the likelihood, is raised to a power alpha near 1 by importance-reweighting the
 * samples already drawn; the weights are Pareto smoothed; the distance each quantity's marginal moves is measured.  DESIGN.md
 * section 21.
 * Samples: selected, merged and refused exactly as ptnn_calibration's two sources (the trace, or host vectors w [n_w, P] with
 * eta [n_w] for a regression and optional multiplicities; same rules and error texts).  M = occurrences (>= 2), U = distinct
 * (w, eta) (a classification: distinct w); the base weight of distinct vector u is c_u / M, c_u its multiplicity.  A vector
 * of multiplicity 0 takes no part in anything.
 * Components, one double per distinct vector:
 *   likelihood  l_u  = the sum over the TRAINING rows, in row order, of ptnn_elpd's pointwise log-likelihood (untempered, from
 *                      the fp32 forward outputs) -- the training rows whatever rows the predictions are taken on;
 *   prior       pi_u = prior_likelihood (REG:207-221, CLS:224-230) with the handle's sigma_squared, nu_1, nu_2:
 *                      part1 - sum_p w_p^2 / (2 sigma^2) [ - (1 + nu_1) eta - nu_2 exp(-eta) for a regression ],
 *                      part1 = -(cnt / 2) log sigma^2, cnt = I H + H + 2 (REG) or I H + H + O + H O (CLS); double arithmetic on
 *                      the fp32 w and eta (ptnn_evaluate's column 5 to fp32 accuracy).
 * Perturbations: delta > 0; sign 0 is alpha_minus = 1 / (1 + delta), sign 1 is alpha_plus = 1 + delta.  For component c and
 * alpha the log ratio of an occurrence is lr = (alpha - 1) c_u.  (lw, khat, T) = the Pareto smoothing of ptnn_elpd applied to
 * lr (same r_eff rule for the tail bound M_t = ceil(min(0.2 M, 3 sqrt(M / r_eff))) <= PTNN_ELPD_TAIL_CAP, cut, Zhang-Stephens
 * fit and cap at 0; khat = +inf and no smoothing where the tail holds <= 4 samples); tail positions are ordered by lr, then by
 * distinct index, the c_u positions of a vector being consecutive.  The smoothed weight of u is the sum of exp(lw) over its
 * c_u positions; q = those weights normalised to sum 1.
 * Quantities, fp32 values per distinct vector, in this order, of the groups asked for: PTNN_POWERSCALE_WEIGHTS w_0 .. w_{P-1};
 * _ETA eta (regression only); _PREDICTIONS the n_rows * n_out forward outputs of ptnn_predict on the chosen rows (x_source
 * _TRAIN / _TEST, or _HOST with x [n_rows, n_in]), row-major; _LOGLIK (float)l_u.  Q = their count.
 * Distance of one quantity under one perturbation: the U values in ascending order (-0 before +0, then by distinct index);
 * P_j, Q_j = the base and perturbed weights cumulated through position j (double, in that order); b_j = x_{j+1} - x_j;
 * m_j = (P_j + Q_j) / 2; h(a, m) = a (log2 a - log2 m), h(0, .) = 0;
 *   d2 = sum_{j < U-1} b_j [h(P_j, m_j) + h(Q_j, m_j)] / sum_{j < U-1} b_j (P_j + Q_j);
 * the same on the survival side (the order reversed, values negated, weights cumulated from the top); d = sqrt of the larger d2,
 * 0 where that is negative, and 0 where all values are equal.  Sensitivity D = (d(alpha_minus) + d(alpha_plus)) / (2 log2
 * alpha_plus).  Moments per quantity: mean = sum q_u x_u, sd = sqrt(sum q_u (x_u - mean)^2), and the same with the base weights
 * (two passes, double, in the sorted order).
 * Outputs, any may be NULL, k = 2 * component + sign with component 0 = likelihood, 1 = prior: sens [2][Q]; dist, mean, sd
 * [2][2][Q]; base_mean, base_sd [Q]; khat, tail_len [2][2]; logp: room for 2 * n_items doubles (n_items = n_w or the selected
 * trace rows), written as [2][U]: l_u then pi_u; n_samples = M; n_distinct = U; n_quantities = Q.
 * Refused: delta or r_eff not finite and > 0; no group, an unknown group bit, _ETA on a classification; M < 2; the PSIS tail
 * bound above PTNN_ELPD_TAIL_CAP (ptnn_elpd's text); U > PTNN_POWERSCALE_MAX_DISTINCT (thin= lowers U); a component that is
 * not finite for a selected sample; an attached communicator.
 * Runs on the handle's stream behind everything queued and returns when done.  The quantities are ordered and measured in
 * blocks whose scratch (8 * 2^ceil(log2 U) + 4 U bytes per quantity) stays under $PTNN_POWERSCALE_SCRATCH_BYTES (read per call,
 * default 1 GiB; at least one quantity -- predictions: one row's n_out, which alone may exceed a budget smaller than that; the
 * budget bounds these per-quantity buffers and the forward pass over the training rows, not the 32 U bytes of weights, the
 * 2 U components and the outputs [Q]).  A block holds whole quantities with all U values, so
 * no block size changes a bit; the results depend on the sequence of distinct samples and multiplicities only (bitwise: trace,
 * host vectors, expanded or (distinct, multiplicity)).  Touches no chain state, tape, counter or trace row. */
#define PTNN_POWERSCALE_WEIGHTS 1
#define PTNN_POWERSCALE_ETA 2
#define PTNN_POWERSCALE_PREDICTIONS 4
#define PTNN_POWERSCALE_LOGLIK 8
#define PTNN_POWERSCALE_MAX_DISTINCT 65536

typedef struct ptnn_powerscale_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_powerscale_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* the rows of the predictions group (ignored without it) */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    int32_t groups;               /* PTNN_POWERSCALE_* bits */
    int32_t reserved_;            /* set 0 */
    double delta;                 /* > 0 */
    double r_eff;                 /* > 0; 1 = independent draws */
    /* outputs */
    double *sens, *dist, *mean, *sd, *base_mean, *base_sd, *khat;
    int64_t *tail_len;
    double *logp;
    int64_t *n_samples, *n_distinct, *n_quantities;
} ptnn_powerscale_spec;

int ptnn_powerscale(ptnn_handle *h, const ptnn_powerscale_spec *spec);

/* ---- prior predictive checks (nothing in the reference: its prior constants are literals nobody looks at) ----
 * What does the prior imply, before any data is looked at?  (Gabry, Simpson, Vehtari, Betancourt & Gelman 2019.)  Weight
 * vectors are drawn from the prior w ~ N(0, sigma_squared I), the network is evaluated on the rows, and the drawn functions
 * are summarised: per row and output over the draws, and per draw over the rows.  DESIGN.md section 22.
 * Everything is about f, the output ptnn_predict returns (the sigmoid output of a regression, the class probabilities of a
 * classification): tau^2 has an improper prior (nu_1 = nu_2 = 0), so replicated data y is not defined under the prior.
 * Draws: draw i (i = draw0 .. draw0 + n_draws - 1) at scale s is w = float32(sqrt(s)) * z_i, z_i[k] = the device's Box-Muller
 * of component k % 4 of philox4x32_10(k / 4, i, 0, 5, seed): ptnn_evidence's prior vector (philox.prior_weights).  Every
 * scale uses the same z (common random numbers): curves over the scale are smooth.  n_scales = 0: one scale, the handle's
 * sigma_squared; else sigma_squared [n_scales], n_scales <= PTNN_PRIOR_MAX_SCALES, every one finite and > 0.  S = the scales.
 * Rows: x_source _TRAIN / _TEST (with their targets), or _HOST with x [n_rows, n_in + has_target]: has_target != 0 says that
 * column n_in is the target (a classification's: an integer in [0, n_out)).
 * Per scale, row and output over the draws: mean (double); the exact order statistics of ranks[] (0-based ranks among the
 * n_draws values, at most PTNN_PREDICT_MAX_RANKS) -- ptnn_predict's reduction with multiplicity 1, bit for bit; vote (the
 * share of draws whose argmax is this class; classification); sat_count = the draws with f < eps or f > 1 - eps (compared in
 * double), eps in (0, 0.5).
 * Per scale and draw, statistics of the drawn function over the rows, double arithmetic on the fp32 outputs, rows in row order,
 * centred sums in a second pass.  Regression (n_out == 1), n_stats = 7:
 *   0 mean, 1 sd (population), 2 min, 3 max, 4 acf1 = sum_{r >= 1} (f_r - m)(f_{r-1} - m) / sum_r (f_r - m)^2,
 *   5 rmse = sqrt(mean (y - f)^2) (needs the target), 6 saturated = the share of rows with f < eps or f > 1 - eps.
 * Classification, n_stats = 4 + n_out, arg = the first class of the largest probability:
 *   0 accuracy = the share of rows with y == arg, 1 log_score = mean of -log p_y (both need the target), 2 confidence = mean of
 *   max_k p_k, 3 saturated = the share of rows with max_k p_k > 1 - eps, 4 + k class_share[k] = the share of rows with arg == k.
 * A statistic that needs a target is NaN without one.  T(y), the data's counterpart: 0-4 of the target series (regression),
 * the label shares 4 + k (classification); NaN for the others and without a target.
 * Per scale and statistic over the draws: stat_mean, stat_sd (population; two passes, double, a tree fixed by n_draws), the
 * order statistics of ranks[] of the statistic rounded to fp32, and the integer counts n_defined = the draws whose statistic is
 * not NaN (the others are left out of everything), n_greater = #{T(f_i) > T(y)}, n_equal = #{T(f_i) == T(y)} (both 0 where
 * T(y) is NaN).  Shares are counts divided by the same n_rows, so class_share compares as integer counts do.  The caller forms
 * p = (n_greater + n_equal / 2) / n_defined.
 * Outputs, any may be NULL: mean, vote [S, n_rows, n_out]; order_stats [S, n_ranks, n_rows, n_out] fp32; sat_count [S, n_rows,
 * n_out]; t_obs [n_stats]; stat_mean, stat_sd, n_greater, n_equal, n_defined [S, n_stats]; stat_order_stats [S, n_ranks,
 * n_stats] fp32; t_draw [S, n_draws, n_stats]; samples [S, n_draws, n_rows, n_out] fp32; weights [S, n_draws, P] fp32;
 * n_stats; n_blocks = the blocks of draws one scale was generated in.  t_draw and samples are transposed on the host: asking
 * for one costs, per scale, a host copy of its size (samples: the size of the scale's output matrix) and a wait for the stream.
 * Refused: n_draws < 1; draw0 < 0 or draw0 + n_draws > 2^32 (the Philox counter); n_scales outside [0, PTNN_PRIOR_MAX_SCALES]
 * or without sigma_squared; a scale that is not finite and > 0; eps outside (0, 0.5); more than PTNN_PREDICT_MAX_RANKS ranks,
 * a rank outside [0, n_draws); vote on a regression; a regression with n_out != 1; a class label that is no integer in [0,
 * n_out); 2^31 or more draws or columns; an attached communicator; and a selection whose one-scale output matrix 4 n_rows
 * n_out n_draws bytes exceeds $PTNN_PRIOR_SCRATCH_BYTES (read per call, default 1 GiB) -- the text names the largest n_draws
 * that fits: a prior predictive check needs thousands of draws, not millions.
 * Runs on the handle's stream behind everything queued and returns when done.  The scales run one after another; the vectors
 * of a scale are generated and evaluated in blocks of draws that take what the budget leaves beside the output matrix (4 P + 8
 * + 4 n_rows n_out bytes per draw, at least one draw), and every reduction reads the whole matrix: no block size changes a
 * bit, and draws [0, n) are draws [0, m) followed by draws [m, n) of a call with draw0 = m.  Works as soon as ptnn_set_data
 * and ptnn_set_state have been called: it needs no trace.  Touches no chain state, tape, counter or trace row. */
#define PTNN_PRIOR_MAX_SCALES 8

typedef struct ptnn_prior_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_prior_spec): ABI guard */
    int32_t n_scales;             /* 0 = the handle's sigma_squared, else <= PTNN_PRIOR_MAX_SCALES */
    const double *sigma_squared;  /* [n_scales], each finite and > 0 */
    int64_t n_draws;              /* >= 1 */
    int64_t draw0;                /* the first draw's Philox counter: >= 0, draw0 + n_draws <= 2^32 */
    uint64_t seed;                /* Philox key of the draws */
    /* rows */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in + (has_target != 0)] (host rows only) */
    int32_t has_target;           /* host rows: column n_in is the target */
    int32_t n_ranks;              /* <= PTNN_PREDICT_MAX_RANKS */
    const int64_t *ranks;         /* [n_ranks] 0-based ranks among the n_draws values */
    double eps;                   /* saturation margin, in (0, 0.5) */
    /* outputs */
    double *mean;
    float *order_stats;
    double *vote;
    int64_t *sat_count;
    double *t_obs, *stat_mean, *stat_sd;
    float *stat_order_stats;
    int64_t *n_greater, *n_equal, *n_defined;
    double *t_draw;
    float *samples, *weights;
    int64_t *n_stats, *n_blocks;
} ptnn_prior_spec;

int ptnn_prior_predictive(ptnn_handle *h, const ptnn_prior_spec *spec);

/* ---- classification report (nothing in the reference: it reports acc_train / acc_test, one number per sample) ----
 * How well a classifier separates its classes, per sampled net and for the pooled classifier: confusion counts, per-class
 * precision / recall / F1 and one-vs-rest ROC-AUC.  Classification handles only; DESIGN.md section 26.
 * Rows n = 0 .. N-1 with labels y_n in [0, K), K = n_out.  Samples: the expanded multiset of S selected rows, U distinct vectors
 * with integer counts c_u, selected, merged and refused exactly as ptnn_predict's sources 1 and 2.  p_u[n, k] = the fp32
 * probability ptnn_predict's forward pass returns; pred_u[n] = argmax_k p_u[n, k], first index on a tie (the rule of vote).
 * Per distinct sample, exact integers: conf_u[i, j] = #{n: y_n = i, pred_u[n] = j} (int32), n_k = #{y_n = k}, col_u[k] = sum_i
 * conf_u[i, k], and auc2_u[k] = sum_{n: y_n = k} sum_{m: y_m != k} (2 [p_u[n, k] > p_u[m, k]] + [p_u[n, k] == p_u[m, k]]) (int64,
 * compared as fp32 values): twice the Mann-Whitney U statistic with ties counted half.
 * Per distinct sample Q metric columns, each from those integers by one division in double (a mean: the sum of the quotients in
 * class order divided by their count), stored as fp32, in this order: accuracy = tr(conf) / N; balanced_accuracy = the mean of
 * recall over the classes with n_k > 0; macro_f1 = the mean of f1 over those classes; macro_auc = the mean of auc over the
 * classes with 0 < n_k < N; precision[k] = conf[k, k] / col[k] (0 when col[k] = 0); recall[k] = conf[k, k] / n_k; f1[k] =
 * 2 conf[k, k] / (n_k + col[k]); auc[k] = auc2[k] / (2 n_k (N - n_k)).  Q = 4 + 4 K, or 3 + 3 K with auc == 0 (no macro_auc, no
 * auc[k]).  A column the data leave undefined -- recall and f1 of a class with n_k = 0, auc with n_k in {0, N}, a macro column
 * with no class left -- is written as 0 (the caller knows them from the labels).
 * Over the samples, as ptnn_predict reduces a column: metric_mean [Q] (weighted, accumulated in double), metric_order_stats
 * [n_ranks, Q] (exact fp32 order statistics of the expanded multiset; n_ranks <= 16, 0 <= rank < S), confusion_sum [K, K] int64
 * = sum_u c_u conf_u, sample_metrics [S, Q] fp32 and sample_confusion [S, K, K] int32, chain-major.  The pooled classifier:
 * p_mean and vote [N, K] are bitwise ptnn_predict's mean and vote for the same selection; p_correct [N] = vote[n, y_n].
 * Data as ptnn_elpd: x_source _TRAIN / _TEST or _HOST with x [n_rows, n_in + 1] (last column the label).  Outputs, any may be
 * NULL.  Refused: a regression handle; a label that is not an integer in [0, K) (the first such row is named); n_ranks > 16 or a
 * rank outside [0, S); auc != 0 with more than PTNN_REPORT_MAX_AUC_ROWS rows (a sample's scores of one class are ranked in one
 * work-group's LDS; auc == 0 has no cap); more than 65535 x 64 rows.
 * Runs on the handle's stream behind everything queued and returns when done.  The forward image [N K][U] is computed at once
 * where it fits $PTNN_REPORT_SCRATCH_BYTES (read per call, default 1 GiB); else p_mean / vote come from ptnn_predict's blocks of
 * rows and everything per sample from blocks of samples, which changes no result.  Touches no chain state, tape, counter or
 * trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_REPORT_MAX_AUC_ROWS 16384

typedef struct ptnn_class_report_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_class_report_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* data */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in + 1] (host rows only) */
    /* order statistics of the metric columns */
    const int64_t *ranks;         /* [n_ranks] */
    int32_t n_ranks;
    int32_t auc;                  /* 0 / 1: the auc columns */
    /* outputs */
    double *p_mean, *vote;        /* [n_rows, n_out] */
    double *p_correct;            /* [n_rows] */
    double *metric_mean;          /* [Q] */
    float *metric_order_stats;    /* [n_ranks, Q] */
    int64_t *confusion_sum;       /* [n_out, n_out] */
    float *sample_metrics;        /* [S, Q] */
    int32_t *sample_confusion;    /* [S, n_out, n_out] */
    int64_t *n_samples, *n_distinct;
} ptnn_class_report_spec;

int ptnn_class_report(ptnn_handle *h, const ptnn_class_report_spec *spec);

/* ---- predictive uncertainty: aleatoric and epistemic (nothing in the reference) ----
 * How uncertain the sampled nets are on a data row, and whether that is noise in the data or disagreement among the nets;
 * DESIGN.md section 28.  Samples: the expanded multiset of S selected rows, U distinct vectors with integer counts c_u,
 * selected, merged and refused exactly as ptnn_calibration's sources 1 and 2 (same rules and error texts: a regression's host
 * vectors need eta, trace rows without a recorded eta are refused).  p_u[n, k] / f_u[n, o] = the fp32 outputs of ptnn_predict's
 * forward pass; everything after it is double.  Rows: x_source _TRAIN / _TEST or _HOST with x [n_rows, n_in], as ptnn_predict;
 * no target is read.
 * Both tasks: mean [n_rows, n_out] = (1/S) sum c_u output_u, bitwise ptnn_predict's mean for the same selection.
 * Classification (K = n_out), per row n, natural log, 0 log 0 = 0: vote [n_rows, K], bitwise ptnn_predict's;
 * H_u[n] = -sum_k p_u[n, k] log p_u[n, k], each product and each sum rounded once, terms added in class order;
 * entropy_mean[n] = (1/S) sum c_u H_u[n], the expected entropy (the aleatoric part), an exact fixed-point sum of the terms
 * H_u / log K clamped to [0, 1] (fp32 probabilities may sum to a little over 1 and carry H_u an fp32 rounding above log K: such
 * a term counts as log K); entropy_order_stats [n_ranks, n_rows] = exact fp32 order statistics of (float)H_u[n] over the expanded
 * multiset (n_ranks <= 16, 0 <= rank < S); sample_entropy [S, n_rows] fp32 = (float)H_u[n], chain-major.
 * Regression, per row n and output o: epistemic_var [n_rows, n_out] = (1/S) sum c_u (f_u - mean)^2 in two passes, centred on
 * the mean above: an exact fixed-point sum of the terms d^2 / R^2 with R the range of f over the samples (R = 0: exactly 0);
 * aleatoric_var [1] = (1/S) sum c_u exp((double)eta_u), an exact sum of the terms exp(eta_u) / max_u exp(eta_u).
 * entropy_mean, epistemic_var and aleatoric_var depend on the multiset of samples only (bitwise: trace, host vectors, expanded or
 * (distinct, multiplicity), any block size).
 * Outputs, any may be NULL.  Refused: vote or an entropy output on a regression; a variance output on a classification;
 * n_ranks > 16 or a rank outside [0, S); n_rows < 1.
 * Runs on the handle's stream behind everything queued and returns when done; rows are processed in blocks whose scratch stays
 * under $PTNN_UNC_SCRATCH_BYTES (read per call, default 1 GiB) and of at most 65535 x 64 rows, which changes no result.
 * Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
typedef struct ptnn_uncertainty_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_uncertainty_spec): ABI guard */
    /* source 1: the trace (used when w == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each */
    int64_t n_w;
    /* data */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* order statistics of the per-sample entropy (classification) */
    const int64_t *ranks;         /* [n_ranks] */
    int32_t n_ranks;
    int32_t reserved_;
    /* outputs */
    double *mean;                 /* [n_rows, n_out] */
    double *vote;                 /* [n_rows, n_out] (classification) */
    double *entropy_mean;         /* [n_rows] (classification) */
    float *entropy_order_stats;   /* [n_ranks, n_rows] (classification) */
    float *sample_entropy;        /* [S, n_rows] (classification) */
    double *epistemic_var;        /* [n_rows, n_out] (regression) */
    double *aleatoric_var;        /* [1] (regression) */
    int64_t *n_samples, *n_distinct;
} ptnn_uncertainty_spec;

int ptnn_uncertainty(ptnn_handle *h, const ptnn_uncertainty_spec *spec);

/* ---- case influence: which data rows drive a prediction (nothing in the reference) ----
 * For a posterior p(theta) ~ prior x prod_i p(y_i | theta)^{w_i}, d E[g] / d w_i at w = 1 is Cov_post(g, l_i) with l_i = log p(y_i |
 * x_i, theta): cov[a, b] = the covariance over the samples of target column a with the log-likelihood of case row b, minus it the
 * first-order effect of deleting the case; DESIGN.md section 30.  Samples: the expanded multiset of M selected rows, U distinct
 * (w, eta) samples with integer counts c_u, selected, merged and refused exactly as ptnn_elpd's sources 1 and 2 (same rules and
 * error texts: a regression's host vectors need eta, trace rows without a recorded eta are refused); or source 3, host matrices
 * target_values [n_w, n_a] float32 and loglik [n_w, n_b] double with multiplicity and no forward pass, every host row a sample.
 * Cases (sources 1, 2): case_source _TRAIN / _TEST or _HOST with case_x [n_cases, n_in + 1] (last column the target); column b of
 * B = l of case row b, formed as ptnn_elpd forms it; n_b = n_cases.  Targets: target_kind PTNN_INFLUENCE_OUTPUT: target_x
 * [n_targets, n_in], the fp32 outputs of ptnn_predict's forward pass widened to double, n_a = n_targets x n_out, column n x n_out
 * + o; PTNN_INFLUENCE_LOGLIK: target_x [n_targets, n_in + 1], l of the target rows, n_a = n_targets.
 * With m_a = (1/M) sum c_u A[a, u] (the sum taken of A - min A):
 *   cov[a, b] = sum_u c_u (A[a, u] - m_a)(B[b, u] - m_b) / (M - 1), every product and sum in double: fused multiply-adds in
 *   ascending u within chunks of 512 distinct samples, the chunks added in ascending order (no atomics);
 *   target_mean, target_var [n_a], case_mean, case_var [n_b]: m and sum c_u (. - m)^2 / (M - 1) (ddof 1 over the expanded multiset).
 * A result's bits depend on the list of distinct samples and their counts only: not on the row blocks, the grid or the scratch.
 * Outputs, any may be NULL.  Refused: n_a x n_b > 2^27; M < 2; U > 65535 x 512; a host loglik that is not finite; target_values without loglik or
 * the reverse, or either with w; an unknown target_kind; n_cases or n_targets < 1.
 * Runs on the handle's stream behind everything queued and returns when done; the rows of A and B are processed in blocks whose
 * scratch stays under $PTNN_INFLUENCE_SCRATCH_BYTES (read per call, default 1 GiB; the output matrix lies beside it), which
 * changes no result.  Touches no chain state, tape, counter or trace row.  Not with a communicator attached (one GPU only). */
#define PTNN_INFLUENCE_OUTPUT 0
#define PTNN_INFLUENCE_LOGLIK 1
#define PTNN_INFLUENCE_MAX_ELEMENTS (1 << 27)
#define PTNN_INFLUENCE_KCHUNK 512

typedef struct ptnn_influence_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_influence_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and loglik == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const float *eta;             /* [n_w] log tau^2 (regression) */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each (sources 2 and 3) */
    int64_t n_w;
    /* source 3: host matrices */
    const float *target_values;   /* [n_w, n_a] or NULL */
    const double *loglik;         /* [n_w, n_b] or NULL */
    int32_t n_a, n_b;             /* source 3 only */
    /* cases (sources 1 and 2) */
    int32_t case_source;          /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_cases;
    const float *case_x;          /* [n_cases, n_in + 1] (host rows only) */
    /* targets (sources 1 and 2) */
    int32_t target_kind;          /* PTNN_INFLUENCE_OUTPUT | _LOGLIK */
    int32_t target_source;        /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_targets;
    int32_t reserved_;
    const float *target_x;        /* [n_targets, n_in] (OUTPUT) or [n_targets, n_in + 1] (LOGLIK) (host rows only) */
    /* outputs */
    double *cov;                  /* [n_a, n_b] */
    double *target_mean, *target_var;   /* [n_a] */
    double *case_mean, *case_var;       /* [n_b] */
    int64_t *n_samples, *n_distinct;
} ptnn_influence_spec;

int ptnn_influence(ptnn_handle *h, const ptnn_influence_spec *spec);

/* ---- posterior modes: function-space clusters of the sampled nets (nothing in the reference) ----
 * A one-hidden-layer net has H! x (sign) equivalent labelings of its hidden units, so sampled nets are compared by what they
 * compute, not by where their weights lie; DESIGN.md section 31.
 * Samples: ptnn_predict's selection, sources 1 (the trace) and 2 (host vectors w with multiplicity), no eta: a mode is a property of
 *   the function.  It yields U distinct weight vectors with integer counts c_u, M = sum c_u, and per selected item the distinct
 *   sample it belongs to (predict_scan_kernel's item_run).  Source 3: a host matrix values [n_w, n_a] float32 with multiplicity and
 *   no forward pass; every host row is a sample, U = n_w.
 * Outputs of the nets: F[u, j], j < n = n_rows x n_out, the fp32 outputs of ptnn_predict's forward pass on the rows x (source 3:
 *   F = values, n = n_a).
 * Squared distance: sq[u, v] = sum_j (F[u, j] - F[v, j])^2 in double: each difference is taken of the two values widened to
 *   double, each term added by fma(d, d, acc), one accumulator per element, carried in the matrix across the column blocks, columns
 *   ascending.  An element's bits depend on the two samples' output vectors and n only: not on the tile, the row blocks, the grid or
 *   the scratch.  sq[u, u] = 0, sq[u, v] = sq[v, u] bit for bit, no atomics.  The distance a user sees is d = sqrt(sq / n), the RMS
 *   difference of two nets' outputs in output units (both tasks put out values in [0, 1]).
 * Density (density-peaks clustering, Rodriguez & Laio 2014; all comparisons on sq): near_sq = radius^2 x n, formed by the caller in
 *   double.  rho_u = sum_v c_v [sq[u, v] <= near_sq] (includes v = u).  v precedes u iff rho_v > rho_u, or rho_v = rho_u and v < u.
 *   delta_sq_u = min over the v that precede u of sq[u, v]; parent_u = the lowest such v that attains it.  The one sample nothing
 *   precedes has parent -1 and delta_sq = max_v sq[u, v].  Samples with c_u = 0 (multiplicities of sources 2 and 3) are absent: they
 *   count nowhere and come back with rho 0, delta_sq 0 and parent -1.  A non-finite sq (NaN or infinite outputs) among the present
 *   samples is counted and the call refused with a text that names the first such sample.
 * spread_sq = sum_u sum_v c_u c_v sq[u, v] / M^2 in double, in a fixed order (per row a strided partial and an LDS tree, the rows
 *   added in ascending order).
 * Outputs, any may be NULL (without sq_dist the matrix is still formed in device memory): rho, delta_sq, parent, count hold
 *   n_items entries (n_items = the selected trace rows, or n_w), of which the first U = *n_distinct are written; item_sample
 *   [n_items], items chain-major [n_chains, m] for the trace; sq_dist and outputs are written packed, [U, U] and [U, n], and must
 *   hold min(n_items, 11585)^2 and min(n_items, 11585) x n entries.
 * Refused: U x U > PTNN_MODES_MAX_ELEMENTS (the text gives U and names thin= / chains= as the way down); M < 1; near_sq not finite
 *   or < 0; values together with w; room < n_items; a communicator attached (one GPU only).
 * Runs on the handle's stream behind everything queued and returns when done; the columns are processed in blocks as ptnn_predict
 *   cuts them, whose scratch stays under $PTNN_MODES_SCRATCH_BYTES (read per call, default 1 GiB; the matrix lies beside it), which
 *   changes no result.  Touches no chain state, tape, counter or trace row. */
#define PTNN_MODES_MAX_ELEMENTS (1 << 27)

typedef struct ptnn_modes_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_modes_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and values == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each (sources 2 and 3) */
    int64_t n_w;
    /* input rows (sources 1 and 2) */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* source 3: a host matrix */
    const float *values;          /* [n_w, n_a] or NULL */
    int32_t n_a;
    int32_t reserved_;
    double near_sq;               /* radius^2 x n */
    int64_t room;                 /* entries that rho, delta_sq, parent, count and item_sample each hold: >= n_items, else refused */
    /* outputs */
    int64_t *rho;                 /* [n_items], U written */
    double *delta_sq;             /* [n_items], U written */
    int32_t *parent;              /* [n_items], U written */
    int32_t *count;               /* [n_items], U written */
    int32_t *item_sample;         /* [n_items] */
    double *spread_sq;            /* [1] */
    double *sq_dist;              /* [U, U] packed */
    float *outputs;               /* [U, n] packed */
    int64_t *n_samples, *n_distinct;
} ptnn_modes_spec;

int ptnn_modes(ptnn_handle *h, const ptnn_modes_spec *spec);

/* ---- posterior compression: a small ensemble that stands for all the sampled nets (nothing in the reference) ----
 * Kernel herding with the energy-distance kernel ("support points", Mak & Joseph 2018; Chen, Welling & Smola 2010) on the
 * function-space distance of ptnn_modes; DESIGN.md section 34.
 * Samples: exactly those of ptnn_modes -- sources 1 (the trace), 2 (host vectors w with multiplicity) and 3 (a host matrix values
 *   [n_w, n_a]).  A selection yields U distinct samples with integer counts c_u, M = sum c_u, and item_sample maps every selected
 *   item to its distinct sample.  Samples with c_u = 0 are absent: never chosen, counted nowhere.
 * sq[u, v]: ptnn_modes' matrix, formed by the same kernels (modes_outputs_kernel, modes_dist_kernel): the same bits, the same
 *   PTNN_MODES_MAX_ELEMENTS cap with the same refusal text, the same $PTNN_MODES_SCRATCH_BYTES column blocks.  A non-finite sq among
 *   the present samples is refused with a text that names the first such sample.
 * Arithmetic: double throughout, every operation rounded once, none contracted with its neighbour, in the orders given here, so that
 *   a float64 replay in the same order reproduces every bit.
 * Distance: d[u, v] = sqrt(sq[u, v]), correctly rounded, taken on the fly (the matrix is not modified).  d / sqrt(n) is the RMS
 *   output difference of two nets, the unit of posterior_modes.
 * Mean distance: mu_u = (sum_v (double)c_v d[u, v]) / M over the present v: thread t of 256 adds v = t, t + 256, ... in ascending
 *   order, the 256 partials go down the LDS tree (pairs i, i + 128; i, i + 64; ...; 0, 1).  mu of an absent sample is 0.
 * Spread: D0 = (sum_u (double)c_u mu_u) / M, the rows added in ascending order: the energy-distance self term of the full weighted
 *   sample, E d(X, X').
 * Herding, m picks without replacement among the present samples: r_c = 0; for j = 0 .. m - 1: score_c = mu_c - r_c / (j + 1) over
 *   the present, not yet chosen c; x_{j+1} = the c with the smallest score, the lowest c on a tie (compared as the order-preserving
 *   bit map of the signed double, then c); then r_c += d[c, x_{j+1}] for every remaining c.  pick_score[j] = the winning score.
 * Energy curve, for every prefix n = 1 .. m: musum_n = musum_{n-1} + mu_{x_n}; pair_n = pair_{n-1} + 2 r_{x_n} (r before x_n's own
 *   column is added); energy_n = ((2 musum_n) / n - pair_n / (n n)) - D0: the energy distance between the n chosen nets with equal
 *   weights and the full weighted sample.  >= 0 up to rounding; NOT monotone in n.  A random n-subset drawn with replacement has
 *   expected energy exactly D0 / n.
 * Subset evaluation: row b of subset_items [n_subsets, subset_size] holds item indices, repeats allowed; its measure is
 *   (1 / m_b) sum_k delta(item_sample[s_k]).  energy = ((2 sum_k mu) / m_b - (sum_{k, l} d) / (m_b m_b)) - D0; thread t of 256 adds
 *   k = t, t + 256, ... and the ordered pairs p = t, t + 256, ... -> (p / m_b, p % m_b), ascending, each down the LDS tree.
 * Outputs, any may be NULL: picks, energy, pick_score [m]; mu, count hold `room` entries of which U = *n_distinct are written;
 *   d0 [1]; subset_energy [n_subsets]; item_sample, sq_dist, outputs, n_samples, n_distinct exactly as ptnn_modes.
 * Refused: as ptnn_modes (the cap, M < 1, values together with w, room < n_items, a communicator attached); m < 0 or m > the present
 *   samples (the text gives both); n_subsets < 0; n_subsets > 0 without subset_items or with subset_size outside [1, 65536]; a
 *   subset entry outside [0, n_items); a subset that holds an absent sample.
 * Runs on the handle's stream behind everything queued and returns when done.  Touches no chain state, tape, counter or trace row. */
typedef struct ptnn_compress_spec {
    int32_t struct_bytes;         /* = sizeof(ptnn_compress_spec): ABI guard */
    /* source 1: the trace (used when w == NULL and values == NULL) */
    const int32_t *replicas;      /* local replica indices, or NULL = all */
    int32_t n_replicas;           /* entries of replicas (ignored when NULL) */
    int32_t step0, nsteps, thin;  /* trace rows step0, step0 + thin, ... < step0 + nsteps (thin >= 1) */
    /* source 2: host vectors */
    const float *w;               /* [n_w, P] or NULL */
    const int32_t *multiplicity;  /* [n_w] >= 0, or NULL = 1 each (sources 2 and 3) */
    int64_t n_w;
    /* input rows (sources 1 and 2) */
    int32_t x_source;             /* PTNN_PREDICT_X_HOST | _TRAIN | _TEST */
    int32_t n_rows;
    const float *x;               /* [n_rows, n_in] (host rows only) */
    /* source 3: a host matrix */
    const float *values;          /* [n_w, n_a] or NULL */
    int32_t n_a;
    int32_t m;                    /* picks: 0 <= m <= the present samples */
    const int32_t *subset_items;  /* [n_subsets, subset_size] item indices, or NULL */
    int32_t n_subsets, subset_size;
    int64_t room;                 /* entries that mu, count and item_sample each hold: >= n_items, else refused */
    /* outputs */
    int32_t *picks;               /* [m] distinct-sample indices, in herding order */
    double *energy;               /* [m] */
    double *pick_score;           /* [m] */
    double *mu;                   /* [n_items], U written */
    double *d0;                   /* [1] */
    double *subset_energy;        /* [n_subsets] */
    int32_t *count;               /* [n_items], U written */
    int32_t *item_sample;         /* [n_items] */
    double *sq_dist;              /* [U, U] packed */
    float *outputs;               /* [U, n] packed */
    int64_t *n_samples, *n_distinct;
} ptnn_compress_spec;

int ptnn_compress(ptnn_handle *h, const ptnn_compress_spec *spec);

/* the HIP stream (hipStream_t) all of this handle's work is queued on: lets the caller order its collectives after the
 * segment / before the swap kernels on the device instead of synchronising the host */
int ptnn_stream(ptnn_handle *h, void **hip_stream);

/* ---- results ---- */
/* traces of rows [step0, step0+nsteps) for all local replicas (row i+1 is written by MH step i; the rows must still be in
 * the ring: step0 >= steps_done + 1 - trace_capacity); any pointer may be NULL.
 * pos_w [R,nsteps,P] (REG:240,408,417); likeh [R,nsteps] = column 0 of likeh_list (REG:391 / CLS:404);
 * rmse_* / acc_* [R,nsteps] (REG:403-423); accept_count [R,nsteps] = accept_list (REG:380). */
int ptnn_get_traces(ptnn_handle *h, int step0, int nsteps, float *pos_w, float *likeh, float *rmse_train,
                    float *rmse_test, float *acc_train, float *acc_test, int32_t *accept_count);
/* The scalar trace rows as the device keeps them, rows [R, nsteps, 8] float32: {likeh, rmse_train, rmse_test, acc_train,
 * acc_test, accept_count (int32 bits), log alpha of the step as the kernel computed it (REG:372: diff_likelihood + diff_prior +
 * diff_prop; diagnostic, the parity tests measure the fp32 error of the MH decision with it), 0}.  Regression (task 0): the
 * acc_train slot -- identically 0 in the reference (REG:403) and in ptnn_get_traces -- holds eta = log tau^2 of the recorded
 * state here (the chain's eta after an accepted step; tests set the oracle's state from it).  Does not mark rows as
 * fetched.  Same range rules as ptnn_get_traces. */
int ptnn_get_trace_rows(ptnn_handle *h, int step0, int nsteps, float *rows);
/* Trace images: the trace download overlapped with sampling (the reference's chains write their files after their last step and
 * the parent reads them back, REG:454-481, 775-871; here rows can leave while later steps are sampled).  ptnn_trace_image: pinned
 * host copies owned by the handle, in the device's layout -- pos_w [R, n_samples, *row_floats] (the first n_param floats of a row
 * are the vector), rows [R, n_samples, 8] as ptnn_get_trace_rows describes them; allocated on the first call; needs every row
 * resident (trace_capacity 0) and non-compact traces.  ptnn_trace_image_fetch: behind everything queued on the handle so far
 * (ptnn_run returns once the steps are queued), copies rows [step0, step0+nsteps) of every local replica into the images on a
 * second stream and returns a ticket >= 0; marks the rows as fetched.  ptnn_trace_image_wait: blocks until that copy has landed.
 * A run's errors surface at ptnn_sync as always.  ptnn_set_state (a restart) forgets all tickets. */
int ptnn_trace_image(ptnn_handle *h, float **pos_w, int32_t *row_floats, float **rows);
int ptnn_trace_image_fetch(ptnn_handle *h, int step0, int nsteps);
int ptnn_trace_image_wait(ptnn_handle *h, int ticket);
/* num_swap / total_swap_proposals (REG:501-502, 680-688) */
int ptnn_get_swap_stats(ptnn_handle *h, int64_t *num_swap, int64_t *total_proposals, int32_t *rounds_done);
/* src permutation of every completed round, [rounds, R_global] (tests) */
int ptnn_get_swap_log(ptnn_handle *h, int32_t *src, int max_rounds);
/* current chain state per local replica: w [R,P], eta [R], likelihood [R] (tempered, possibly stale: Q12),
 * prior_current [R], num_accepted [R], langevin_count [R] (Langevin steps proposed, REG:347), langevin_accepted [R]
 * (of those, accepted; cooperative, speculative and packed schedules); any pointer may be NULL */
int ptnn_get_state(ptnn_handle *h, float *w, float *eta, float *likelihood, float *prior, int32_t *num_accepted,
                   int32_t *langevin_count, int32_t *langevin_accepted);

/* label_swap = 1: label[R_global] = the temperature index every chain slot of the whole ladder holds after the rounds queued so
 * far (identity without label swapping) */
int ptnn_get_labels(ptnn_handle *h, int32_t *label);

/* ---- checkpoint / resume (the reference has none) ----
 * The RNG is counter based, so the state of the chains is small: (w, eta), cached gradient, recorded row, likelihood / prior /
 * counters per replica, posted scalars, swap counters and log, step and round indices.  ptnn_checkpoint_save writes it into a
 * caller buffer of ptnn_checkpoint_size bytes; ptnn_checkpoint_load on a handle created with the same chain configuration
 * (after ptnn_set_data, instead of ptnn_set_state) continues the chains bit for bit.  Trace rows are not part of it: rows up
 * to the checkpoint step stay with whoever fetched them, and ptnn_get_traces of the restored handle refuses them. */
int ptnn_checkpoint_size(ptnn_handle *h, int64_t *bytes);
int ptnn_checkpoint_save(ptnn_handle *h, void *buf, int64_t bytes);
int ptnn_checkpoint_load(ptnn_handle *h, const void *buf, int64_t bytes);

/* ---- the model functions on their own (same device code as the sampler) ---- */
/* Network.evaluate_proposal + likelihood_func + prior_likelihood for n weight vectors w [n,P] (REG:120-134, 200-221;
 * CLS:134-153, 209-230); tau_sq [n] (ignored for CLS, may be NULL).  out [n,8] =
 * {loglik_train (untempered), rmse_train, rmse_test, acc_train, acc_test, prior, loglik_test, 0}. */
int ptnn_evaluate(ptnn_handle *h, const float *w, const float *tau_sq, int n, float *out);
/* Network.langevin_gradient(train, w, depth=1) for n weight vectors (REG:99-118, CLS:114-132) */
int ptnn_langevin_gradient(ptnn_handle *h, const float *w_in, int n, float *w_out);
/* What ONE sequential SGD epoch (langevin_gradient of one chain, REG:99-118) costs on this device, in milliseconds: `reps` epochs
 * back to back on one wavefront, timed inside the kernel with the constant-rate counter (s_memrealtime; the rate comes from
 * hipDeviceAttributeWallClockRate).  An accepted Langevin step makes the next proposal wait for a fresh epoch, so accepted steps x
 * this number is the floor of a swap interval whatever the number of speculative slots (bench.py: roofline.chain).
 * ms_per_epoch[2]: [0] one epoch; [1] wide nets (n_hidden > 64) only: a PAIR of epochs run through one row loop (what two Langevin
 * steps of one speculative window cost together), else 0. */
int ptnn_time_sgd_epoch(ptnn_handle *h, const float *w, int reps, double *ms_per_epoch);
/* What a round of the prefetching-tree schedule cannot do without, timed on the device (in-kernel constant-rate counter, `reps`
 * repetitions): ms[0] = one forward pass over all rows with the likelihood and prior sums by one work-group of the handle's block
 * size (what a node does between its proposal and its record); ms[1] = one {tag, value} granule from one work-group to another,
 * one way (half a round trip between two work-groups of one XCD), through the XCD's L2 when xcd_local != 0 and the two groups
 * report the same XCC id (ms[2] = 1), else through the agent-scope path.  bench.py's roofline.tree floor is made of these. */
int ptnn_time_tree_round(ptnn_handle *h, const float *w, int reps, int xcd_local, double *ms);
/* the random tape of MH step `step` of global replica `replica`: noise [P] normals, scal[3] = {lx, u, n_eta} */
int ptnn_tape(ptnn_handle *h, int replica, int step, float *noise, float *scal);

/* What this handle will launch, as one line of JSON text written into buf (returns its length, or negative): the segment
 * kernel the schedule resolved to for this topology / data set / replica count, its grid, block and dynamic LDS size, the
 * work-groups per replica and speculative slots per round, and what the runtime reports for it (blocks per CU from
 * hipOccupancyMaxActiveBlocksPerMultiprocessor, VGPRs, scratch bytes).  After ptnn_set_data.  The reference has no
 * counterpart (its "schedule" is one OS process per chain, REG:709-712); bench.py and the profiles name kernels with it. */
int ptnn_describe(ptnn_handle *h, char *buf, int nbytes);

/* timing of the dominant kernel, measured with HIP events on the library's stream around every segment launch
 * since the last reset: launches, total milliseconds */
int ptnn_kernel_time(ptnn_handle *h, int reset, int64_t *launches, double *total_ms);

/* cycle sums per phase of the speculative kernel, replica 0 / wave 0; all zero unless the library was built with
 * -DPTNN_STAMPS (diagnostic build, never the product).  160 entries: [0..8] phase sums, [9] rounds, [16+2r], [17+2r] =
 * cycles and rounds of replica r < 64; reading resets. */
int ptnn_debug_stamps(ptnn_handle *h, uint64_t *out16);

/* ---- host-side helper (no GPU): the text dump the result-file layout requires ---- */
/* np.savetxt(path, data[rows, cols], fmt=fmt) with ' ' between columns and '\n' after rows (REG:454-481, 864-868).
 * fmt is one printf floating conversion such as "%.18e", "%1.8f", "%1.2f". */
int ptnn_savetxt(const char *path, const double *data, int64_t rows, int64_t cols, const char *fmt);
/* the same for float32 data as the device's traces are fetched (ptnn_get_traces): row r starts at data + r * row_stride; every
 * value is printed as the double it converts to, exactly as np.savetxt prints a float32 array; append != 0 continues an existing
 * file (a run written in windows).  Both savetxt entry points produce np.savetxt's bytes: values are formatted by exact integer
 * arithmetic (correctly rounded, ties to even, as glibc's printf), printf itself only for formats or magnitudes outside that
 * path, and a row identical to the one before it (a rejected MH step: pos_w[i+1] = pos_w[i], REG:417) reuses that row's text. */
int ptnn_savetxt_f32(const char *path, const float *data, int64_t rows, int64_t cols, int64_t row_stride, const char *fmt, int append);
/* n_files such files (the per-chain files of a window of trace rows, REG:454-481) by `threads` host threads, taken in the order
 * given (put the large ones first); returns when all are written, < 0 with the first failure's message */
int ptnn_savetxt_f32_batch(int n_files, const char *const *paths, const float *const *data, const int64_t *rows, const int64_t *cols,
                           const int64_t *row_stride, const char *const *fmts, int append, int threads);

/* in place: every value as np.loadtxt would read it back after np.savetxt(fmt=fmt) (show_results re-reads the per-chain
 * files, REG:795-831) */
int ptnn_text_round(double *values, int64_t n, const char *fmt);
int ptnn_text_round_f32(const float *in, double *out, int64_t n, const char *fmt);
/* out[p][c * m + t] = pos_w[c][first_row + t][p] with m = n_rows - first_row, as float64: the posterior matrix show_results
 * returns (REG:795-797, 848: every chain's pos_w file read back, burn-in cut, chains side by side, transposed).
 * pos_w [n_chains, n_rows, row_floats >= n_param] float32 (row_floats == n_param as ptnn_get_traces delivers it, the padded row of
 * ptnn_trace_image); out [n_param, n_chains * m]; `threads` host threads. */
int ptnn_posterior_matrix(const float *pos_w, int64_t n_chains, int64_t n_rows, int64_t n_param, int64_t row_floats, int64_t first_row,
                          double *out, int threads);

#ifdef __cplusplus
}
#endif
#endif /* PTNN_H */
