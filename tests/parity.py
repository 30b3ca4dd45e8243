"""Shared helpers of the GPU parity tests and of __graft_entry__.smoke(): run the HIP path through the C ABI and the
CPU oracle on the same seeded inputs and compare.  The oracle is the checker here, never the product."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ptnn_oracle as orc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# fp32 kernel vs float64 oracle: unit values rel 1e-5 / abs 1e-6, log-likelihood sums rel 1e-5 (+ abs 2e-3
# on sums of several hundred terms), MH decisions identical until |log alpha - log u| is inside the fp32 error of log alpha.
RTOL, ATOL = 2e-5, 2e-6

# ---- the fp32 error of the MH decision: measured, not guessed ----------------------------------------------------------------
# log alpha = (lik_prop - lik) + (prior_prop - prior) + diff_prop (REG:365-372) is a small difference of large terms, so its
# fp32 error is proportional to their size `scale` = |lik_prop| + |lik| + |prior_prop| + |prior| + (|first| + |second|) / T
# (oracle: Replica.last_scale), not to log alpha.  The kernels record the log alpha they decided on (column 6 of
# ptnn_get_trace_rows), so the error is measured directly against the float64 oracle on the same tape.  On the MI355X, over every
# step of the nine F4 trajectories (profiles/tools/logalpha_probe.py -> profiles/r02_logalpha_error.json):
#
#   trajectory (net, kernel)                     steps   scale (median)   max |error|   max |error| / scale
#   reg_rw          4-5-1    speculative          199        183            8.7e-5          9.2e-7
#   reg_lg          4-5-1    packed                99        519            5.8e-4          3.3e-7
#   reg_lg_mackey   4-10-1   speculative           59        758            4.4e-4          5.4e-7
#   cls_rw          4-12-3   cooperative          199        423            1.8e-5          4.2e-8
#   cls_lg          4-12-3   speculative           99        810            6.6e-4          7.6e-7
#   cls_rw_ions     34-50-2  cooperative (MFMA)    59       6225            2.0e-4          3.3e-8
#   reg_rw_noswitch 4-5-1    speculative           56        255            2.4e-5          6.9e-8
#   reg_lg_wide     32-96-1  wide                  29      12980            1.5e-3          1.1e-7
#   cls_lg_wide     34-100-2 wide                  29      12386            2.0e-3          1.2e-7
#
# i.e. below SURVEY 8d's 1e-3 for every net of BASELINE configs 1-4 and 16 ulp of the largest term at worst.  The bound the
# tests hold every step to is twice the largest measured ratio; a decision may differ from the oracle's only where log u lies
# within that bound of the oracle's log alpha (and, where the kernel's value is at hand, between the two values).
# With swap rounds the reference keeps `likelihood` and `prior_current` of the state that LEFT a slot (Q12, REG:435-438): until
# the next accepted step log alpha compares a fresh likelihood of the arrived state with a stale one of another state, so the
# fp32 evaluation errors of the two no longer cancel (a single chain's proposal and current state differ by one small step and
# round alike).  Measured over every multi-replica test of the suite (PTNN_PARITY_PROBE=file pytest -m gpu, condensed in
# profiles/r02_logalpha_error.json): at most 8.0e-6 of the scale on such steps (Mackey-Glass, 64 replicas, tau^2 ~ 1e-4:
# 2.6e-2 on a scale of 3275), 5.1e-6 on the other steps of runs with swaps (Sunspot, 64 replicas: the arrived state carries the
# fp32 history of another chain, and the prior stays stale across the temperature switch).
LOGALPHA_REL = 2e-6              # single chain: 2 x the largest measured ratio (9.2e-7)
LOGALPHA_REL_COUPLED = 1e-5      # chains coupled through swaps, likelihood current: 2 x 5.1e-6
LOGALPHA_REL_STALE = 2e-5        # steps deciding on a stale likelihood after a swap (Q12): 2.5 x 8.0e-6
LOGALPHA_ABS = 1e-5              # v_exp_f32 and the compare u < exp(log alpha) in fp32
SWAP_L_REL = 2e-5                # a posted scalar L is one likelihood evaluation (times T for REG): same class as a stale step
MIN_IDENTICAL_STEPS = 50         # decisions identical for at least the first 50 steps
# Whole runs followed to the end (follow_device_run): over 10^5 - 10^6 steps the chains visit states where the likelihood is far
# more sensitive than at the start (Sunspot after burn-in: tau^2 ~ 1e-4, so one fp32 ulp of a prediction moves log alpha by
# ~1e-2).  Measured on the MI355X (profiles/r03_follow_probe.jsonl, PTNN_PARITY_PROBE): at most 1.9e-5 of the scale over the
# 639 936 steps of the headline run (2.0e-5 on stale steps), 5.3e-5 under shared noise, 1.4e-5 Mackey-Glass, 7e-6 / 6e-8 / 4e-8 on
# the shorter Sunspot / Iris / Ionosphere runs -- and NOT ONE MH or cascade decision of the headline run differed from the
# float64 oracle's.  The bound for followed runs is twice the largest of these.
LOGALPHA_REL_FOLLOWED = 1.1e-4
# The same whole runs with the device's STATE imposed as well (follow_device_run(sync=True), the default): after every accepted
# step the oracle continues from the (w, eta) the device recorded, its likelihood / prior re-evaluated in float64 there.  Two
# classes of comparison come out of it (measured on the MI355X: profiles/r04_follow_synced.jsonl):
#
# (1) IDENTICAL INPUTS -- every accepted step re-evaluated by the oracle at the device's own recorded proposal (w', eta') from the
#     common state (oracle/ptnn_oracle_c.c: orc_replica_run, la_sync).  What differs is the arithmetic of ONE evaluation.
#     A-priori model: log alpha is a sum of N = 2 (Ntr + P) + O(1) fp32 terms (two log-likelihood sums over the training rows,
#     two priors over the weights, the Langevin ratio), each formed by k ~ 25 roundings (the forward pass of a row: H fused
#     multiply-adds, two hardware exp / rcp pairs at 1 ulp, the squared residual over tau^2) and summed through reductions of
#     depth log2 N ~ 9: |error| <= (k + log2 N) eps32 sum |terms| ~ 34 x 5.96e-8 x scale = 2.0e-6 x scale; a Langevin step adds
#     the fp32 SGD epoch of the proposal (298 sequential row updates) inside first = -|w - sgd(w')|^2 / 2 step^2.  Measured maxima
#     over every accepted step of every followed run (10^4 - 10^5 per run): 1.97e-6 of the scale (Sunspot 64 x 1500), 1.2e-6 on
#     the headline's 12 397 / 13 342 accepted steps, 6.5e-7 Mackey-Glass, 4e-8 - 8e-8 on the classification nets; in absolute
#     terms 7.6e-4 on the headline -- SURVEY 8d's 1e-3 holds there -- 3.0e-3 on Mackey-Glass (tau^2 ~ 3e-5: 6 of 5030 steps above
#     1e-3).  Bound: 2 x the largest measured ratio.  The recorded log-likelihood of the step is held the same way.
#     A defect of 1e-6 relative in one likelihood sum (scale ~ 1.5e3: 1.5e-3 absolute) is outside this bound on every ACCEPTED
#     step -- 2 % of the headline's steps.  The other 98 % get the same class through the rebuilt proposal: see below.
#
# (2) ALL STEPS from the common state, each side forming ITS OWN proposal.  The named term that separates (2) from (1) is the
#     POSITION of the proposal: w' = w + step n (or sgd(w) + step n) is rounded to float32 on the device and n comes from the
#     hardware log / sin / cos, so the two proposals differ by ~ half an ulp (2.4e-7 at |w| ~ 4) per weight -- and with
#     tau^2 ~ 1e-4 the Gaussian log-likelihood changes by |grad| dw ~ (N rmse / tau^2) |dfx/dw| dw = 1e-4 .. 1e-2 over such a
#     distance (the fp32 SGD epoch of a Langevin proposal moves w' by another ~ 4e-6).  Both are valid proposals of the same
#     kernel; the decisions still agree (0 of 639 936 on the headline) because |log alpha - log u| is rarely that small.
#     Measured maxima at the BASELINE run lengths: regression 3.6e-5 of the scale (Mackey-Glass 64 x 10 000, tau^2 ~ 3e-5: 0.13
#     absolute; headline 1.6e-5 / 1.8e-2), classification 8.9e-8 (no 1 / tau^2 in a multinomial likelihood).  Bounds: 2.5 x
#     the largest measured ratio per task.  The recorded log-likelihood of a REJECTED step (the likeh column) is the same
#     quantity at the same two positions and is held to the same bound.  This class stays as the outer assertion of every
#     followed run; where ident_all is on, the rejected steps are ALSO held to class (1):
LOGALPHA_REL_SYNCED = {0: 1e-4, 1: 2e-6}         # by task (0 regression, 1 classification), every step, fresh or stale
LOGALPHA_REL_IDENT = 4e-6                        # accepted steps re-evaluated at the device's own proposal
LIK_REL_IDENT, LIK_ABS_IDENT = 2e-6, 1e-4        # recorded log-likelihood of an accepted step: rel of (|lik| + Ntr) (the sum's terms change sign) + abs
# (1) on EVERY step, rejected ones included (follow_device_run(ident_all=True), tests/test_gpu_follow_ident.py): a rejected step leaves
#     no proposal in the trace, but every schedule forms w' = fmaf(step_w, noise, base), eta' = fmaf(step_eta, n_eta, eta) with base =
#     the state or its SGD epoch, the library hands out its own tape and epoch, and the state is common -- so the device's proposal is
#     rebuilt bit for bit (rebuild_device_proposals; checked against the recorded row on every accepted step: 0 mismatches in 40 000
#     steps under every schedule, Langevin proposals included) and the oracle evaluated there.  The a-priori model above does not
#     depend on the verdict.  Measured on the MI355X, largest |error| / scale per class of step over the suite's seed and three others of each case of
#     tests/test_gpu_follow_ident.py (profiles/follow_ident_all.jsonl; fresh | stale cached likelihood):
#
#       case (net, kernel)                            accepted rw        rejected rw        accepted Langevin   rejected Langevin    likeh
#       cooperative     4-5-1   segment_kernel        7.0e-7 | 2.5e-7    7.2e-7 | 4.1e-7    6.6e-7 | 5.6e-7     3.9e-6 | 1.8e-6      2.2e-7
#       speculative     4-5-1   segment_spec_kernel   7.9e-7 | 2.5e-7    7.2e-7 | 3.9e-7    1.4e-7 | 1.3e-7     3.9e-6 | 1.9e-6      2.7e-7
#       packed          4-5-1   segment_pack_kernel   7.9e-7 | 2.5e-7    7.2e-7 | 3.9e-7       -   | 5.6e-7     3.9e-6 | 1.9e-6      2.7e-7
#       packed, shared noise                          9.2e-7 | 2.2e-7    7.3e-7 | 5.2e-7    2.6e-7 |    -       3.5e-6 | 4.5e-6      2.3e-7
#       packed, 4 CUs   4-10-1  segment_packm_kernel  2.9e-7 | 1.7e-7    1.8e-7 | 1.7e-7    4.3e-7 | 3.9e-7     1.0e-6 | 8.9e-7      8.1e-7
#       5 inputs        5-5-1   segment_pack_kernel   3.8e-7 | 7.8e-8    5.3e-7 | 1.7e-7       -   | 3.4e-7     2.5e-6 | 1.6e-6      2.4e-7
#       tree            4-12-3  segment_tree_kernel   6.1e-8 | 4.3e-8    3.8e-8 | 5.6e-8                                             1.2e-7
#       classification  4-12-3  segment_spec_kernel   4.8e-8 | 4.0e-8    5.8e-8 | 5.3e-8    3.7e-7 | 7.6e-8     9.3e-7 | 7.4e-7      1.3e-7
#       MFMA forward    34-50-2 segment_kernel        3.8e-8 | 3.4e-8    3.9e-8 | 4.0e-8                                             1.1e-7
#       wide, resident  32-96-1 segment_wide_res      7.3e-8 | 4.4e-8    7.0e-8 | 6.7e-8    2.0e-7 | 5.6e-8     9.0e-8 | 7.8e-8      9.0e-7
#       wide, streaming 32-70-1 segment_wide_kernel   6.5e-8 | 3.2e-8    8.8e-8 | 4.1e-8    5.2e-8 | 5.5e-8     6.1e-8 | 5.6e-8      1.5e-6
#       wide, resident  32-128-1, 256 rows            1.3e-7 | 4.4e-8    5.5e-8 | 5.6e-8    2.9e-7 | 4.2e-8     6.7e-8 | 8.1e-8      1.1e-6
#
#     Random-walk steps, rejected or accepted, fresh or stale, stay below 1e-6 and the likeh column below 2e-6 of (|lik| + Ntr): the
#     constants of the accepted steps hold unchanged on them.  REJECTED LANGEVIN steps of the 4-H-1 nets reach 4.47e-6 (3.9e-6 on
#     the seeds the suite does not run).  The term is named and measured: first = -|w - sgd(w')|^2 / 2 step^2 holds the fp32 SGD epoch
#     of the proposal (298 sequential row updates, up to 5e-6 off the float64 epoch per weight), a rejected Langevin proposal is
#     rejected BECAUSE |w - sgd(w')| is large -- `first` is 60 - 80 % of the scale of such a step on Sunspot -- and its error
#     2 |w - sgd(w')| d / 2 step^2 grows with that distance.  With the device's own epoch of w' (ptnn_langevin_gradient)
#     put into `first` in float64, 4.39e-6 of the worst step's 4.47e-6 are accounted for and 2.6e-7 of the scale at most is left on
#     any Langevin step (profiles/follow_ident_all.jsonl, "diag" rows) -- the random-walk level.  The bound for Langevin steps is
#     twice the largest measured ratio; it stays below LOGALPHA_REL_COUPLED.
LOGALPHA_REL_IDENT_ALL = {0: LOGALPHA_REL_IDENT, 1: 9e-6}     # EVERY step at the device's rebuilt proposal, by proposal: random walk, Langevin
LIK_REL_IDENT_ALL = LIK_REL_IDENT


def logalpha_slack(scale, rel=LOGALPHA_REL):
    return rel * float(scale) + LOGALPHA_ABS


def check_logalpha_error(la_gpu, la_oracle, scale, label="", rel=LOGALPHA_REL):
    """Every step whose inputs were still identical: the kernel's log alpha within the measured fp32 bound of the oracle's.
    `rel`: a constant or one value per step."""
    la_gpu, la_oracle, scale = (np.asarray(v, dtype=np.float64) for v in (la_gpu, la_oracle, scale))
    rel = np.broadcast_to(np.asarray(rel, dtype=np.float64), scale.shape)
    ok = np.isfinite(la_oracle) & np.isfinite(la_gpu)
    err = np.abs(la_gpu - la_oracle)[ok]
    lim = (rel * scale + LOGALPHA_ABS)[ok]
    if os.environ.get("PTNN_PARITY_PROBE"):                 # measurement mode: record the ratios instead of judging them
        import json
        with open(os.environ["PTNN_PARITY_PROBE"], "a") as f:
            ratio = err / scale[ok]
            k = int(np.argmax(ratio)) if err.size else -1
            f.write(json.dumps(dict(label=label, test=os.environ.get("PYTEST_CURRENT_TEST", ""), steps=int(err.size),
                                    max_err=float(err.max()) if err.size else 0.0, max_ratio=float(ratio.max()) if err.size else 0.0,
                                    at_step=int(np.flatnonzero(ok)[k]) if err.size else -1,
                                    scale_there=float(scale[ok][k]) if err.size else 0.0,
                                    rel_there=float(rel[ok][k]) if err.size else 0.0,
                                    max_ratio_by_rel={str(v): float(ratio[rel[ok] == v].max()) for v in np.unique(rel[ok])})) + "\n")
        return float(err.max()) if err.size else 0.0
    bad = err > lim
    assert not bad.any(), (f"{label}log alpha off by {err[bad].max():.3g} (bound {lim[bad][np.argmax(err[bad])]:.3g}) at step "
                           f"{int(np.flatnonzero(ok)[np.flatnonzero(bad)[np.argmax(err[bad])]])}")
    return float(err.max()) if err.size else 0.0


def check_divergence(la_oracle, logu, scale, la_gpu=None, label="", rel=LOGALPHA_REL):
    """The two sides decided differently at a step: legitimate only if the oracle's decision was closer than the fp32 error of
    log alpha, and (when the kernel's own log alpha is known) log u lies between the two values."""
    gap = abs(la_oracle - logu)
    assert np.isnan(gap) or gap <= logalpha_slack(scale, rel), f"{label}decision flipped with |log alpha - log u| = {gap:.3g} > {logalpha_slack(scale, rel):.3g}"
    if la_gpu is not None and np.isfinite(la_gpu) and np.isfinite(la_oracle):
        lo, hi = min(la_oracle, la_gpu), max(la_oracle, la_gpu)
        assert lo - LOGALPHA_ABS <= logu <= hi + LOGALPHA_ABS, f"{label}log u = {logu} not between the two log alphas {la_oracle}, {la_gpu}"


def datasets():
    return dict(np.load(os.path.join(GOLDEN, "datasets.npz")))


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def make_sampler(task, topo, train, test, *, R_local, R_global, first, S, si, use_lg, lr, seed, l_prob=0.5, waves=0,
                 schedule=0, groups=0, trace_capacity=0, forward_bf16=0, swap_rule=0, shared_noise=0, label_swap=0):
    import ptnn_amd
    from ptnn_amd import _lib
    pt = S * 0.6
    s = _lib.Sampler(device_id=0, task=task, n_in=topo[0], n_hidden=topo[1], n_out=topo[2], n_replicas_local=R_local,
                     n_replicas_global=R_global, first_global_replica=first, n_samples=S, swap_interval=si,
                     pt_switch_step=int(pt) if pt == int(pt) else -1, use_langevin=int(bool(use_lg)),
                     waves_per_replica=waves, schedule=schedule, groups_per_replica=groups, trace_capacity=trace_capacity, forward_bf16=forward_bf16, swap_rule=swap_rule, shared_noise=int(shared_noise), label_swap=int(label_swap), l_prob=l_prob, learn_rate=lr, step_w=0.025, step_eta=0.2,
                     sigma_squared=25.0, nu_1=0.0, nu_2=0.0, seed=seed)
    s.set_data(train, test)
    return s


def compare_replica_trace(tr, r, rep, label="", limit=None):
    """tr: Sampler.traces() dict; rep: oracle Replica run over the same tape.  Returns the first step whose MH
    decision differs (or None).  Everything before it must agree within the fp32 tolerances.  `limit`: compare only the first
    `limit` rows (the chains are known to part there for another reason, e.g. a near-tie decision in another replica whose
    state arrived through an exchange)."""
    S = rep.S if limit is None else min(rep.S, int(limit))
    acc_g = tr["accept"][r].astype(np.int64)[:S]
    acc_o = rep.accept_list.astype(np.int64)[:S]
    diff = np.nonzero(acc_g != acc_o)[0]
    first = int(diff[0]) if diff.size else None          # index into accept_list: decision of step first-2 differed
    upto = S if first is None else first - 1             # rows [0, upto) were produced by identical decisions
    if upto > 1:
        np.testing.assert_allclose(tr["pos_w"][r, :upto], rep.pos_w[:upto], rtol=RTOL, atol=2e-5, err_msg=label + " pos_w")
        lk = rep.likeh[:upto, 0]
        np.testing.assert_allclose(tr["likeh"][r, :upto], lk, rtol=5e-5, atol=5e-3, err_msg=label + " likeh")
        for nm in ("rmse_train", "rmse_test"):
            np.testing.assert_allclose(tr[nm][r, :upto], getattr(rep, nm)[:upto], rtol=1e-4, atol=1e-6, err_msg=label + nm)
        for nm in ("acc_train", "acc_test"):
            np.testing.assert_allclose(tr[nm][r, :upto], getattr(rep, nm)[:upto], rtol=1e-5, atol=1e-4, err_msg=label + nm)
    return first


class OracleRun:
    """Oracle replicas advanced step by step, recording log alpha and u of every step (for divergence analysis)."""

    def __init__(self, pt):
        self.pt = pt
        self.logalpha = np.full((pt.R, pt.S), np.nan)
        self.logu = np.full((pt.R, pt.S), np.nan)
        self.scale = np.full((pt.R, pt.S), np.nan)
        self.stale = np.zeros((pt.R, pt.S), dtype=bool)

    def run(self):
        pt = self.pt
        for i in range(pt.S - 1):
            for r, rep in enumerate(pt.replicas):
                rep.step(i)
                self.logalpha[r, i] = rep.last_logalpha
                self.logu[r, i] = np.log(rep.last_u)
                self.scale[r, i] = rep.last_scale
                self.stale[r, i] = rep.last_stale
            pt._steps_done = i + 1
            if orc.swap_trigger(pt.task, i, pt.si):
                pt.swap_round()
        rounds = int(pt.S / pt.si) if pt.si > 0 else 0
        if pt.swap_rule == 0 and rounds > pt.rounds_done:
            pt.swap_round(L=[rep.likelihood for rep in pt.replicas], apply=False)
        return self


def handoff_step(task, k, si):
    """MH step after which swap round k (0-based) runs: REG i = (k+1) si (REG:427), CLS i = (k+1) si - 1 (CLS:438)."""
    return (k + 1) * si - (0 if task == orc.TASK_REG else 1)


def check_swap_divergence(pt, k, src_gpu, label=""):
    """Round k of the cascade came out differently on the device: legitimate only if the first pair decided differently was
    closer than the fp32 error of the two posted scalars it compares (REG:674: u < 0.5 exp(min(709, L2 - L1)))."""
    L = pt.L_log[k]
    u = pt.tape.swap_uniforms(k, pt.R - 1)
    src_o = pt.src_log[k]
    c = 0
    for j in range(pt.R - 1):
        if src_gpu[j] != src_o[j]:
            d = min(709.0, L[j + 1] - L[c])
            margin = abs(np.log(u[j]) - (np.log(0.5) + d))
            bound = SWAP_L_REL * (abs(L[j + 1]) + abs(L[c])) + LOGALPHA_ABS
            assert margin <= bound, f"{label}swap round {k} pair {j}: decision flipped with margin {margin:.3g} > {bound:.3g}"
            return j
        if src_o[j] != j + 1:
            c = j + 1
    raise AssertionError(f"{label}swap round {k}: permutations differ only in the last slot?")


def check_run_against_oracle(s, tr, o, label="", limit=None):
    """A whole ladder (swap rounds included) against the oracle run `o` (OracleRun) on the same tape.  The replicas are coupled
    through the swaps, so only the EARLIEST difference is attributable: either an MH decision or a cascade decision.  Up to it
    every trace row agrees within the fp32 tolerances and the kernel's log alpha is within the measured fp32 bound of the
    oracle's on every step; the difference itself must be a decision inside that bound.  Returns the list of first differing
    accept_list indices per replica (None = none) within the compared range."""
    pt = o.pt
    log = s.swap_log()
    swap_div = next((k for k in range(min(len(log), len(pt.src_log))) if list(log[k]) != list(pt.src_log[k])), None)
    if swap_div is not None and pt.swap_rule == 0:
        rows = handoff_step(pt.task, swap_div, pt.si) + 2     # rows [0, rows) were written before that round moved anything
        limit = rows if limit is None else min(int(limit), rows)
    # earliest differing MH decision of ANY replica: from there on a swap can carry the difference into every other slot, so
    # all replicas are compared on the rows written before it only
    S_cmp = pt.S if limit is None else min(pt.S, int(limit))

    def first_diff(r):
        d = np.nonzero(tr["accept"][r].astype(np.int64)[:S_cmp] != pt.replicas[r].accept_list.astype(np.int64)[:S_cmp])[0]
        return int(d[0]) if d.size else None
    fd = [first_diff(r) for r in range(pt.R)]
    early = [f for f in fd if f is not None]
    if early:
        limit = max(min(early) - 1, 2)                       # rows [0, first - 1) of the earliest diverging replica
    firsts = [compare_replica_trace(tr, r, pt.replicas[r], f"{label}r{r} ", limit=limit) for r in range(pt.R)]
    if early:                                               # compare_replica_trace saw rows below the divergence only: put it back
        firsts[fd.index(min(early))] = min(early)
    lag = s.log_alpha()
    div = [f for f in firsts if f is not None]
    upto = (pt.S - 1) if not div else min(div) - 2           # steps [0, upto) had identical inputs in every replica
    if limit is not None:
        upto = max(min(upto, int(limit) - 1), 0)
    coupled = pt.rounds_done > 0 and pt.swap_rule == 0
    for r in range(pt.R):
        rel = np.where(o.stale[r, :upto], LOGALPHA_REL_STALE, LOGALPHA_REL_COUPLED if coupled else LOGALPHA_REL)
        check_logalpha_error(lag[r, :upto], o.logalpha[r, :upto], o.scale[r, :upto], f"{label}r{r} ", rel=rel)
    if div:
        r = firsts.index(min(div))
        i = min(div) - 2
        rel = LOGALPHA_REL_STALE if o.stale[r, i] else (LOGALPHA_REL_COUPLED if coupled else LOGALPHA_REL)
        check_divergence(o.logalpha[r, i], o.logu[r, i], o.scale[r, i], lag[r, i], f"{label}r{r} step {i}: ", rel=rel)
    elif swap_div is not None and pt.swap_rule == 0:
        check_swap_divergence(pt, swap_div, list(log[swap_div]), label)
    return firsts


def follow_cascade(L, u, src_dev, label="", strict=True):
    """One round of the reference's bubble pass (REG:659-690) walked pair by pair along the DEVICE's permutation: at
    every pair the oracle's decision (from its own float64 scalars and the carried state the device's history implies) must equal
    the device's, or differ inside the fp32 error of the two posted scalars it compares.  Returns the number of such pairs."""
    R = len(L)
    c, forced = 0, 0
    for j in range(R - 1):
        d = L[j + 1] - L[c]
        d = 709.0 if not (d < 709.0) else d
        nat = np.log(u[j]) < np.log(0.5) + d
        dev = int(src_dev[j]) == j + 1
        if not dev:
            assert int(src_dev[j]) == c, f"{label}pair {j}: slot receives {src_dev[j]}, not the carried state {c}"
        if bool(nat) != dev:
            margin = abs(np.log(u[j]) - (np.log(0.5) + d))
            bound = SWAP_L_REL * (abs(L[j + 1]) + abs(L[c])) + LOGALPHA_ABS
            assert margin <= bound or not strict, f"{label}pair {j}: swap decision differs with margin {margin:.3g} > {bound:.3g}"
            forced += 1
        if not dev:
            c = j + 1
    assert int(src_dev[R - 1]) == c, f"{label}last slot receives {src_dev[R - 1]}, not the carried state {c}"
    return forced


def follow_device_run(s, tr, pt, label="", threads=8, row_rtol=None, row_atol=None, sync=True, arrays=None, study=False,
                      ident_all=False, eta0=None):
    """EVERY step of a whole run against the oracle, not only the prefix up to the first fp32 coin flip: the oracle FOLLOWS the
    device.  `pt` is a PTOracle whose chains are C chains (ptnn_oracle_c.adopt) started from the device's initial weights.  It
    is advanced interval by interval with the device's own MH decisions imposed (from the accept counters of the trace) and the
    device's swap permutations imposed (from the swap log); at every step it records what it WOULD have decided.  Held:

      * the kernel's log alpha within the measured fp32 bound of the oracle's on every step of every chain (inputs now stay
        comparable to the end of the run);
      * every MH decision the two sides take differently lies inside that bound (check_divergence), every cascade pair decision
        they take differently inside the bound of the two posted scalars (follow_cascade);
      * every trace row (pos_w, likeh, rmse, accuracy) of the whole run within row_rtol / row_atol -- wider than the prefix
        tolerances because fp32 round-off now accumulates over thousands of accepted steps instead of fifty;
      * the swap counters.

    sync=True (default) -- the per-step form: the device's DECISIONS and its STATE are imposed.  After every accepted step the
    oracle chain continues from the (w, eta) the device recorded for that step (pos_w row; eta from the regression's raw scalar
    row, Sampler.eta_trace), with its cached likelihood and prior re-evaluated in float64 from that state
    (oracle/ptnn_oracle_c.c: orc_replica_set_state); swap rounds then move those same values.  Both sides enter every step
    from the same numbers, so the difference in log alpha and in the trace row of a step is the fp32 error of THAT step --
    held to the per-step bounds (LOGALPHA_REL_SYNCED on every step; LOGALPHA_REL_IDENT / LIK_*_IDENT on the accepted steps, which
    the oracle re-evaluates at the device's own proposal: identical inputs; the prefix tolerances for the rows) -- instead of the drift
    two chains accumulate over thousands of accepted steps times the conditioning of the likelihood (tau^2 ~ 1e-4), which is
    what sync=False measures and holds to LOGALPHA_REL_FOLLOWED (kept as the drift report).

    ident_all=True (with sync) -- the identical-input class on EVERY step, rejected ones included: the device's proposal of every
    step is rebuilt bit for bit from its own tape and, on Langevin steps, its own epoch (rebuild_device_proposals), the oracle is
    evaluated there (ident_all_eval) and the recorded log alpha and likeh of every step are held to LOGALPHA_REL_IDENT /
    LIK_*_IDENT (ident_all_check).  eta0: the device's start-up eta per chain (device_startup_eta; NaN = not known), imposed on
    the oracle's chains before the first step.

    swap_rule 0 without label swapping.  Returns a report: steps, forced MH decisions, forced cascade pairs, max log-alpha
    error / scale by class of step, absolute maxima.  `arrays`: a dict that receives the per-step arrays behind the report
    (log alpha error of every step, of the accepted steps at identical inputs, of their recorded log-likelihood).  `study`
    (tolerance studies of a deliberately less precise arithmetic, profiles/tools/bf16_study.py): nothing is asserted, decisions
    taken differently outside the coin-flip bound are counted (`flips_outside_bound`) instead of refused."""
    from concurrent.futures import ThreadPoolExecutor
    assert pt.swap_rule == 0 and not pt.label_swap
    assert sync or not ident_all, "the all-steps identical-input class needs the synced form"
    R, S, si, task = pt.R, pt.S, pt.si, pt.task
    if eta0 is not None and task == orc.TASK_REG:
        for rep, e in zip(pt.replicas, np.asarray(eta0, dtype=np.float64)):
            if np.isfinite(e):                               # both sides start from the same (w0, eta0): likelihood / prior in float64 from it
                rep.set_state(rep.w, e)
                rep.tau_pro = float(np.exp(e))
    if row_rtol is None:
        row_rtol = RTOL if sync else 2e-4
    if row_atol is None:
        row_atol = 2e-5 if sync else 2e-4
    sync_w = np.ascontiguousarray(tr["pos_w"], dtype=np.float32) if sync else None
    sync_eta = None
    if sync and task == orc.TASK_REG and getattr(s, "eta_trace", None) is not None:
        sync_eta = np.ascontiguousarray(s.eta_trace(), dtype=np.float32)       # [R, S]: eta of the state recorded in row i
    acc = tr["accept"].astype(np.int64)
    dec = np.empty((R, S - 1), dtype=np.int8)
    dec[:, :S - 2] = acc[:, 2:] - acc[:, 1:S - 1]
    dec[:, S - 2] = np.asarray(s.state()["num_accepted"], dtype=np.int64) - acc[:, S - 1]
    assert set(np.unique(dec).tolist()) <= {0, 1}, "accept counters of the device are not a step function"
    lag = s.log_alpha().astype(np.float64)
    log = s.swap_log()
    la, lu, sc = (np.empty((R, S - 1)) for _ in range(3))
    la_id, sc_id, lik_id = (np.full((R, S - 1), np.nan) for _ in range(3))   # accepted steps re-evaluated at the device's own proposal
    stale, nat = (np.empty((R, S - 1), dtype=np.int8) for _ in range(2))
    recs = None
    if ident_all:                                            # what the evaluation of a step at a rebuilt proposal needs (orc_step_rec)
        recs = dict(w_before=np.empty((R, S - 1, pt.P), dtype=np.float32), lg=np.empty((R, S - 1), dtype=np.int8),
                    **{k_: np.empty((R, S - 1)) for k_ in ("eta_before", "lik_cur", "prior_cur", "adapttemp")})
    forced_pairs, k, i0 = 0, 0, 0
    with ThreadPoolExecutor(threads) as ex:
        while i0 < S - 1:
            i1 = i0
            while i1 < S - 1 and not orc.swap_trigger(task, i1, si):
                i1 += 1
            handoff = i1 < S - 1
            i1 = i1 + 1 if handoff else S - 1

            def run(r, a=i0, b=i1):
                if not sync:
                    return pt.replicas[r].run(a, b, dec[r, a:b])
                return pt.replicas[r].run(a, b, dec[r, a:b], sync_w=sync_w[r, a + 1:b + 1],
                                          sync_eta=None if sync_eta is None else sync_eta[r, a + 1:b + 1], records=ident_all)
            for r, rec in enumerate(ex.map(run, range(R))):
                la[r, i0:i1], lu[r, i0:i1], sc[r, i0:i1] = rec["logalpha"], rec["logu"], rec["scale"]
                stale[r, i0:i1], nat[r, i0:i1] = rec["stale"], rec["natural"]
                if "la_sync" in rec:
                    la_id[r, i0:i1], sc_id[r, i0:i1], lik_id[r, i0:i1] = rec["la_sync"], rec["scale_sync"], rec["lik_sync"]
                if recs is not None:
                    for k_ in recs:
                        recs[k_][r, i0:i1] = rec[k_]
            pt._steps_done = i1
            if handoff:
                L = [rep.posted_L() for rep in pt.replicas]
                forced_pairs += follow_cascade(L, pt.tape.swap_uniforms(k, R - 1), log[k], f"{label}swap round {k} ", strict=not study)
                pt.swap_round(L=L, force_src=[int(v) for v in log[k]])
                k += 1
            i0 = i1
    if int(S / si) > pt.rounds_done:                          # Q13 phantom round: counted, result discarded
        L = [rep.likelihood for rep in pt.replicas]
        forced_pairs += follow_cascade(L, pt.tape.swap_uniforms(k, R - 1), log[k], f"{label}phantom round ", strict=not study)
        pt.swap_round(L=L, apply=False, force_src=[int(v) for v in log[k]])
    nsw, tot, rounds = s.swap_stats()
    assert (nsw, tot, rounds) == (pt.num_swap, pt.total_swap_proposals, pt.rounds_done), (nsw, tot, rounds, pt.num_swap, pt.total_swap_proposals)
    # ---- every step's log alpha
    rel = np.full(la.shape, LOGALPHA_REL_SYNCED[task] if sync else LOGALPHA_REL_FOLLOWED)
    ok = np.isfinite(la) & np.isfinite(lag)
    err = np.abs(lag - la)
    ratio = np.where(ok, err / np.maximum(sc, 1e-300), 0.0)
    over = ok & (err > rel * sc + LOGALPHA_ABS)
    report = dict(steps=int(R * (S - 1)), forced_mh=int((nat != dec).sum()), forced_swap_pairs=int(forced_pairs),
                  swap_pairs=int(pt.total_swap_proposals), accepted=int(dec.sum()),
                  max_ratio_fresh=float(ratio[stale == 0].max()), max_ratio_stale=float(ratio[stale != 0].max()) if (stale != 0).any() else 0.0,
                  max_abs_err=float(err[ok].max()), steps_over_bound=int(over.sum()), synced=bool(sync), eta_synced=sync_eta is not None,
                  max_abs_err_fresh=float(err[ok & (stale == 0)].max()),
                  max_abs_err_stale=float(err[ok & (stale != 0)].max()) if (ok & (stale != 0)).any() else 0.0,
                  median_scale=float(np.median(sc[ok])), steps_over_1e3=int((ok & (err > 1e-3)).sum()))
    if sync:
        # ---- identical inputs: every ACCEPTED step re-evaluated by the oracle at the device's own recorded proposal (w', eta') from
        # the common state -- what differs is the arithmetic of one evaluation, so this is where a per-step defect of a kernel
        # would show (a 1e-6-relative error of a likelihood sum is 5 x the bound), undiluted by where the proposal lies
        okid = np.isfinite(la_id) & np.isfinite(lag)
        err_id = np.abs(lag - la_id)
        lim_id = LOGALPHA_REL_IDENT * sc_id + LOGALPHA_ABS
        lk_dev = np.asarray(tr["likeh"], dtype=np.float64)[:, 1:]
        oklk = np.isfinite(lik_id) & np.isfinite(lk_dev)
        err_lk = np.abs(lk_dev - lik_id)
        lim_lk = LIK_REL_IDENT * (np.abs(lik_id) + pt.train.shape[0]) + LIK_ABS_IDENT
        report.update(ident_steps=int(okid.sum()),
                      ident_max_ratio=float((err_id[okid] / np.maximum(sc_id[okid], 1e-300)).max()) if okid.any() else 0.0,
                      ident_max_abs_err=float(err_id[okid].max()) if okid.any() else 0.0,
                      ident_over_bound=int((okid & (err_id > lim_id)).sum()), ident_over_1e3=int((okid & (err_id > 1e-3)).sum()),
                      ident_lik_max_abs_err=float(err_lk[oklk].max()) if oklk.any() else 0.0,
                      ident_lik_max_rel=float((err_lk[oklk] / np.maximum(np.abs(lik_id[oklk]), 1e-300)).max()) if oklk.any() else 0.0,
                      ident_lik_over_bound=int((oklk & (err_lk > lim_lk)).sum()))
    probing = bool(os.environ.get("PTNN_PARITY_PROBE")) or study
    if ident_all:
        # ---- identical inputs on EVERY step: the oracle evaluated at the device's own proposal, rebuilt bit for bit
        eta_rows = sync_eta if sync_eta is not None else np.zeros((R, S), dtype=np.float32)
        w_prop, eta_pro, noise, chk = rebuild_device_proposals(s, pt, recs, dec, sync_w, eta_rows, label, strict=not probing)
        la_all, sc_all, lik_all = ident_all_eval(pt, recs, w_prop, eta_pro, noise, threads=threads)
        report.update(chk)
        report.update(ident_all_check(lag, np.asarray(tr["likeh"], dtype=np.float64)[:, 1:], la_all, sc_all, lik_all, dec, stale,
                                      recs["lg"], pt.train.shape[0], label, strict=not probing))
        if arrays is not None:
            arrays.update(logalpha_ident_all=la_all, scale_ident_all=sc_all, lik_ident_all=lik_all, langevin=recs["lg"], w_prop=w_prop,
                          w_before=recs["w_before"], adapttemp=recs["adapttemp"])
    if arrays is not None:
        arrays.update(err=np.where(ok, err, np.nan), scale=sc, stale=stale, decided=dec, natural=nat, logalpha_oracle=la, logu=lu)
        if sync:
            arrays.update(err_ident=np.where(okid, err_id, np.nan), scale_ident=sc_id, err_lik_ident=np.where(oklk, err_lk, np.nan), lik_ident=lik_id)
    if os.environ.get("PTNN_PARITY_PROBE"):
        import json
        with open(os.environ["PTNN_PARITY_PROBE"], "a") as f:
            f.write(json.dumps(dict(label=label + "follow", test=os.environ.get("PYTEST_CURRENT_TEST", ""), **report)) + "\n")
    if not probing:
        if sync:
            assert report["ident_over_bound"] == 0, (f"{label}log alpha re-evaluated at the device's own proposal: {report['ident_over_bound']} of "
                                                     f"{report['ident_steps']} accepted steps outside the bound, worst {report['ident_max_ratio']:.3g} of the scale")
            assert report["ident_lik_over_bound"] == 0, (f"{label}log-likelihood at the device's own proposal: {report['ident_lik_over_bound']} accepted "
                                                         f"steps outside the bound, worst relative error {report['ident_lik_max_rel']:.3g}")
        assert not over.any(), (f"{label}log alpha outside the fp32 bound on {int(over.sum())} of {report['steps']} steps; worst "
                                f"{float(ratio.max()):.3g} of the scale at (replica, step) {np.unravel_index(int(np.argmax(np.where(over, ratio, 0))), ratio.shape)}")
    # ---- every decision taken differently is a coin flip inside the bound
    outside = 0
    for r, i in zip(*np.nonzero(nat != dec)):
        try:
            check_divergence(la[r, i], lu[r, i], sc[r, i], lag[r, i], f"{label}r{r} step {i}: ", rel=float(rel[r, i]))
        except AssertionError:
            if not study:
                raise
            outside += 1
    report["flips_outside_bound"] = outside
    # ---- every trace row of the run

    def rows_close(got, want, rtol, atol, what):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        both_nan = np.isnan(got) & np.isnan(want)
        excess = np.where(both_nan, 0.0, np.abs(got - want) - rtol * np.abs(want))
        worst = float(np.nanmax(excess)) if excess.size else 0.0
        report[what] = max(report.get(what, 0.0), worst)
        if not probing:
            assert not np.isnan(excess).any() and worst <= atol, f"{label}{what}: off by {worst:.3g} beyond rtol {rtol} (atol {atol})"
    likeh_atol = max(5e-3, float(np.nanmax(np.where(ok, rel * sc, 0.0)))) if sync else 0.1
    for r, rep in enumerate(pt.replicas):
        rows_close(tr["pos_w"][r], rep.pos_w, row_rtol, row_atol, "pos_w_abs_excess")
        # likeh of step i = the tempered log-likelihood of ITS proposal: for a synced run the all-steps class of bound (the accepted
        # steps are held to the identical-input bound above); unsynced: 0.034 measured on |likeh| ~ 10^3
        rows_close(tr["likeh"][r], rep.likeh[:, 0], 5e-5 if sync else row_rtol, likeh_atol if sync else 0.1, "likeh_abs_excess")
        if task == orc.TASK_REG:
            for nm in ("rmse_train", "rmse_test"):
                rows_close(tr[nm][r], getattr(rep, nm), 1e-4 if sync else 5e-4, 1e-6 if sync else 2e-6, "rmse_abs_excess")
        else:
            # classification scores count data rows: where two outputs of a row agree to fp32 round-off its predicted class may
            # differ from the float64 one (measured: at most 2 rows of Ionosphere's 109 test rows on any recorded step): every
            # recorded accuracy within 3 data rows, the class-id RMSE with what 3 rows can move it
            for nm in ("acc_train", "acc_test", "rmse_train", "rmse_test"):
                n_rows = (pt.train if nm.endswith("train") else pt.test).shape[0]
                rows_close(tr[nm][r], getattr(rep, nm), 0.0, (300.0 / n_rows + 1e-3) if nm.startswith("acc") else 0.08, nm[:4] + "_abs_excess")
    if os.environ.get("PTNN_PARITY_PROBE"):
        import json
        with open(os.environ["PTNN_PARITY_PROBE"], "a") as f:
            f.write(json.dumps(dict(label=label + "follow rows", **report)) + "\n")
    return report


# ---- the identical-input class on EVERY step (follow_device_run(ident_all=True)) --------------------------------------------
def step_class(dec, stale, lg):
    """Name of a step's class: accepted / rejected, fresh / stale cached likelihood, Langevin / random-walk proposal."""
    return ("acc" if dec else "rej") + ("_stale" if stale else "_fresh") + ("_lg" if lg else "_rw")


def device_startup_eta(s, w0, temperatures):
    """Regression: the eta = log var(residuals) every chain starts from is formed by the device in float32 at the head of its first
    launch and is not handed out by the library.  One MH step is run and the chains are restarted: a chain that rejected it still
    holds its start-up eta (exactly), a chain that accepted it has NaN here -- its step 0 is an accepted step, whose eta' the trace
    records.  -> float64 [R]."""
    s.set_state(w0, temperatures)
    s.run(1)
    s.sync()
    st = s.state()
    eta0 = np.where(st["num_accepted"] == 0, st["eta"].astype(np.float64), np.nan)
    s.set_state(w0, temperatures)
    return eta0


def rebuild_device_proposals(s, pt, recs, dec, pos_w, eta_rows, label="", strict=True):
    """The device's own proposal of EVERY step of a synced follow, bit for bit.  Every schedule forms w' = fmaf(step_w, noise, base)
    and eta' = fmaf(step_eta, n_eta, eta) with base = the state, or its SGD epoch on a Langevin step; the library hands out its
    own normals and scalars for any (replica, step) (ptnn_tape) and its own epoch (ptnn_langevin_gradient: ONE batched call over
    the distinct base states), and in a synced follow the oracle's state IS the device's float32 state (recs["w_before"],
    recs["eta_before"]).  fmaf is C's (oracle: orc_fmaf): a float64 multiply-add rounded to float32 rounds twice.

    Self-check, asserted (a mistake here would otherwise hide inside the tolerance): on every ACCEPTED step the rebuilt w' equals
    the recorded pos_w row and the rebuilt eta' the recorded eta bit for bit; the Langevin coin of the tape is the oracle's.
    (Every schedule's in-kernel epoch -- the packed PROP sweep, the wide deciding epoch, the 4-H-1 row loop -- produces the bits of
    ptnn_langevin_gradient: measured, 0 mismatches, so no schedule is exempt.)  A step whose starting eta is the
    oracle's float64 start-up value (device_startup_eta could not tell the device's) must be an accepted one; its eta' is taken
    from the trace.  -> (w_prop f32 [R, S-1, P], eta_pro f32 [R, S-1], noise f32 [R, S-1, P], report)."""
    import ptnn_oracle_c as orc_c
    R, n, P = recs["w_before"].shape
    c = pt.replicas[0].c
    noise, scal = np.empty((R, n, P), dtype=np.float32), np.empty((R, n, 3), dtype=np.float32)
    for r in range(R):
        for i in range(n):
            noise[r, i], scal[r, i] = s.tape(r, i)
    lg = recs["lg"] != 0
    coin = (scal[:, :, 0] < np.float32(c.l_prob)) & bool(c.use_lg)
    assert np.array_equal(coin, lg), f"{label}Langevin coin of the device's tape differs from the oracle's on {int((coin != lg).sum())} steps"
    base = recs["w_before"].copy()
    if lg.any():
        uniq, inv = np.unique(recs["w_before"][lg], axis=0, return_inverse=True)
        base[lg] = s.langevin_gradient(uniq)[np.asarray(inv).reshape(-1)]
    w_prop = orc_c.fmaf(c.step_w, noise, base)
    eta_pro = np.zeros((R, n), dtype=np.float32)
    unknown = np.zeros((R, n), dtype=bool)
    if pt.task == orc.TASK_REG:
        eta32 = recs["eta_before"].astype(np.float32)
        unknown = eta32.astype(np.float64) != recs["eta_before"]          # not a float32 number: the oracle's own start-up eta
        eta_pro = orc_c.fmaf(c.step_eta, scal[:, :, 2], eta32)
    acc = dec != 0
    rec_eta = np.asarray(eta_rows[:, 1:], dtype=np.float32)
    bad_w = acc & (w_prop.view(np.uint32) != np.ascontiguousarray(pos_w[:, 1:, :P]).view(np.uint32)).any(axis=2)
    bad_eta = acc & ~unknown & (eta_pro.view(np.uint32) != np.ascontiguousarray(rec_eta).view(np.uint32)) & (pt.task == orc.TASK_REG)
    eta_pro = np.where(unknown & acc, rec_eta, eta_pro)
    rep = dict(rebuild_accepted=int(acc.sum()), rebuild_w_mismatch_rw=int((bad_w & ~lg).sum()), rebuild_w_mismatch_lg=int((bad_w & lg).sum()),
               rebuild_eta_mismatch=int(bad_eta.sum()), rebuild_eta_from_trace=int((unknown & acc).sum()),
               rebuild_eta_unknown_rejected=int((unknown & ~acc).sum()))
    if strict:
        assert rep["rebuild_eta_unknown_rejected"] == 0, f"{label}{rep['rebuild_eta_unknown_rejected']} rejected steps start from an eta the device never recorded"
        assert rep["rebuild_w_mismatch_rw"] == 0 and rep["rebuild_w_mismatch_lg"] == 0 and rep["rebuild_eta_mismatch"] == 0, \
            f"{label}rebuilt proposals differ from the recorded accepted rows: {rep}"
    return w_prop, eta_pro, noise, rep


def ident_all_eval(pt, recs, w_prop, eta_pro, noise, keep=None, threads=8):
    """The oracle evaluated at the given proposal of every step (oracle/ptnn_oracle_c.c: orc_replica_eval_at) from the step's own
    records: -> float64 log alpha, scale, likeh entry, each [R, S-1] (keep: a mask of the steps wanted, NaN elsewhere)."""
    from concurrent.futures import ThreadPoolExecutor
    R, n, _ = recs["w_before"].shape
    out = np.full((3, R, n), np.nan)

    def one(r):
        rep = pt.replicas[r]                                 # supplies the problem and scratch; one thread per chain object
        for i in range(n):
            if keep is None or keep[r, i]:
                out[:, r, i] = rep.eval_at(recs["w_before"][r, i], w_prop[r, i], eta_pro[r, i], recs["lik_cur"][r, i], recs["prior_cur"][r, i],
                                           recs["adapttemp"][r, i], noise[r, i] if recs["lg"][r, i] else None)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(R)))
    return out[0], out[1], out[2]


def ident_all_check(la_dev, lik_dev, la_id, sc_id, lik_id, dec, stale, lg, n_train, label="", strict=True):
    """Every step's recorded log alpha and likeh against the oracle at identical inputs: LOGALPHA_REL_IDENT_ALL (by kind of
    proposal) of the scale + LOGALPHA_ABS, LIK_REL_IDENT_ALL of (|lik| + Ntr) + LIK_ABS_IDENT.  -> report with the maxima by class of step
    (step_class); strict: assert that no step is outside."""
    la_dev, lik_dev = np.asarray(la_dev, dtype=np.float64), np.asarray(lik_dev, dtype=np.float64)
    ok = np.isfinite(la_id) & np.isfinite(la_dev) & np.isfinite(lik_id) & np.isfinite(lik_dev)
    err = np.abs(la_dev - la_id)
    ratio = np.where(ok, err / np.maximum(sc_id, 1e-300), 0.0)
    rel = np.where(np.asarray(lg) != 0, LOGALPHA_REL_IDENT_ALL[1], LOGALPHA_REL_IDENT_ALL[0])
    over = ok & (err > rel * sc_id + LOGALPHA_ABS)
    err_lk = np.abs(lik_dev - lik_id)
    ratio_lk = np.where(ok, err_lk / (np.abs(lik_id) + n_train), 0.0)
    over_lk = ok & (err_lk > LIK_REL_IDENT_ALL * (np.abs(lik_id) + n_train) + LIK_ABS_IDENT)
    by = {}
    for d in (1, 0):
        for st in (0, 1):
            for l_ in (0, 1):
                m = ok & ((dec != 0) == bool(d)) & ((stale != 0) == bool(st)) & ((lg != 0) == bool(l_))
                if m.any():
                    by[step_class(d, st, l_)] = dict(steps=int(m.sum()), max_ratio=float(ratio[m].max()), over_bound=int((over & m).sum()),
                                                     lik_max_ratio=float(ratio_lk[m].max()), lik_max_abs_err=float(err_lk[m].max()),
                                                     lik_over_bound=int((over_lk & m).sum()))
    rep = dict(ident_all_steps=int(ok.sum()), ident_all_max_ratio=float(ratio.max()), ident_all_over_bound=int(over.sum()),
               ident_all_over_1e3=int((ok & (err > 1e-3)).sum()), ident_all_max_abs_err=float(err[ok].max()) if ok.any() else 0.0,
               ident_all_lik_max_ratio=float(ratio_lk.max()), ident_all_lik_over_bound=int(over_lk.sum()), ident_all_by_class=by)
    if strict:
        worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        assert rep["ident_all_over_bound"] == 0, (f"{label}log alpha at the device's own proposal, all steps: {rep['ident_all_over_bound']} of {rep['ident_all_steps']} "
                                                  f"outside the bound, worst {rep['ident_all_max_ratio']:.3g} of the scale at (replica, step) {worst}: {by}")
        assert rep["ident_all_lik_over_bound"] == 0, (f"{label}likeh at the device's own proposal, all steps: {rep['ident_all_lik_over_bound']} outside the bound, "
                                                      f"worst {rep['ident_all_lik_max_ratio']:.3g} of |lik| + Ntr: {by}")
    return rep


def oracle_alone_run(pt):
    """The C oracle run ALONE as if it were a device (no GPU): after every accepted step its state is replaced by its float32
    rounding (likelihood / prior re-evaluated there), as a synced follow imposes a device's, and the ladder swaps by its own
    cascade.  -> per-step arrays [R, S-1, ...]: its own log alpha, scale, likeh, decisions, classes, the records of
    follow_device_run(ident_all=True) and its own float64 proposals."""
    R, S, P = pt.R, pt.S, pt.P
    out = dict(w_before=np.empty((R, S - 1, P), dtype=np.float32), w_prop=np.empty((R, S - 1, P)), noise=np.empty((R, S - 1, P)),
               **{k: np.empty((R, S - 1), dtype=np.int8) for k in ("lg", "stale", "dec")},
               **{k: np.empty((R, S - 1)) for k in ("eta_before", "lik_cur", "prior_cur", "adapttemp", "eta_pro", "logalpha", "scale", "likeh")})
    import ptnn_oracle_c as orc_c
    for rep in pt.replicas:
        rep.set_state(rep.w.astype(np.float32), np.float32(rep.eta) if pt.task == orc.TASK_REG else None)
    for i in range(S - 1):
        for r, rep in enumerate(pt.replicas):
            rec = rep.run(i, i + 1, records=True)
            for k in ("w_before", "w_prop", "lg", "stale", "eta_before", "lik_cur", "prior_cur", "adapttemp", "eta_pro", "logalpha", "scale"):
                out[k][r, i] = rec[k][0]
            out["dec"][r, i] = rec["natural"][0]
            out["likeh"][r, i] = rep.likeh[i + 1, 0]
            out["noise"][r, i] = orc_c.w_noise(pt.tape.seed, rep.noise_gid, i, P)
            if rec["natural"][0]:
                rep.set_state(rep.w.astype(np.float32), np.float32(rep.eta) if pt.task == orc.TASK_REG else None)
                if pt.task == orc.TASK_REG:
                    rep.tau_pro = float(np.exp(rep.eta))
        pt._steps_done = i + 1
        if orc.swap_trigger(pt.task, i, pt.si):
            pt.swap_round()
    return out


# The cases of tests/test_gpu_follow_ident.py (and, run by the oracle alone, of tests/test_follow_ident_cpu.py): four chains, S across
# the 0.6 S temperature switch, a swap interval below S / 4 so that several rounds and stale steps occur, R (S - 1) <= 1500 (one
# ptnn_tape launch per step).  The seeds were picked by running the oracle alone (oracle_alone_run): every log alpha finite and at
# least one rejected fresh, one rejected stale and -- with Langevin proposals -- one rejected and one ACCEPTED Langevin step (the
# bit-for-bit self-check of the rebuilt Langevin proposals needs accepted ones; on Sunspot few seeds accept any within 300 steps).
# name: task, topology, data set, Langevin, lr, maxtemp, S, swap interval, seed, sampler options, what describe() must say
IDENT_CASES = {
    "cooperative": (0, (4, 5, 1), "sunspot", True, 0.1, 2, 300, 40, 8, dict(schedule=1), dict(schedule="cooperative")),
    "speculative": (0, (4, 5, 1), "sunspot", True, 0.1, 2, 300, 40, 5, dict(schedule=2), dict(schedule="speculative")),
    "packed": (0, (4, 5, 1), "sunspot", True, 0.1, 2, 300, 40, 23, dict(schedule=3), dict(schedule="packed-speculative", kernel="segment_pack_kernel")),
    "packed_shared_noise": (0, (4, 5, 1), "sunspot", True, 0.1, 2, 300, 40, 29, dict(schedule=3, shared_noise=1),
                            dict(schedule="packed-speculative", kernel="segment_pack_kernel")),
    "packed_several_cus": (0, (4, 10, 1), "mackey", True, 0.1, 2, 300, 40, 25, dict(), dict(schedule="packed-speculative", kernel="segment_packm_kernel")),
    "literal_5_inputs": (0, (5, 5, 1), "sunspot5", True, 0.1, 2, 300, 40, 6, dict(schedule=3), dict(schedule="packed-speculative")),
    "tree": (1, (4, 12, 3), "iris", False, 0.01, 10, 300, 40, 27, dict(schedule=4), dict(schedule="prefetching-tree")),
    "classification_langevin": (1, (4, 12, 3), "iris", True, 0.01, 10, 200, 30, 21, dict(schedule=2), dict(schedule="speculative")),
    "mfma_forward": (1, (34, 50, 2), "ions", False, 0.01, 10, 100, 15, 29, dict(schedule=1), dict(schedule="cooperative")),
    "wide": (0, (32, 96, 1), "synth32", True, 0.1, 2, 60, 9, 30, dict(), dict(schedule="-wide")),
    # 96 % 32 == 0 puts the net above on the LDS-resident kernel too; 70 hidden units run the wide kernel that streams its state
    "wide_streaming": (0, (32, 70, 1), "synth32", True, 0.1, 2, 60, 9, 32, dict(), dict(schedule="-wide", kernel="segment_wide_kernel", lds_resident_state=0)),
    "wide_resident": (0, (32, 128, 1), "synthetic256", True, 0.1, 2, 40, 6, 31, dict(), dict(schedule="-wide", lds_resident_state=1)),
}
IDENT_R = 4


def ident_case(name, seed=None):
    """-> (PTOracle on C chains started from float32 weights, w0 float32 [R, P], train, test) of one IDENT_CASES entry; both sides
    read float32 data.  seed: another than the entry's (the runs the bound was measured on)."""
    import ptnn_oracle_c as orc_c
    task, topo, dname, lg, lr, maxtemp, S, si, seed0, kw, _ = IDENT_CASES[name]
    seed = seed0 if seed is None else seed
    if dname == "synthetic256":
        train, test = synthetic_regression(320, 256, topo[0], topo[1], seed=5)
    else:
        d = datasets()
        train, test = d[dname + "_train"], d[dname + "_test"]
    train, test = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (train, test))
    pt = orc.PTOracle(task, topo, train, test, IDENT_R, maxtemp, IDENT_R * S, si, use_lg=lg, l_prob=0.5, lr=lr, seed=seed,
                      shared_noise=bool(kw.get("shared_noise", 0)))
    w0 = np.stack([rep.w for rep in pt.replicas])
    if topo[1] > 64:
        w0 = 0.3 * w0                                        # bench.py's scale for wide nets
    w0 = np.asarray(w0, dtype=np.float32)
    orc_c.adopt(pt, w0=w0.astype(np.float64))
    return pt, w0, train, test


def run_smoke_check():
    """Sunspot, FNN 4-5-1, 4 replicas, Langevin p=0.5, S=60, swaps every 10: HIP vs oracle on the same tape."""
    ds = datasets()
    train, test = ds["sunspot_train"], ds["sunspot_test"]
    topo, R, S, si, seed = (4, 5, 1), 4, 60, 10, 77
    pt = orc.PTOracle(orc.TASK_REG, topo, train, test, R, 2, R * S, si, use_lg=True, l_prob=0.5, lr=0.1, seed=seed)
    w0 = np.stack([rep.w for rep in pt.replicas]).astype(np.float32)
    for rep, w in zip(pt.replicas, w0):                     # both sides start from the same fp32-representable weights
        rep.__init__(orc.TASK_REG, topo, pt.train, pt.test, w.astype(np.float64), rep.T, S, True, 0.5, 0.1, pt.tape, rep.gid)
    o = OracleRun(pt).run()
    s = make_sampler(orc.TASK_REG, topo, train, test, R_local=R, R_global=R, first=0, S=S, si=si, use_lg=True, lr=0.1,
                     seed=seed)
    s.set_state(w0, np.array(pt.temperatures, dtype=np.float32))
    s.run(-1)
    s.sync()
    tr = s.traces()
    firsts = check_run_against_oracle(s, tr, o, "smoke ")
    nsw, tot, rounds = s.swap_stats()
    assert tot == pt.total_swap_proposals and rounds == pt.rounds_done, (tot, rounds)
    s.close()
    return firsts


def synthetic_regression(n_rows, n_train, n_in, n_hidden, seed):
    """SURVEY.md 8(d) config-5 recipe (same as tests/golden/make_fixtures.py): X ~ U(0,1), teacher FNN run through the
    reference forward rule, y = clip(teacher + N(0, 0.02^2), 0, 1)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n_rows, n_in))
    topo = (n_in, n_hidden, 1)
    w_t = np.concatenate([rng.standard_normal(n_in * n_hidden) / np.sqrt(n_in), rng.standard_normal(n_hidden) / np.sqrt(n_hidden),
                          rng.standard_normal(n_hidden) / np.sqrt(n_in), rng.standard_normal(1) / np.sqrt(n_hidden)])
    y = np.clip(orc.forward(X, w_t, topo)[1][:, 0] + rng.normal(0, 0.02, n_rows), 0, 1)
    data = np.hstack([X, y[:, None]])
    return data[:n_train], data[n_train:]


def posterior_parity(ref_runs, dev_runs, task, var_ratio_hi=1.25):
    """Statistical parity of whole runs.  ref_runs: the reference's own runs from one start (fixture); dev_runs:
    device runs from the same start; each a dict with w_mean / w_var [R, P] after burn-in, accept_pct [R], swap_perc, rmse / acc
    means.  MCSE of a difference of means = sqrt(s_ref^2 / K_ref + s_dev^2 / K_dev) from the seed-to-seed spread on each side.

      posterior mean   |mean_dev - mean_ref| <= 0.1 sd_post + 3 MCSE per weight and chain, sd_post^2 = the within-chain
                       posterior variance (mean over both sides' runs).  The chains are short and far from mixed, so s_ref from
                       five runs is itself noisy (t with 4 degrees of freedom: 4 % of exact draws exceed 3 MCSE): at least 90 %
                       of the (chain, weight) pairs must be inside, and the median |z| must be below 1 (a shifted posterior
                       moves every pair, not a tail of them).
      posterior var    per chain, ratio of the geometric means (over the chain's weights, mean over runs of log var) in
                       [0.8, var_ratio_hi] widened by 3 MCSE of that log ratio (seed-to-seed spread of the per-run chain
                       values).  var_ratio_hi = 1.25 is SURVEY 8d's bound and holds under shared_noise = 1 (the reference's
                       behaviour and the drop-in's default); independent noise streams are held to 2.0 (see the test).
      MH acceptance    per temperature, |acc_dev - acc_ref| <= 3 points + 3 MCSE
      swap percentage  |swap_dev - swap_ref| <= 5 points + 3 MCSE
      RMSE, accuracy   |x_dev - x_ref| <= 3 MCSE + 5 % of the reference value
    """
    def arr(runs, k):
        return np.array([np.asarray(r[k], dtype=np.float64) for r in runs])

    def mcse(a, b):
        return np.sqrt(a.var(axis=0, ddof=1) / a.shape[0] + b.var(axis=0, ddof=1) / b.shape[0])
    rep = {}
    mr, md = arr(ref_runs, "w_mean"), arr(dev_runs, "w_mean")
    vr, vd = arr(ref_runs, "w_var"), arr(dev_runs, "w_var")
    sd_post = np.sqrt(0.5 * (vr.mean(axis=0) + vd.mean(axis=0)))
    diff = np.abs(md.mean(axis=0) - mr.mean(axis=0))
    se = mcse(mr, md)
    inside = diff <= 0.1 * sd_post + 3.0 * se
    z = diff / np.maximum(se, 1e-300)
    rep["mean_frac_inside"] = float(inside.mean())
    rep["mean_median_abs_z"] = float(np.median(z))
    ok = rep["mean_frac_inside"] >= 0.90 and rep["mean_median_abs_z"] < 1.0
    # variance ratio per chain, in the log domain: ratio of the geometric means over the chain's weights.  A chain that receives
    # a state from another mode through a swap multiplies the variance of ALL its weights at once, so the Monte Carlo error of
    # the ratio is taken from the seed-to-seed spread of the per-run chain values, not from the number of weights.
    # (a hot chain that accepts nothing after burn-in has variance 0 in that run: floored at (1e-6)^2, far below a single step)
    lr_, ld_ = np.log(np.maximum(vr, 1e-12)).mean(axis=2), np.log(np.maximum(vd, 1e-12)).mean(axis=2)       # [K, R]
    g = ld_.mean(axis=0) - lr_.mean(axis=0)
    gse = mcse(lr_, ld_)
    rep["var_ratio_per_chain"] = [float(v) for v in np.exp(g)]
    rep["var_ratio_mcse"] = [float(v) for v in gse]
    ok = ok and bool(np.all(g <= np.log(var_ratio_hi) + 3.0 * gse) and np.all(g >= -np.log(1.25) - 3.0 * gse))
    ar, ad = arr(ref_runs, "accept_pct"), arr(dev_runs, "accept_pct")
    dacc = np.abs(ad.mean(axis=0) - ar.mean(axis=0))
    rep["accept_pct_ref"] = [float(v) for v in ar.mean(axis=0)]
    rep["accept_pct_dev"] = [float(v) for v in ad.mean(axis=0)]
    ok = ok and bool(np.all(dacc <= 3.0 + 3.0 * mcse(ar, ad)))
    sr, sdv = arr(ref_runs, "swap_perc"), arr(dev_runs, "swap_perc")
    rep["swap_perc_ref"], rep["swap_perc_dev"] = float(sr.mean()), float(sdv.mean())
    ok = ok and abs(sdv.mean() - sr.mean()) <= 5.0 + 3.0 * float(mcse(sr, sdv))
    keys = ["rmse_train_mean", "rmse_test_mean"] + (["acc_train_mean", "acc_test_mean"] if task == orc.TASK_CLS else [])
    for k in keys:
        a, b = arr(ref_runs, k), arr(dev_runs, k)
        rep[k] = [float(a.mean()), float(b.mean())]
        ok = ok and abs(b.mean() - a.mean()) <= 3.0 * float(mcse(a, b)) + 0.05 * abs(a.mean())
    rep["ok"] = bool(ok)
    return rep
