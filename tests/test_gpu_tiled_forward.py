"""The matrix-core forward passes of the wide nets (64 < H <= 512, H % 32 == 0: wide_forward of csrc/ptnn_dev_wide.hpp) at every
compiled shape, through Sampler.evaluate (model_wide_kernel: one vector a work-group, no chain) against the float64 oracle:

  forward_bf16 = 0   the default: eval_rows_mfma_wsplit (three-term bf16 split operands) for 9, 11, 16, 20, 32 and 34 inputs, the
                     exact fp32 instruction for 4, 5 and 6 (SplitK<n_in> has no split for them)
  forward_bf16 = 2   eval_rows_mfma<..., false>: the exact fp32 instruction, k-steps of 2
  forward_bf16 = 1   eval_rows_mfma<..., true>: operands rounded to bf16, k-steps of 16

on the grid of tests/model_cases.py: the ten shapes x TILED = 96, 128, 160, 512 hidden units (3, 4, 5, 16 tiles on 2, 2, 3, 8 waves:
the odd and the even tail of the split pass' two-stage tile pipeline, more waves than row blocks) x the row sets of EVAL_SPLITS
(Nall = 2, 36, 65, 600: 1, 2, 3 and 19 blocks of 32 rows -- a partial block, the repeated last block of an odd count, uneven
work over the waves -- with Ntr = 31, 60, 420 inside a block).  The shapes bring odd n_in (the padding k = n_in of the upper lane
half), the zero-padded bf16 k-step (9, 11), the fp32 remainder columns behind the bf16 k-steps (20: two steps, 34: one) and one
and two bf16 k-steps.  Modes 0 and 2 are held to the oracle at the golden-vector tolerances (check_evaluation, class counts as
integers), mode 1 at the same tolerances to the oracle on bf16-rounded operands (bf16 x bf16 products are exact in fp32).
tests/test_model_cases_cpu.py proves from float64 alone that float32 restatements of the three passes stay inside these tolerances
on this grid and that a dropped input column, dropped remainder columns, a dropped hidden unit and a row scored twice do not.

None of the 40 (shape, H) is refused by ptnn_supports or by the LDS plan: no case is left out.

describe()["forward_mfma"] is 2 for the split pass and 1 -- not 0 -- for the other two matrix-core passes of a wide handle (0 is
the VALU pass of a width that does not tile): it tells the split pass and the matrix cores from the rest, and cannot tell the
exact pass from the bf16 one, which forward_bf16 decides alone (wide_forward).

The LDS-resident wide segment kernel (seg_wide_res) runs Langevin chains at every shape with 96 hidden units against the oracle,
and two work-groups a replica commit the chain of one bit for bit.
Measured on the MI355X: see DESIGN.md, "Every compiled shape: the epoch and the evaluation"."""
import numpy as np
import pytest

import model_cases as mc
import parity
from parity import orc
from test_gpu_model_shapes import check_evaluation, langevin_chains, sampler

pytestmark = pytest.mark.gpu

SHAPE_IDS = {s: f"t{s[0]}-{s[1]}-H-{s[2]}" for s in mc.SHAPES}
CASES = [(shape, mode) for shape in mc.SHAPES for mode in mc.TILED_MODES]
_LIK = {}       # (shape, mode, H) -> the log-likelihoods (train, test) of every cell: the split pass next to the exact one


@pytest.mark.parametrize("shape,mode", CASES, ids=[f"{SHAPE_IDS[s]}-fwd{m}" for s, m in CASES])
def test_tiled_forward_at_every_shape(shape, mode):
    """evaluate of the three vectors under forward_bf16 = mode at the four tiled hidden sizes and the four row sets, one sampler per
    H re-used through set_data: the pass is asserted from describe() first, then every figure is held to the oracle."""
    task, I, O = shape
    rows = mc.eval_data(shape)
    how = mc.tiled_pass(I, mode)
    reference = mc.evaluate_bf16 if mode == 1 else mc.evaluate
    for H in mc.TILED:
        topo = (I, H, O)
        ws = mc.tiled_weights(shape, H, bf16=mode == 1)
        s, liks, err = None, [], 0.0
        for ntr, nte in mc.EVAL_SPLITS:
            train, test = rows[:ntr], rows[ntr:ntr + nte]
            if s is None:
                s = sampler(shape, H, train, test, forward_bf16=mode)
            else:
                s.set_data(train, test)
            # the path, before anything is compared
            assert s.describe()["forward_mfma"] == (2 if how == "split" else 1), (topo, mode, s.describe())
            for tau in (mc.TAUS if task == orc.TASK_REG else (None,)):
                ev = s.evaluate(ws, tau)
                for k in range(3):
                    want = reference(task, topo, train, test, ws[k], tau)
                    liks.append((float(ev[k][0]), float(ev[k][6])))
                    err = max(err, abs(liks[-1][0] - want["lik"]), abs(liks[-1][1] - want["lik_test"]))
                    check_evaluation(ev[k], want, task, ntr, nte, f"{topo} forward_bf16={mode} Ntr={ntr} Nte={nte} tau={tau} w{k}")
        s.close()
        _LIK[shape, mode, H] = np.array(liks)
        other = _LIK.get((shape, 2 if mode == 0 else 0, H)) if mode != 1 else None
        apart = "n/a" if other is None else f"{np.abs(_LIK[shape, mode, H] - other).max():.3g}"
        print(f"MODEL_SHAPES tiled {SHAPE_IDS[shape]} forward_bf16={mode} ({how}) H={H}: max |lik - oracle| {err:.3g}, "
              f"max |lik(default) - lik(exact)| {apart}")


@pytest.mark.parametrize("shape", mc.SHAPES, ids=list(SHAPE_IDS.values()))
def test_resident_wide_segment_kernel_at_every_shape(shape):
    """seg_wide_res, the kernel of every wide net with H % 32 == 0 whose state fits LDS beside the proposal, at 96 hidden units:
    four replicas, 26 samples, swaps every 6, Langevin proposals with probability 0.5 at lr 0.01 on 60 + 20 rows, the schedule left
    to the library, against PTOracle on the same tape; and with two work-groups a replica (speculation over work-groups) traces,
    swap statistics, swap log and state are those of one work-group, bit for bit."""
    task, I, O = shape
    topo = (I, 96, O)
    d = mc.data(task, I, O, 80, 800000 + 1000 * I + O)
    runs = {}
    for groups in (1, 2):
        runs[groups] = {}
        what = langevin_chains(topo, d[:60], d[60:], 0, f"{topo} groups={groups} ", task=task, groups=groups, committed=runs[groups])
        assert what["lds_resident_state"] == 1 and what["groups_per_replica"] == groups, what
        assert what["forward_mfma"] == (2 if mc.split_k(I)[2] else 1), what
    one, two = runs[1], runs[2]
    assert one["swap_stats"] == two["swap_stats"] and np.array_equal(one["swap_log"], two["swap_log"])
    for k in one["traces"]:
        assert np.array_equal(one["traces"][k], two["traces"][k], equal_nan=True), k
    for k in one["state"]:
        assert np.array_equal(one["state"][k], two["state"][k], equal_nan=True), k
