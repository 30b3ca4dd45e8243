"""The grid of tests/model_cases.py judged from the float64 oracle alone (no GPU): what tests/test_gpu_model_shapes.py asserts on the
device can fail for a wrong kernel and cannot fail for a right one.

The epoch bound.  The device's SGD epoch is held to r <= R_BOUND = 0.1 in the unit r(v) = max_j |v_j - ref_j| / (2e-5 + 1e-4 |ref_j|),
i.e. rtol = 1e-5, atol = 2e-6.  It is 16 times what a float32 restatement of the reference's plain chain needs: measured here over
the whole grid (10 shapes x 12 hidden sizes x 8 row counts x 2 learning rates x 3 vectors) the restatement's worst r is 0.0057
(4-100-3, 31 rows), its median 0.0012, and the first test holds it to 0.1 / 16 = 0.00625.  The margin of 16 covers the hardware
exp2 / rcp (1 ulp each, two pairs per row) and the reordering of the deferred update, all O(eps) per row like the restatement's own
roundings.  Every structurally wrong epoch is at least 2 R_BOUND away from the right one in every cell of the same grid (measured
minima: last row's W1 / B1 update dropped 1.16 at lr 0.01 and 8.0 at lr 0.1; hidden unit H-1 never updated 3.1 / 31; input column
I-1 never updated 0.42 / 4.2; last class's B2 update of the last row undone 6.1 / 6.4), and the post-update-W2 epoch (quirk Q4 the
wrong way round) at 31 rows and lr 0.1 (minimum 1.41).  With fewer rows or the smaller rate that last one moves the weights by
less than float32 does: the device test cannot see it there, and does not claim to."""
import os
import re

import numpy as np
import pytest

import model_cases as mc
import ptnn_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN = mc.NARROW + mc.WIDE

_GRID = None


def grid():
    """{(shape, H, Ntr): (ref [6, P], {variant: [6, P]})}: the float64 epochs of the three vectors at lr 0.1 (rows 0..2) and 0.01
    (rows 3..5), the float32 restatement and every wrong epoch, computed once."""
    global _GRID
    if _GRID is None:
        _GRID = {}
        lr6 = np.repeat(mc.LRS, 3)
        for shape in mc.SHAPES:
            task, I, O = shape
            train, _ = mc.epoch_data(shape)
            for H in HIDDEN:
                ws = mc.weights(shape, H)
                w6 = np.concatenate([ws, ws])
                for ntr in mc.NTRS:
                    args = (train[:ntr], w6, (I, H, O), lr6, task)
                    var = {"float32": mc.epoch(*args, dtype=np.float32)}
                    for m in mc.MUTANTS[:3 if O == 1 else 4]:
                        var[m] = mc.epoch(*args, mutant=m)
                    if ntr == 31:
                        var["post_w2"] = mc.epoch(*args, mutant="post_w2")
                    _GRID[shape, H, ntr] = (mc.epoch(*args), var)
    return _GRID


def cell_r(ref, v, j):
    """The largest r over the three vectors of learning rate LRS[j]."""
    return max(mc.r_unit(v[3 * j + k], ref[3 * j + k]) for k in range(3))


def test_grid_is_the_compiled_shapes_and_the_stated_bound():
    text = open(os.path.join(ROOT, "parallel-tempering-neural-net_amd", "csrc", "ptnn_shapes.hpp")).read()
    line = re.search(r"^#define PTNN_SHAPES\(X\)(.*)$", text, re.M).group(1)
    assert [tuple(map(int, m)) for m in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", line)] == mc.SHAPES
    assert len(HIDDEN) == 12 and max(mc.NARROW) == 64 and min(mc.WIDE) == 65
    assert mc.R_BOUND == pytest.approx(0.1) and mc.MUTANT_MIN == pytest.approx(0.2)
    # r <= 0.1 is rtol = 1e-5, atol = 2e-6
    assert mc.R_BOUND * mc.R_RTOL == pytest.approx(1e-5) and mc.R_BOUND * mc.R_ATOL == pytest.approx(2e-6)


def test_batched_epoch_is_the_oracles():
    """model_cases.epoch with no mutant is oracle.langevin_gradient, bit for bit, on a regression and a many-class cell."""
    for shape, H, ntr in (((0, 5, 1), 9, 7), ((1, 6, 18), 17, 5), ((1, 34, 2), 65, 3)):
        task, I, O = shape
        train, _ = mc.epoch_data(shape)
        ws = mc.weights(shape, H)
        got = mc.epoch(train[:ntr], ws, (I, H, O), 0.1, task)
        for k in range(3):
            assert np.array_equal(got[k], orc.langevin_gradient(train[:ntr], ws[k], (I, H, O), 0.1, task))


def test_float32_restatement_stays_a_sixteenth_of_the_bound():
    worst = max((cell_r(ref, var["float32"], j), key, mc.LRS[j]) for key, (ref, var) in grid().items() for j in range(2))
    assert worst[0] <= mc.F32_WORST, worst


@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_structural_mutants_are_twice_the_bound_away_in_every_cell(mutant):
    found = []
    for key, (ref, var) in grid().items():
        if mutant in var:
            for j in range(2):
                found.append((cell_r(ref, var[mutant], j), key, mc.LRS[j]))
    # every (shape, H, Ntr, lr); the B2 mutant exists where n_out > 1
    shapes = [s for s in mc.SHAPES if s[2] > 1] if mutant == "last_row_b2_last" else mc.SHAPES
    assert len(found) == len(shapes) * len(HIDDEN) * len(mc.NTRS) * len(mc.LRS)
    assert min(found)[0] >= mc.MUTANT_MIN, min(found)


def test_post_update_w2_is_seen_at_31_rows_and_the_larger_rate():
    """... and not promised anywhere else: over a short epoch or at lr 0.01 the two W2 differ by less than float32 rounds."""
    found = [(cell_r(ref, var["post_w2"], 0), key) for key, (ref, var) in grid().items() if "post_w2" in var]
    assert len(found) == len(mc.SHAPES) * len(HIDDEN)
    assert min(found)[0] >= mc.MUTANT_MIN, min(found)
    short = []
    for shape, H in (((0, 4, 1), 1), ((1, 6, 18), 64), ((1, 34, 2), 130)):
        task, I, O = shape
        args = (mc.epoch_data(shape)[0][:1], mc.weights(shape, H), (I, H, O), 0.01, task)
        short.append(cell_r(mc.epoch(*args), mc.epoch(*args, mutant="post_w2"), 0))
    assert min(short) < mc.R_BOUND          # the stated blind spot is real


def test_evaluation_grid_has_no_near_ties_and_no_saturated_output():
    """Accuracy and class RMSE can then be compared exactly: no row's argmax is a matter of rounding (two largest pre-activations at
    least 1e-4 apart: a float32 hidden sum is good to ~1e-6), and no output enters the quantised regimes of argmax_key (z >= 30)."""
    for shape in mc.SHAPES:
        rows = mc.eval_data(shape)
        assert rows.shape == (mc.EVAL_ROWS, shape[1] + 1) and max(a + b for a, b in mc.EVAL_SPLITS) == mc.EVAL_ROWS
        for H in HIDDEN:
            assert mc.tie_free(shape, H, mc.eval_weights(shape, H), rows), (shape, H)
            k = mc.SEED_MOVES.get((shape, H), 0)
            for lower in range(k):         # a moved seed is the first that gives this and a regression RMSE float32 can hold
                assert not mc.usable(shape, H, mc.weights(shape, H, seed=1000 * shape[1] + H + 100000 * lower), rows), (shape, H, lower)
        if shape[0] == orc.TASK_CLS:       # several classes occur in every row set: accuracy and class RMSE have something to tell apart
            for ntr, nte in mc.EVAL_SPLITS[1:]:
                assert len(np.unique(rows[:ntr, -1])) > 1 and len(np.unique(rows[ntr:ntr + nte, -1])) > 1, shape


def test_regression_rmse_is_within_reach_of_float32_in_every_row_set():
    """The device test holds the regression RMSE to rtol = 1e-5 in row sets down to a single row, where RMSE = |f - y| is a difference
    of two numbers of order 0.5: with the unmoved seeds one set (5-130-1, the test row of (1, 1), second vector) has |f - y| = 2.1e-4,
    and half a float32 ulp of f is 1.6e-4 of that.  Here, from float64 alone: a float32 forward is at most RMSE_ULPS = 8 ulp off at
    any output of the grid (the restatement's worst: 6.9), and in every row set of every (shape, H) outputs 8 ulp off, all to the
    worse side, move the RMSE by no more than 1e-5 of itself.  The restatement's own RMSE then meets the device's tolerance."""
    worst_ulp = 0.0
    for shape in [s for s in mc.SHAPES if s[0] == orc.TASK_REG]:
        _, I, O = shape
        rows = mc.eval_data(shape)
        for H in HIDDEN:
            ws = mc.eval_weights(shape, H)
            assert mc.rmse_conditioned(shape, H, ws, rows), (shape, H)
            for w in ws:
                f = orc.forward(rows[:, :I], w, (I, H, O))[1].ravel()
                f32 = mc.forward_f32(rows[:, :I], w, (I, H, O)).ravel()
                worst_ulp = max(worst_ulp, float(np.max(np.abs(f32 - f) / np.spacing(f.astype(np.float32)))))
                for ntr, nte in mc.EVAL_SPLITS:
                    for part in (slice(0, ntr), slice(ntr, ntr + nte)):
                        np.testing.assert_allclose(orc.rmse(f32[part].astype(np.float64), rows[part, I]), orc.rmse(f[part], rows[part, I]),
                                                   rtol=mc.RMSE_RTOL, err_msg=f"{shape} {H} {ntr} {nte}")
    assert worst_ulp <= mc.RMSE_ULPS, worst_ulp
    # the criterion is the cancellation it is named for: one row, prediction 0.5, 2.1e-4 from its target
    assert mc.rmse_ulp_sensitivity(np.array([0.5]), np.array([0.5 - 2.1e-4])) == pytest.approx(2.0 ** -24 / 2.1e-4)


def test_long_evaluation_cases_reach_every_row_blocking():
    """eval_rows takes a lane's rows in blocks of RB = 8 / 4 / 2 (n_in <= 7 / <= 15 / above), then 4, 2, 1.  The 600-row grid reaches
    two rows a lane on a narrow net; with the long cases every blocking of a shape runs in the wide family, and on a narrow net of up
    to 11 inputs on each forward image it has; the narrow nets' rows fit the LDS the runtime grants; and the long rows are as free
    of near ties, saturated outputs and ill-conditioned RMSEs as the 600."""
    for shape in mc.SHAPES:
        _, I, O = shape
        rows = mc.long_data(shape)
        rb = 8 if I <= 7 else 4 if I <= 15 else 2
        every = {b for b in (8, 4, 2, 1) if b <= rb}
        for family, hs in mc.FAMILIES.items():
            reached = {}
            for H in hs:
                reached[H] = set().union(*(mc.eval_blocks(I, H, a + b) for a, b in mc.EVAL_SPLITS))
            for H, splits in mc.long_cases(shape, family):
                assert H in hs and max(a + b for a, b in splits) <= mc.LONG_ROWS
                reached[H] |= set().union(*(mc.eval_blocks(I, H, a + b) for a, b in splits))
                if family == "narrow":
                    assert max(mc.model_lds_bytes(shape, H, a + b) for a, b in splits) <= 152 * 1024, (shape, H)
                n = max(a + b for a, b in splits)
                assert mc.usable(shape, H, mc.long_weights(shape, H), rows[:n], splits), (shape, H)
                for lower in range(mc.LONG_SEED_MOVES.get((shape, H), 0)):
                    assert not mc.usable(shape, H, mc.weights(shape, H, seed=mc.weight_seed(shape, H) + 100000 * lower), rows[:n], splits)
                if shape[0] == orc.TASK_CLS:
                    assert all(len(np.unique(rows[:a, -1])) > 1 and len(np.unique(rows[a:a + b, -1])) > 1 for a, b in splits)
            if family == "wide":
                assert set().union(*reached.values()) == every, (shape, reached)
            elif I <= 15:          # the unit-row image (odd H) and the pair image (even H >= 8; the only one from 8 inputs on)
                assert reached[16] == every and (I >= 8 or reached[9] == every), (shape, reached)
            else:                  # two rows a block: 600 rows on 512 threads, and one row a lane below that
                assert all(r == every for r in reached.values()), (shape, reached)
    assert mc.eval_blocks(4, 16, 600) == {2} and mc.eval_blocks(4, 100, 600) == {4, 1} and mc.eval_blocks(4, 64, 3600) == {8}
    assert mc.model_threads(64, 600) == 512 and mc.model_threads(16, 36) == 64 and mc.model_threads(130, 5) == 192


def test_inputs_are_float32_values():
    for shape in mc.SHAPES:
        for a in (*mc.epoch_data(shape), mc.eval_data(shape), mc.weights(shape, 17), mc.eval_weights(shape, 64)):
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("shape,H", mc.ARGMAX_SHAPES, ids=["4-3-3", "6-8-18"])
def test_argmax_regime_cases_are_what_they_claim(shape, H):
    """From float64 alone: the special classes sit in the stated regime on every row, well inside it, and np.argmax over the float64
    outputs picks the class the regime is named for -- which an ordering by the float32 output, or by z itself, would not."""
    task, I, O = shape
    topo = (I, H, O)
    for regime in mc.ARGMAX_REGIMES:
        train, test, w, spec = mc.argmax_case(shape, H, regime)
        rows = np.vstack([train, test])
        z = mc.pre_activations(rows, w, topo)
        with np.errstate(over="ignore"):
            out = orc.forward(rows[:, :I], w, topo)[1]
        for o, zo in spec.items():
            assert np.abs(z[:, o] - zo).max() <= 0.02, (regime, o)
        others = [o for o in range(O) if o not in spec]
        assert all(np.abs(z[:, o]).max() < 20 for o in others)
        arg = np.argmax(out, axis=1)
        if regime == "saturated_first_wins":
            assert (out[:, 1] == 1.0).all() and (out[:, 2] == 1.0).all() and (z[:, 2] > z[:, 1]).all() and (arg == 1).all()
        elif regime == "quantised_different":
            assert (out[:, 2] > out[:, 0]).all() and (arg == 2).all()
            assert (out[:, [0, 2]].astype(np.float32) == 1.0).all()                       # fp32 outputs would tie: class 0
            k = np.exp(-z[:, [0, 2]]) * 2.0 ** 52                                         # far from a rounding edge of rint
            assert (np.abs(k - np.rint(k)) < 0.25).all()
        elif regime == "quantised_equal":
            assert (out[:, 1] == out[:, 2]).all() and (z[:, 2] > z[:, 1] + 0.1).all() and (arg == 1).all()
            k = np.exp(-z[:, [1, 2]]) * 2.0 ** 52
            assert (np.rint(k) == 1).all() and (np.abs(k - 1) < 0.25).all()
        elif regime == "underflow_one":
            assert (out[:, 0] == 0.0).all() and (arg != 0).all() and (out[:, others] > 0).all()
        else:
            assert (out == 0.0).all() and (z.argmax(axis=1) == O - 1).all() and (arg == 0).all() and z.max() < -712
        # the labels tell the right class from the one a wrong ordering would pick, in both row sets
        wrong = {"saturated_first_wins": 2, "quantised_different": 0, "quantised_equal": 2, "underflow_all": O - 1}.get(regime)
        if wrong is not None:
            for part in (train, test):
                y = part[:, I]
                assert np.count_nonzero(y == arg[0]) != np.count_nonzero(y == wrong) or np.sum((y - arg[0]) ** 2) != np.sum((y - wrong) ** 2)


# ---- the tiled family: the matrix-core forward passes of the wide nets (tests/test_gpu_tiled_forward.py) -------------------------------
#
# From float64 alone, over the ten shapes x TILED x the four row sets x the three vectors (x two tau for regression): a float32
# restatement of each pass's summation -- exact fp32 and bf16 operands k ascending, the split pass in the kernel's order of its six
# products -- stays inside check_evaluation's tolerances (the golden-vector ones, class counts as integers), and the structurally
# wrong forwards fall outside them on at least one row set of every (shape, H): the last input column never multiplied, the fp32
# remainder columns never multiplied (20 and 34 inputs), the last hidden unit of the last tile left out, row Nall - 1 scored twice
# (the repeated block of an odd block count).  Measured here, largest |log-likelihood - float64| of the restatements over the grid
# in units of the tolerance 1e-3 + 2e-5 |lik|: exact 0.017, bf16 (against the oracle on rounded operands) 0.019, split 0.004.
# The split reduced to two terms (hi + mid) is measured and printed, not asserted: 0.077 at worst, refused in none of the 24
# (shape, H) that have a split pass -- these tolerances cannot see a 2^-16 relative error in a product.
from test_gpu_model_shapes import check_evaluation  # noqa: E402

_TILED = {}


def tiled_cell(shape, H):
    """(rows, {bf16: three vectors}, {bf16: {(split, tau, k): the oracle's figures}}, {pass: [(z, out) of each vector] float32})"""
    if (shape, H) not in _TILED:
        task, I, O = shape
        topo = (I, H, O)
        rows = mc.eval_data(shape)
        ws = {False: mc.tiled_weights(shape, H), True: mc.tiled_weights(shape, H, bf16=True)}
        want = {False: {}, True: {}}
        for bf, fn in ((False, mc.evaluate), (True, mc.evaluate_bf16)):
            for ntr, nte in mc.EVAL_SPLITS:
                for tau in taus(task):
                    for k in range(3):
                        want[bf][(ntr, nte), tau, k] = fn(task, topo, rows[:ntr], rows[ntr:ntr + nte], ws[bf][k], tau)
        passes = {}
        hows = ["exact", "bf16"] + (["split", "two_terms"] if mc.split_k(I)[2] else [])
        for how in hows:
            w3 = ws[how == "bf16"]
            Z = mc.hidden_sums_f32(rows[:, :I], w3[:, :I * H].reshape(3, I, H), "split" if how == "two_terms" else how,
                                   two_terms=how == "two_terms")
            passes[how] = [mc.outputs_f32(Z[k], w3[k], topo) for k in range(3)]
        _TILED[shape, H] = (rows, ws, want, passes)
    return _TILED[shape, H]


def taus(task):
    return mc.TAUS if task == orc.TASK_REG else (None,)


def outside(shape, H, zo, bf16=False, twice=False):
    """[(units of the log-likelihood tolerance, (split, tau, k))] of one forward pass' outputs zo = [(z, out) of each vector] over
    the 600 rows, and the cells in which check_evaluation refuses them."""
    task, I, O = shape
    rows, ws, want, _ = tiled_cell(shape, H)
    units, refused = [], []
    for ntr, nte in mc.EVAL_SPLITS:
        for tau in taus(task):
            for k in range(3):
                z, out = zo[k]
                ev = mc.scores(task, (I, H, O), z, out, rows, ntr, nte, ws[bf16][k], tau, twice=ntr + nte - 1 if twice else None)
                ref = want[bf16][(ntr, nte), tau, k]
                units.append((max(abs(ev[0] - ref["lik"]) / (1e-3 + 2e-5 * abs(ref["lik"])),
                                  abs(ev[6] - ref["lik_test"]) / (1e-3 + 2e-5 * abs(ref["lik_test"]))), ((ntr, nte), tau, k)))
                try:
                    check_evaluation(ev, ref, task, ntr, nte, f"{shape} {H} {ntr} {nte} {tau} w{k}")
                except AssertionError:
                    refused.append(((ntr, nte), tau, k))
    return units, refused


def test_tiled_list_is_what_the_matrix_core_passes_can_run():
    """Every entry a multiple of 32 in (64, 512] (wide_mfma; MAX_HIDDEN = 8 waves of 64), an odd and an even tile count (the tail of
    the two-stage tile pipeline), more waves than row blocks somewhere, waves without a group of two row blocks, an odd block count
    (the repeated block), uneven work over the waves at 600 rows, and a training set that ends inside a block in three row sets."""
    text = open(os.path.join(ROOT, "parallel-tempering-neural-net_amd", "csrc", "ptnn.hip")).read()
    assert re.search(r"MAX_HIDDEN = MAX_WAVES \* WAVE;", text)
    assert mc.TILED == (96, 128, 160, 512) and "tiled" not in mc.FAMILIES and not set(mc.TILED) & set(HIDDEN)
    assert all(64 < H <= 512 and H % 32 == 0 for H in mc.TILED)
    tiles = [H // 32 for H in mc.TILED]
    nw = [-(-H // 64) for H in mc.TILED]
    assert tiles == [3, 4, 5, 16] and nw == [2, 2, 3, 8]
    assert any(t % 2 for t in tiles) and any(t % 2 == 0 for t in tiles)
    nrb = [-(-(a + b) // 32) for a, b in mc.EVAL_SPLITS]
    assert nrb == [1, 2, 3, 19]
    assert any(w > b for w in nw for b in nrb) and any(b % 2 for b in nrb[1:]) and all(nrb[-1] % w for w in nw)
    assert all(a % 32 for a, _ in mc.EVAL_SPLITS[1:])
    # SplitK<n_in> as the header has it: which shapes have the split pass, their bf16 k-steps and fp32 remainder steps
    assert {s[1]: mc.split_k(s[1]) for s in mc.SHAPES} == {4: (0, 2, False), 5: (0, 3, False), 6: (0, 3, False), 9: (1, 0, True),
                                                           11: (1, 0, True), 16: (1, 0, True), 20: (1, 2, True), 32: (2, 0, True),
                                                           34: (2, 1, True)}
    coop = open(os.path.join(ROOT, "parallel-tempering-neural-net_amd", "csrc", "ptnn_dev_coop.hpp")).read()
    for line in ("PADLAST = REM0 >= 7;", "KB = KB0 + (PADLAST ? 1 : 0);", "KR = (REM + 1) / 2;", "OK = (KB == 1 || KB == 2 || KB == 4);"):
        assert line in coop, line


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3, 0.0, 3.0e38 / 2], dtype=np.float32)
    r = mc.bf16_round(x)
    assert r.dtype == np.float32 and r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0 + 2.0 ** -6 and r[3] == 1.0 + 2.0 ** -7 and r[5] == 0.0
    assert (r.view(np.uint32) & 0xFFFF == 0).all() and np.all(np.abs(r - x) <= np.abs(x) * 2.0 ** -8)
    hi, mid, lo = mc.split3(x)
    assert np.all(np.abs((hi.astype(np.float64) + mid + lo) - x) <= np.abs(x) * 2.0 ** -24)


def test_tiled_seeds_are_the_smallest_usable_moves():
    for shape in mc.SHAPES:
        rows = mc.eval_data(shape)
        for H in mc.TILED:
            for moves, ok, bf in ((mc.TILED_SEED_MOVES, mc.usable, False), (mc.TILED_BF16_SEED_MOVES, mc.usable_bf16, True)):
                ws = mc.tiled_weights(shape, H, bf16=bf)
                assert ok(shape, H, ws, rows), (shape, H, bf)
                assert np.array_equal(ws, ws.astype(np.float32).astype(np.float64))
                for lower in range(moves.get((shape, H), 0)):
                    assert not ok(shape, H, mc.weights(shape, H, seed=mc.weight_seed(shape, H) + 100000 * lower), rows), (shape, H, lower)
    assert all(H in mc.TILED and s in mc.SHAPES for s, H in list(mc.TILED_SEED_MOVES) + list(mc.TILED_BF16_SEED_MOVES))


def test_scores_restate_the_oracles_evaluation():
    """model_cases.scores on the float64 forward pass is model_cases.evaluate, to float64 round-off, on a regression and a
    many-class cell; and evaluate_bf16 is evaluate but for the rounded operands (the prior excepted)."""
    for shape, H in (((0, 5, 1), 96), ((1, 11, 10), 160)):
        task, I, O = shape
        rows, ws, want, _ = tiled_cell(shape, H)
        for ntr, nte in mc.EVAL_SPLITS:
            for tau in taus(task):
                z, out = mc.outputs_wrong(rows[:, :I], ws[False][1], (I, H, O), None)
                ev = mc.scores(task, (I, H, O), z, out, rows, ntr, nte, ws[False][1], tau)
                ref = want[False][(ntr, nte), tau, 1]
                names = ("lik", "rmse_train", "rmse_test", "acc_train", "acc_test", "prior", "lik_test")
                for j, nm in enumerate(names):
                    if nm in ref:
                        assert ev[j] == pytest.approx(ref[nm], rel=1e-12, abs=1e-12), (shape, ntr, nm)
                bf = want[True][(ntr, nte), tau, 1]
                if np.array_equal(ws[True][1], ws[False][1]):
                    assert bf["prior"] == ref["prior"] and bf["lik"] != ref["lik"]


def test_float32_restatements_of_the_tiled_passes_stay_inside_the_tolerances():
    worst = {}
    for shape in mc.SHAPES:
        for H in mc.TILED:
            passes = tiled_cell(shape, H)[3]
            for how in ("exact", "bf16", "split"):
                if how in passes:
                    units, refused = outside(shape, H, passes[how], bf16=how == "bf16")
                    assert not refused, (how, shape, H, refused)
                    worst[how] = max(worst.get(how, (0.0,)), (max(units)[0], shape, H, max(units)[1]))
    print("MODEL_SHAPES tiled float32 restatements, worst |lik - float64| / (1e-3 + 2e-5 |lik|): "
          + "; ".join(f"{how} {v[0]:.4f} at {v[1:]}" for how, v in worst.items()))
    assert set(worst) == {"exact", "bf16", "split"}


TILED_MUTANTS = ("input_last", "remainder", "unit_last", "row_twice")


@pytest.mark.parametrize("mutant", TILED_MUTANTS)
def test_structurally_wrong_tiled_forwards_fall_outside_the_tolerances(mutant):
    """... in at least one row set of every (shape, H) the mutant applies to, under every one of the three vectors."""
    seen = 0
    for shape in mc.SHAPES:
        task, I, O = shape
        if mutant == "remainder" and mc.split_k(I)[1:] not in ((1, True), (2, True)):
            continue
        for H in mc.TILED:
            rows, ws, _, _ = tiled_cell(shape, H)
            kind = None if mutant == "row_twice" else mutant
            zo = [mc.outputs_wrong(rows[:, :I], ws[False][k], (I, H, O), kind) for k in range(3)]
            _, refused = outside(shape, H, zo, twice=mutant == "row_twice")
            assert {k for _, _, k in refused} == {0, 1, 2}, (mutant, shape, H, refused)
            seen += 1
    assert seen == (2 if mutant == "remainder" else len(mc.SHAPES)) * len(mc.TILED)


def test_two_term_split_is_measured_not_promised():
    """The split pass reduced to hi + mid (16 significant bits an operand, products good to 2^-16) against float64: how many cells of
    the grid the tolerances refuse, and how far the log-likelihood is off.  Printed; DESIGN.md has the figures and what follows."""
    cells, caught, worst = 0, 0, (0.0,)
    for shape in mc.SHAPES:
        for H in mc.TILED:
            passes = tiled_cell(shape, H)[3]
            if "two_terms" in passes:
                units, refused = outside(shape, H, passes["two_terms"])
                cells += 1
                caught += bool(refused)
                worst = max(worst, (max(units)[0], shape, H, max(units)[1]))
    print(f"MODEL_SHAPES tiled two-term split: refused in {caught} of {cells} (shape, H); worst |lik - float64| / (1e-3 + 2e-5 |lik|) "
          f"{worst[0]:.3f} at {worst[1:]}")
    assert cells == 6 * len(mc.TILED)
