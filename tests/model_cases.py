"""The cases on which the sampler's own device functions -- the SGD epoch (Sampler.langevin_gradient: sgd_sweep, sgd_sweep_wide_n) and
the model evaluation (Sampler.evaluate: build_fw + eval_rows, the wide forward) -- are compared with the float64 oracle at every
compiled shape: shapes, hidden sizes, generators, the seed of every case, the error unit and its bound, a float32 restatement of the
epoch and the wrong epochs the bound must tell from the right one.  tests/test_gpu_model_shapes.py runs the cases on the device;
tests/test_model_cases_cpu.py proves, from the oracle alone, that the bound leaves room for float32 and none for the wrong epochs.
The tiled family (TILED) holds the matrix-core forward passes of the wide nets: tests/test_gpu_tiled_forward.py, with float32
restatements of their summations, a bf16 operand model and the wrong forwards the evaluation's tolerances must refuse.
Nothing here reads anything but the oracle."""
import numpy as np

import ptnn_oracle as orc

# (task, n_in, n_out): PTNN_SHAPES of csrc/ptnn_shapes.hpp (the CPU test holds this list to the header)
SHAPES = [(0, 4, 1), (0, 5, 1), (0, 32, 1), (1, 4, 3), (1, 34, 2), (1, 9, 2), (1, 11, 10), (1, 20, 2), (1, 16, 10), (1, 6, 18)]
# narrow: one hidden unit, a partial group, and both sides of every lane-group edge of sgd_sweep (NRED 3|4|5|6: 8|9, 16|17, 32|33, 64);
# wide: one past the wave, not a multiple of 32 or 64, and more than two waves
NARROW = (1, 3, 8, 9, 16, 17, 32, 33, 64)
WIDE = (65, 100, 130)
FAMILIES = {"narrow": NARROW, "wide": WIDE}

# ---- the epoch grid: the first Ntr rows of one 64-row draw.  rem 0..3 of the deferred chain, zero / one / several passes of its 4-row
# loop, odd and even tails of the plain chain, the one- and two-row start-up of the wide loop
EPOCH_ROWS, EPOCH_NTE = 64, 5
NTRS = (1, 2, 3, 4, 5, 7, 8, 31)
LRS = (0.1, 0.01)
# ---- the evaluation grid: (Ntr, Nte) prefixes of one 600-row draw: Nall below a wave, one past a wave (with 31 and 60 training rows),
# and 600 rows on 512 threads (lanes with two rows and lanes with one)
EVAL_ROWS = 600
EVAL_SPLITS = ((1, 1), (31, 5), (60, 5), (420, 180))
TAUS = (0.01, 0.1)

# ---- the error unit of the epoch: r(v) = max_j |v_j - ref_j| / (2e-5 + 1e-4 |ref_j|), the suite's rtol = 1e-4, atol = 2e-5 at r = 1
R_ATOL, R_RTOL = 2e-5, 1e-4
F32_WORST = 0.1 / 16        # the float32 restatement of the epoch stays below this over the whole grid (test_model_cases_cpu.py)
R_BOUND = 16 * F32_WORST    # what the device is held to: rtol = 1e-5, atol = 2e-6
MUTANT_MIN = 2 * R_BOUND    # every wrong epoch is at least this far from the right one

MUTANTS = ("last_row_w1b1", "unit_last", "input_last", "last_row_b2_last")     # the last one: n_out > 1 only
SIGMA_SQUARED, NU_1, NU_2 = 25.0, 0.0, 0.0                                       # parity.make_sampler's prior

# A weight seed is 1000 n_in + H: for the epoch cases always; for the evaluation cases (eval_weights) moved by 100000 k for the
# (shape, H) whose three vectors would otherwise leave an evaluation row with its two largest output pre-activations closer than
# TIE_GAP (argmax would be a matter of rounding), or (regression) a row set whose RMSE float32 outputs cannot give to RMSE_RTOL:
# the smallest such k.  A float32 forward is up to RMSE_ULPS ulp off at its worst row (the float32 restatement of the oracle's
# forward: 6.9 over the grid); where a prediction nearly hits its target, as in a set of one row, the RMSE is what cancellation
# leaves of that error.
TIE_GAP, Z_MAX = 1e-4, 30.0
RMSE_RTOL, RMSE_ULPS = 1e-5, 8.0
SEED_MOVES = {((0, 4, 1), 16): 3, ((0, 4, 1), 32): 2, ((0, 4, 1), 64): 2, ((0, 5, 1), 9): 1, ((0, 5, 1), 33): 3, ((0, 5, 1), 64): 4,
              ((0, 5, 1), 130): 6, ((0, 32, 1), 9): 1, ((0, 32, 1), 17): 1, ((0, 32, 1), 64): 3, ((0, 32, 1), 65): 2, ((0, 32, 1), 100): 1,
              ((0, 32, 1), 130): 2, ((1, 34, 2), 64): 1, ((1, 9, 2), 8): 1, ((1, 9, 2), 33): 1, ((1, 11, 10), 1): 1, ((1, 11, 10), 64): 1,
              ((1, 16, 10), 9): 1, ((1, 16, 10), 16): 1, ((1, 16, 10), 17): 1, ((1, 16, 10), 64): 1, ((1, 6, 18), 1): 1, ((1, 6, 18), 3): 1,
              ((1, 6, 18), 33): 1, ((1, 6, 18), 100): 1, ((1, 6, 18), 130): 1}


def r_unit(v, ref):
    v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(v - ref) / (R_ATOL + R_RTOL * np.abs(ref))))


def data(task, I, O, rows, seed):
    """[rows, I + 1] float64 holding float32 values: X ~ N(0, 1); labels argmax(X proj + 0.5 noise); target sigmoid(X . v / sqrt(I))."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, I))
    if task == orc.TASK_CLS:
        proj = rng.standard_normal((I, O))
        y = np.argmax(X @ proj + 0.5 * rng.standard_normal((rows, O)), axis=1).astype(np.float64)
    else:
        y = orc.sigmoid(X @ rng.standard_normal(I) / np.sqrt(I))
    return np.hstack([X, y[:, None]]).astype(np.float32).astype(np.float64)


def epoch_data(shape):
    """(the 64 rows the training sets are prefixes of, the 5 test rows)."""
    task, I, O = shape
    d = data(task, I, O, EPOCH_ROWS + EPOCH_NTE, 500000 + 1000 * I + O)
    return d[:EPOCH_ROWS], d[EPOCH_ROWS:]


def eval_data(shape):
    task, I, O = shape
    return data(task, I, O, EVAL_ROWS, 700000 + 1000 * I + O)


def weight_seed(shape, H):
    return 1000 * shape[1] + H


def weights(shape, H, seed=None):
    """Three vectors [3, P] float64 holding float32 values, fan-in scaled so that no layer saturates."""
    _, I, O = shape
    rng = np.random.default_rng(weight_seed(shape, H) if seed is None else seed)
    out = []
    for _ in range(3):
        W1 = rng.standard_normal((I, H)) / np.sqrt(I)
        W2 = 2.0 * rng.standard_normal((H, O)) / np.sqrt(H)
        B1 = 0.5 * rng.standard_normal(H)
        B2 = 0.5 * rng.standard_normal(O)
        out.append(np.concatenate([W1.ravel(), W2.ravel(), B1, B2]))
    return np.stack(out).astype(np.float32).astype(np.float64)


def eval_weights(shape, H):
    """The vectors of the evaluation cases: weights() from the seed moved as SEED_MOVES says."""
    return weights(shape, H, seed=weight_seed(shape, H) + 100000 * SEED_MOVES.get((shape, H), 0))


def epoch(train, w, topo, lr, task, dtype=np.float64, mutant=None):
    """oracle.langevin_gradient (the plain chain, file order) for a batch: w [B, P], lr a scalar or [B] -> [B, P] of `dtype`, every
    array of the chain held in `dtype` (float32: the restatement whose distance from float64 sizes the bound).
    mutant: None, one of MUTANTS (last_row_w1b1: the last row's W1 / B1 update dropped; unit_last: hidden unit H-1 never updated;
    input_last: input column I-1 never updated; last_row_b2_last: the last class's B2 update of the last row undone), or "post_w2":
    the hidden deltas taken with the post-update W2 (quirk Q4 the wrong way round)."""
    I, H, O = topo
    w = np.array(np.atleast_2d(w), dtype=dtype, copy=True)
    B = w.shape[0]
    lr = np.broadcast_to(np.asarray(lr, dtype=dtype), (B,)).astype(dtype)[:, None]
    a, b = I * H, I * H + H * O
    W1, W2, B1, B2 = w[:, :a].reshape(B, I, H), w[:, a:b].reshape(B, H, O), w[:, b:b + H], w[:, b + H:]      # views into w
    one = dtype(1)
    X = np.asarray(train[:, :I], dtype=dtype)
    Y = np.asarray(train[:, I])
    N = train.shape[0]
    for n in range(N):
        x = X[n]
        hid = one / (one + np.exp(-(np.matmul(x, W1) - B1)))                                # [B, H]
        out = one / (one + np.exp(-(np.matmul(hid[:, None, :], W2)[:, 0, :] - B2)))         # [B, O]
        if task == orc.TASK_CLS:
            t = np.zeros(O, dtype=dtype)
            t[int(Y[n])] = one
        else:
            t = dtype(Y[n])
        od = (t - out) * (out * (one - out))
        dW2 = lr[:, :, None] * (hid[:, :, None] * od[:, None, :])
        if mutant == "post_w2":
            hd = np.matmul(W2 + dW2, od[:, :, None])[:, :, 0] * (hid * (one - hid))
        else:
            hd = np.matmul(W2, od[:, :, None])[:, :, 0] * (hid * (one - hid))               # pre-update W2 (Q4)
        dB2 = lr * od
        dW1 = lr[:, :, None] * (x[None, :, None] * hd[:, None, :])
        dB1 = lr * hd
        if mutant == "unit_last":
            dW2[:, H - 1, :] = 0
            dW1[:, :, H - 1] = 0
            dB1[:, H - 1] = 0
        elif mutant == "input_last":
            dW1[:, I - 1, :] = 0
        elif n == N - 1 and mutant == "last_row_w1b1":
            dW1[:], dB1[:] = 0, 0
        elif n == N - 1 and mutant == "last_row_b2_last":
            dB2[:, O - 1] = 0
        W2 += dW2
        B2 -= dB2
        W1 += dW1
        B1 -= dB1
    return w


def evaluate(task, topo, train, test, w, tau_sq=None):
    """What Sampler.evaluate returns for one vector, from the oracle: log-likelihood of the training rows at T = 1, RMSE train / test,
    the prior, log-likelihood of the test rows; classification also the accuracies, and the integers behind them: rows classified
    right and the sum of squared class differences, (train, test)."""
    if task == orc.TASK_REG:
        lik, _, rm = orc.likelihood_reg(train, w, tau_sq, topo, 1.0)
        lik_te, _, rm_te = orc.likelihood_reg(test, w, tau_sq, topo, 1.0)
        return dict(lik=lik, rmse_train=rm, rmse_test=rm_te, prior=orc.prior_reg(SIGMA_SQUARED, NU_1, NU_2, w, tau_sq, topo),
                    lik_test=lik_te)
    I = topo[0]
    lik, fx, rm = orc.likelihood_cls(train, w, topo, 1.0)
    lik_te, fx_te, rm_te = orc.likelihood_cls(test, w, topo, 1.0)
    return dict(lik=lik, rmse_train=rm, rmse_test=rm_te, prior=orc.prior_cls(SIGMA_SQUARED, w, topo), lik_test=lik_te,
                acc_train=orc.accuracy(fx, train[:, I]), acc_test=orc.accuracy(fx_te, test[:, I]),
                right=(int(np.count_nonzero(fx == train[:, I])), int(np.count_nonzero(fx_te == test[:, I]))),
                sq=(int(round(float(np.sum((fx - train[:, I]) ** 2)))), int(round(float(np.sum((fx_te - test[:, I]) ** 2))))))


def pre_activations(rows, w, topo):
    """Output pre-activations [N, O] in float64."""
    W1, W2, B1, B2 = orc.decode(w, topo)
    return orc.sigmoid(rows[:, :topo[0]] @ W1 - B1) @ W2 - B2


def rmse_ulp_sensitivity(f, y):
    """The relative change of sqrt(mean((f - y)^2)) when every output f_i moves by one float32 ulp, all to the worse side (first
    order): sum |d_i| ulp(f_i) / sum d_i^2.  For a single row it is ulp(f) / |f - y|: the RMSE of a row whose prediction nearly hits
    the target is a difference of two close numbers, and float32 cannot hold it to any relative tolerance."""
    d = f - y
    return float(np.sum(np.abs(d) * np.spacing(f.astype(np.float32)).astype(np.float64)) / np.sum(d * d))


def rmse_conditioned(shape, H, ws, rows, splits=None):
    """Regression: in every row set of `splits` (EVAL_SPLITS) and under each vector, outputs RMSE_ULPS float32 ulp off move the RMSE
    by no more than RMSE_RTOL."""
    splits = EVAL_SPLITS if splits is None else splits
    task, I, O = shape
    if task != orc.TASK_REG:
        return True
    for w in ws:
        f = orc.forward(rows[:, :I], w, (I, H, O))[1].ravel()
        for ntr, nte in splits:
            for part in (slice(0, ntr), slice(ntr, ntr + nte)):
                if RMSE_ULPS * rmse_ulp_sensitivity(f[part], rows[part, I]) > RMSE_RTOL:
                    return False
    return True


def usable(shape, H, ws, rows, splits=None):
    """What a weight seed has to give on the evaluation rows: see SEED_MOVES."""
    return tie_free(shape, H, ws, rows) and rmse_conditioned(shape, H, ws, rows, splits)


def forward_f32(X, w, topo):
    """The oracle's forward with every array float32 -> outputs [N, O] float32."""
    I, H, O = topo
    w, X, one = np.asarray(w, dtype=np.float32), np.asarray(X, dtype=np.float32), np.float32(1)
    a, b = I * H, I * H + H * O
    hid = one / (one + np.exp(-(X @ w[:a].reshape(I, H) - w[b:b + H])))
    return one / (one + np.exp(-(hid @ w[a:b].reshape(H, O) - w[b + H:])))


# ---- long evaluation cases: the row blockings of eval_rows the 600 rows do not reach.  A lane takes its rows in blocks of RB = 8
# (n_in <= 7), 4 (n_in <= 15) or 2, then 4, 2, 1 for what is left, of cnt = ceil(Nall / threads) rows; 600 rows on 512 threads are
# cnt = 2.  Wide nets read their rows from global memory (128 threads at H = 65 and 100: cnt = 15 = 8 + 4 + 2 + 1; 192 at H = 130:
# cnt = 10 = 8 + 2); narrow nets hold them in LDS, which bounds the rows: cnt = 7 = 4 + 2 + 1 and cnt = 8 for n_in <= 7 on the unit-row
# (H = 9) and the pair image (H = 16), cnt = 4 and cnt = 5 = 4 + 1 for n_in = 9 and 11.
LONG_ROWS = 3600
LONG_WIDE_SPLITS = ((1300, 620),)
LONG_NARROW = {4: ((9, 16), ((2500, 600), (2900, 700))), 5: ((9, 16), ((2500, 600), (2900, 700))), 6: ((9, 16), ((2500, 600), (2900, 700))),
               9: ((16,), ((1300, 300), (1700, 400))), 11: ((16,), ((1300, 300), (1700, 400)))}
# the weight seed of a long case: 1000 n_in + H + 100000 k with the smallest k that is usable() on the long rows
LONG_SEED_MOVES = {((1, 4, 3), 130): 1, ((1, 11, 10), 16): 1, ((1, 11, 10), 65): 1, ((1, 11, 10), 130): 2, ((1, 16, 10), 65): 1,
                   ((1, 6, 18), 16): 7, ((1, 6, 18), 100): 14, ((1, 6, 18), 130): 1}


def long_data(shape):
    task, I, O = shape
    return data(task, I, O, LONG_ROWS, 710000 + 1000 * I + O)


def long_cases(shape, family):
    """[(H, splits)] of the long evaluation cases of a shape and family (none for a narrow net of 16 inputs or more: two rows a
    block, which 600 rows already take, and no room in LDS for more)."""
    if family == "wide":
        return [(H, LONG_WIDE_SPLITS) for H in WIDE]
    hs, splits = LONG_NARROW.get(shape[1], ((), ()))
    return [(H, splits) for H in hs]


def long_weights(shape, H):
    return weights(shape, H, seed=weight_seed(shape, H) + 100000 * LONG_SEED_MOVES.get((shape, H), 0))


def model_threads(H, Nall):
    """Threads of the model kernel (plan_launch, plan_wide of csrc/ptnn.hip)."""
    if H > 64:
        return (H + 63) // 64 * 64
    pow2 = 1
    while pow2 < (Nall + 63) // 64:
        pow2 *= 2
    return min(pow2, 8) * 64


def eval_blocks(I, H, Nall):
    """The row blockings eval_rows runs for a net of I inputs and H hidden units on Nall rows, as a set."""
    rb = 8 if (I + 1) * 8 <= 64 else 4 if (I + 1) * 4 <= 64 else 2 if (I + 1) * 2 <= 80 else 1
    cnt = -(-Nall // model_threads(H, Nall))
    out = set()
    if cnt >= rb:
        out.add(rb)
    cnt %= rb
    for b in (4, 2, 1):
        if b < rb and cnt >= b:
            out.add(b)
            cnt -= b
    return out


def model_lds_bytes(shape, H, Nall):
    """LDS of a narrow net's model kernel (lds_floats of csrc/ptnn_dev_sweep_forward.hpp): the rows, seven vectors, the forward image."""
    _, I, O = shape
    r4 = lambda v: (v + 3) & ~3
    PS, IPY, FWS = r4(I * H + H * O + H + O + 1), r4(I + 2), r4(I + 1 + O)
    return 4 * ((Nall + 2) * IPY + 7 * PS + (2 * ((H + 1) // 2) + 1) * FWS + 8 * 8 + 16)


def tie_free(shape, H, ws, rows):
    """No row of `rows` has, under any of the vectors, a pre-activation of Z_MAX or more, or (classification) its two largest
    closer than TIE_GAP."""
    task, I, O = shape
    for w in ws:
        z = pre_activations(rows, w, (I, H, O))
        if np.abs(z).max() >= Z_MAX:
            return False
        if task == orc.TASK_CLS:
            zs = np.sort(z, axis=1)
            if (zs[:, -1] - zs[:, -2]).min() < TIE_GAP:
                return False
    return True


# ---- the tiled family: wide nets whose hidden layer is a multiple of 32 take a matrix-core forward pass (wide_forward of
# csrc/ptnn_dev_wide.hpp): H / 32 tiles, ceil(H / 64) waves.  96: 3 tiles on 2 waves, the two-stage tile pipeline of the split pass
# ends on its odd tail; 128: 4 tiles, the even tail; 160: 5 tiles on 3 waves; 512: 16 tiles on 8 waves, more waves than the small row
# sets have row blocks, and the widest net there is.  The evaluation rows and EVAL_SPLITS stay: Nall = 2, 36, 65, 600 are 1, 2, 3
# and 19 blocks of 32 rows, and Ntr = 31, 60, 420 each fall inside a block.  NOT in FAMILIES: the epoch does not depend on tiling.
TILED = (96, 128, 160, 512)
# forward_bf16: 0 the default (split bf16 operands where SplitK<n_in> has them, else the exact fp32 instruction), 2 exact fp32, 1 bf16
TILED_MODES = (0, 2, 1)
# weight seeds of the tiled evaluation cases, by the rule of SEED_MOVES: the smallest k that is usable() ...
TILED_SEED_MOVES = {((0, 4, 1), 96): 1, ((0, 4, 1), 160): 1, ((0, 32, 1), 96): 1, ((1, 34, 2), 512): 1, ((1, 16, 10), 160): 2,
                    ((1, 6, 18), 160): 1}
# ... and, for the cases with bf16 operands (forward_bf16 = 1), usable() on the rounded operands as well as on the plain ones
TILED_BF16_SEED_MOVES = {((0, 4, 1), 96): 1, ((0, 4, 1), 160): 1, ((0, 32, 1), 96): 1, ((1, 34, 2), 512): 1, ((1, 20, 2), 96): 2,
                         ((1, 16, 10), 96): 3, ((1, 16, 10), 128): 1, ((1, 16, 10), 160): 2, ((1, 6, 18), 160): 3}


def tiled_weights(shape, H, bf16=False):
    moves = TILED_BF16_SEED_MOVES if bf16 else TILED_SEED_MOVES
    return weights(shape, H, seed=weight_seed(shape, H) + 100000 * moves.get((shape, H), 0))


def split_k(I):
    """SplitK<I> of csrc/ptnn_dev_coop.hpp -> (KB bf16 k-steps of 16, KR fp32 k-steps of 2 behind them, whether the split pass exists)."""
    kb, rem = divmod(I, 16)
    if rem >= 7:                    # PADLAST: a zero-padded bf16 k-step
        kb, rem = kb + 1, 0
    return kb, (rem + 1) // 2, kb in (1, 2, 4)


def tiled_pass(I, mode):
    """The forward pass a tiled wide net of I inputs takes under forward_bf16 = mode: "split", "exact" or "bf16"."""
    return "bf16" if mode == 1 else "split" if mode == 0 and split_k(I)[2] else "exact"


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even) as float32: the integer form of f32_to_bf16 (csrc/ptnn_dev_coop.hpp); finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return (u << np.uint32(16)).view(np.float32)


def bf16_operands(topo, rows, w):
    """What eval_rows_mfma<..., true> rounds: the input columns of the rows and W1; B1, W2, B2 and the targets stay.  float64 copies."""
    I, H, _ = topo
    rows, w = np.array(rows, dtype=np.float64), np.array(w, dtype=np.float64)
    rows[:, :I] = bf16_round(rows[:, :I])
    w[..., :I * H] = bf16_round(w[..., :I * H])
    return rows, w


def evaluate_bf16(task, topo, train, test, w, tau_sq=None):
    """evaluate() of a net whose forward product has bf16 operands; the prior is that of the vector as it is."""
    tr, wr = bf16_operands(topo, train, w)
    te, _ = bf16_operands(topo, test, w)
    out = evaluate(task, topo, tr, te, wr, tau_sq)
    w = np.asarray(w, dtype=np.float64)
    out["prior"] = (orc.prior_reg(SIGMA_SQUARED, NU_1, NU_2, w, tau_sq, topo) if task == orc.TASK_REG
                    else orc.prior_cls(SIGMA_SQUARED, w, topo))
    return out


def usable_bf16(shape, H, ws, rows, splits=None):
    """usable() on the operands as given and as forward_bf16 = 1 rounds them."""
    rr, wr = bf16_operands((shape[1], H, shape[2]), rows, ws)
    return usable(shape, H, ws, rows, splits) and usable(shape, H, wr, rr, splits)


def split3(x):
    """x = hi + mid + lo, three bf16 roundings of a float32 array (x - hi and x - hi - mid are exact in float32)."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_round(x)
    r = x - hi
    mid = bf16_round(r)
    return hi, mid, bf16_round(r - mid)


def hidden_sums_f32(X, W1, how, two_terms=False):
    """A float32 restatement of the hidden pre-activation sums X @ W1 of one matrix-core pass: X [N, I], W1 [B, I, H] -> [B, N, H]
    float32, one float32 accumulator per element, one rounding per product added.
    "exact": k ascending, fused multiply-add (the product is exact in float64).  "bf16": operands rounded to bf16 (products exact in
    float32), k ascending.  "split": per bf16 k-step the six products in the kernel's order, small terms first -- W1.lo X.hi,
    W1.hi X.lo, W1.mid X.mid of every k-step, then W1.mid X.hi, W1.hi X.mid, then W1.hi X.hi -- and the columns k >= 16 KB behind
    them as in "exact".  two_terms: the split reduced to hi + mid (the four products without a lo term): a WRONG pass."""
    X, W1 = np.asarray(X, dtype=np.float32), np.asarray(W1, dtype=np.float32)
    I = X.shape[1]
    acc = np.zeros((W1.shape[0], X.shape[0], W1.shape[2]), dtype=np.float32)

    def add(xk, wk, fused=False):
        nonlocal acc
        if fused:
            acc = (acc + xk.astype(np.float64)[None, :, None] * wk.astype(np.float64)[:, None, :]).astype(np.float32)
        else:
            acc += xk[None, :, None] * wk[:, None, :]
    if how == "exact":
        for k in range(I):
            add(X[:, k], W1[:, k], fused=True)
        return acc
    if how == "bf16":
        Xb, Wb = bf16_round(X), bf16_round(W1)
        for k in range(I):
            add(Xb[:, k], Wb[:, k])
        return acc
    assert how == "split", how
    KB = split_k(I)[0]
    xs, ws = split3(X), split3(W1)                                   # (hi, mid, lo)
    HI, MID, LO = 0, 1, 2
    groups = (((LO, HI), (HI, LO), (MID, MID)), ((MID, HI), (HI, MID)), ((HI, HI),))
    for group in groups:
        for s in range(KB):
            for a, b in group:
                if two_terms and LO in (a, b):
                    continue
                for k in range(16 * s, min(16 * s + 16, I)):
                    add(xs[b][:, k], ws[a][:, k])
    for k in range(16 * KB, I):
        add(X[:, k], W1[:, k], fused=True)
    return acc


def outputs_f32(Z, w, topo):
    """The rest of the forward pass in float32 from the hidden sums Z [N, H]: -> (output pre-activations, outputs) [N, O] float32."""
    I, H, O = topo
    w, one = np.asarray(w, dtype=np.float32), np.float32(1)
    a, b = I * H, I * H + H * O
    hid = one / (one + np.exp(-(np.asarray(Z, dtype=np.float32) - w[b:b + H])))
    z = hid @ w[a:b].reshape(H, O) - w[b + H:]
    return z, one / (one + np.exp(-z))


def outputs_wrong(X, w, topo, mutant):
    """float64 (output pre-activations, outputs) of a structurally wrong forward pass: "input_last" (input column I - 1 never
    multiplied), "remainder" (the columns k >= 16 KB behind the bf16 k-steps never multiplied), "unit_last" (hidden unit H - 1, the
    last of the last tile, left out of the product with W2); None: the right one."""
    I, H, O = topo
    W1, W2, B1, B2 = orc.decode(np.asarray(w, dtype=np.float64), topo)
    keep = np.ones(I)
    if mutant == "input_last":
        keep[I - 1] = 0
    elif mutant == "remainder":
        keep[16 * split_k(I)[0]:] = 0
        assert keep.sum() < I
    hid = orc.sigmoid((X * keep) @ W1 - B1)
    if mutant == "unit_last":
        hid[:, H - 1] = 0
    z = hid @ W2 - B2
    return z, orc.sigmoid(z)


def scores(task, topo, z, out, rows, ntr, nte, w, tau_sq=None, twice=None):
    """One vector's row of Sampler.evaluate (log-likelihood, RMSE train / test, accuracy train / test, prior, log-likelihood of the
    test rows, 0) from the outputs of a forward pass over `rows` = the ntr + nte rows: out [N, O], and z, the output pre-activations
    the class is taken from (tie_free: no row's argmax is a matter of rounding).  The sums over rows in float64, as the model kernel
    forms them (finish_eval): per-row terms, N = the row count.  twice: a row that is scored twice (a WRONG evaluation)."""
    I = topo[0]
    y = rows[:ntr + nte, I]
    out = np.asarray(out, dtype=np.float64)[:ntr + nte]
    cnt = np.ones(ntr + nte)
    if twice is not None:
        cnt[twice] += 1
    parts = (slice(0, ntr), slice(ntr, ntr + nte))
    ev = np.zeros(8)
    if task == orc.TASK_REG:
        a = (y - out[:, 0]) ** 2 * cnt
        ssq = [float(a[p].sum()) for p in parts]
        n = (ntr, nte)
        lik = [-0.5 * n[j] * np.log(2.0 * np.pi * tau_sq) - 0.5 * ssq[j] / tau_sq for j in range(2)]
        ev[0], ev[6] = lik
        ev[1], ev[2] = np.sqrt(ssq[0] / ntr), np.sqrt(ssq[1] / nte)
        ev[5] = orc.prior_reg(SIGMA_SQUARED, NU_1, NU_2, np.asarray(w, dtype=np.float64), tau_sq, topo)
        return ev
    arg = np.argmax(np.asarray(z)[:ntr + nte], axis=1).astype(np.float64)
    a = (out[np.arange(ntr + nte), y.astype(np.int64)] - np.log(np.exp(out).sum(axis=1))) * cnt
    ev[0], ev[6] = (float(a[p].sum()) for p in parts)
    ev[1], ev[2] = (np.sqrt(float((((arg - y) ** 2) * cnt)[p].sum()) / n) for p, n in zip(parts, (ntr, nte)))
    ev[3], ev[4] = (100.0 * float(((arg == y) * cnt)[p].sum()) / n for p, n in zip(parts, (ntr, nte)))
    ev[5] = orc.prior_cls(SIGMA_SQUARED, np.asarray(w, dtype=np.float64), topo)
    return ev


# ---- the regimes of np.argmax over float64 sigmoid outputs (argmax_key of the device): cases for two small nets, a few rows ----------------
ARGMAX_SHAPES = (((1, 4, 3), 3), ((1, 6, 18), 8))
ARGMAX_ROWS = (13, 8)
# name -> {class: pre-activation it is given}; the other classes stay ordinary (|z| of order 1).  e^-z 2^52 is 2.84 at z = 35,
# 1.04 at 36 and 0.86 at 36.2: float64 outputs 1 - 3 ulp, 1 - 1 ulp, 1 - 1 ulp; from 36.74 on every output is exactly 1.
ARGMAX_REGIMES = {
    "saturated_first_wins": {1: 40.0, 2: 45.0},         # both outputs exactly 1.0: class 1, not the larger z
    "quantised_different": {0: 35.0, 2: 36.0},          # outputs differ in float64 (and are both 1.0f in fp32): class 2
    "quantised_equal": {1: 36.0, 2: 36.2},              # the same float64 output: class 1, the first, although z[2] > z[1]
    "underflow_one": {0: -720.0},                       # np.exp overflows: output exactly 0.0, any ordinary class beats it
    "underflow_all": None,                              # every class below -709.78, the last the largest: all 0.0, class 0
}


def argmax_case(shape, H, regime):
    """(train, test, w float64 of float32 values, {class: z}) of one regime: the special classes get W2 columns of at most 0.002 in
    size (|hid . W2| <= 0.002 H) and B2 = -z, so that their pre-activation is the stated one within 0.02 on every row."""
    task, I, O = shape
    d = data(task, I, O, sum(ARGMAX_ROWS), 900000 + 1000 * I + O)
    d[:, I] = np.arange(d.shape[0]) % O                         # every class among the labels, as far as the rows reach
    w = weights(shape, H, seed=900000 + 1000 * I + H)[0]
    spec = ARGMAX_REGIMES[regime]
    if spec is None:
        spec = {o: -715.0 - 1.0 * (O - 1 - o) for o in range(O)}
    W1, W2, B1, B2 = orc.decode(w, (I, H, O))                  # views
    rng = np.random.default_rng(17)
    for o, z in spec.items():
        W2[:, o] = rng.uniform(-0.002, 0.002, H)
        B2[o] = -z
    w = w.astype(np.float32).astype(np.float64)
    return d[:ARGMAX_ROWS[0]], d[ARGMAX_ROWS[0]:], w, spec
