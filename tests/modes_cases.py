"""The planted cases of the posterior-modes tests: three groups of weight vectors on the (4, 5, 1) regression rows of
tests/uncertainty_cases.py and on the classification shape of tests/report_cases.py with the most outputs.  A group is a centre
(one of six widely spread vectors, three picked greedily at least 4 separations apart) with small relative perturbations; group 0
also holds copies of its first member with the hidden units permuted.  The members are interleaved, with multiplicities 1..3.
tests/test_modes_cpu.py proves the margins with the oracle's float64 forward; tests/test_gpu_modes.py runs them.  No device."""
import functools

import numpy as np

import report_cases
import uncertainty_cases
from parity import orc

REG_TOPO = (4, 5, 1)
CLS_TOPO = max(report_cases.SHAPES, key=lambda t: t[2])
# The separation of a case, in output units: 5 % of the range for the regression; the 18 softmax outputs of the classification
# shape all lie in [0.02, 0.14], and two widely spread nets differ by about 0.025 RMS there, so its separation is 0.005.
SEPARATION = {REG_TOPO: 0.05, CLS_TOPO: 0.005}
SIZES = (9, 6, 5)
N_PERMUTED = 2
NOISE = 2e-4


def permute_hidden(w, topo, perm):
    """The same function with its hidden units relabelled: W1's columns, W2's rows and B1 permuted."""
    I, H, O = topo
    a, b = I * H, I * H + H * O
    w = np.asarray(w)
    return np.concatenate([w[:a].reshape(I, H)[:, perm].ravel(), w[a:b].reshape(H, O)[perm].ravel(), w[b:b + H][perm], w[b + H:]])


def outputs(task, topo, test, W):
    """The float64 oracle's outputs of the vectors W [U, P] on the test rows -> [U, n_rows * n_out]."""
    from test_gpu_predict import _outputs
    return _outputs(task, test[:, :topo[0]], W.T.astype(np.float64), topo).reshape(len(W), -1)


def rms(F):
    return np.sqrt(((F[:, None, :] - F[None, :, :]) ** 2).mean(axis=2))


@functools.lru_cache(maxsize=None)
def planted(topo):
    """(task, train, test, W [U, P] float32, mult [U], group [U], base [U] (the index of a permuted copy's base, else -1),
    separation, radius); shared, not to be written to."""
    from test_gpu_analysis_shapes import _vectors
    if topo == REG_TOPO:
        task = orc.TASK_REG
        train, test = uncertainty_cases.regression_case(topo)[:2]
    else:
        task = orc.TASK_CLS
        train, test = report_cases.case(topo)[:2]
    sep = SEPARATION[topo]
    cand = _vectors(topo, 6, 77, spread=2.0)
    d = rms(outputs(task, topo, test, cand))
    picked = [0]
    for k in range(1, len(cand)):
        if len(picked) < 3 and all(d[k, j] >= 4.4 * sep for j in picked):
            picked.append(k)
    assert len(picked) == 3, d
    rng = np.random.default_rng(5)
    rows, group, base = [], [], []
    for g, size in enumerate(SIZES):
        for _ in range(size):
            rows.append((cand[picked[g]].astype(np.float64) * (1.0 + NOISE * rng.standard_normal(cand.shape[1]))).astype(np.float32))
            group.append(g)
            base.append(-1)
    for _ in range(N_PERMUTED):
        rows.append(permute_hidden(rows[0], topo, rng.permutation(topo[1])).astype(np.float32))
        group.append(0)
        base.append(0)
    order = rng.permutation(len(rows))
    where = np.argsort(order)                                              # old index -> new index
    W = np.stack(rows)[order]
    group = np.asarray(group)[order]
    base = np.asarray([where[b] if b >= 0 else -1 for b in np.asarray(base)[order]])
    mult = rng.integers(1, 4, len(W)).astype(np.int32)
    for a in (W, mult, group, base):
        a.setflags(write=False)
    return task, train, test, W, mult, group, base, sep, sep / 2


def planted_labels(group, mult):
    """The labelling the analysis must return: the groups numbered by descending mass (no two are equal: asserted)."""
    mass = np.asarray([int(mult[group == g].sum()) for g in range(3)])
    assert len(set(mass)) == 3
    number = np.empty(3, np.int64)
    number[np.argsort(-mass)] = np.arange(3)
    return number[group], np.sort(mass)[::-1] / mass.sum()
