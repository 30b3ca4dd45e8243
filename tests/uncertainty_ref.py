"""Float64 numpy restatement of predictive uncertainty (include/ptnn.h: ptnn_uncertainty), on EXPANDED samples:
class probabilities p [S, N, K] or regression outputs f [S, N, O] with eta [S], one entry per selected sample, repeats included.
No device, no sharing of code with the package under test."""
import math

import numpy as np


def _mean0(x):
    """The mean over the first axis, accumulated in extended precision: the reference's own summation error stays far below the
    bounds it is used to check."""
    return (np.sum(np.asarray(x, dtype=np.longdouble), axis=0) / np.longdouble(len(x))).astype(np.float64)


def sample_entropy(p):
    """H_s[n] = -sum_k p log p per sample and row, natural log, 0 log 0 = 0, the terms added in class order -> [S, N] float64."""
    p = np.asarray(p, dtype=np.float64)
    h = np.zeros(p.shape[:-1])
    for k in range(p.shape[-1]):
        pk = p[..., k]
        with np.errstate(divide="ignore", invalid="ignore"):
            h = h + np.where(pk > 0.0, pk * np.log(pk), 0.0)
    return 0.0 - h


def entropy(p):
    """The same of any array of distributions over the last axis."""
    return sample_entropy(p)


def classification(p, vote=None):
    """Every classification quantity from expanded probabilities p [S, N, K].  A sample's term of the expected entropy is
    H_s / log K clamped to [0, 1], as the definition has it: fp32 probabilities may sum to a little over 1 and carry H_s an
    fp32 rounding above log K; the entropy of the pooled prediction is held to log K in the same way."""
    p = np.asarray(p, dtype=np.float64)
    S, N, K = p.shape
    H = sample_entropy(p)
    p_mean = _mean0(p)
    total = np.minimum(entropy(p_mean), math.log(K))
    aleatoric = _mean0(np.minimum(H, math.log(K))) if K > 1 else np.zeros(N)
    if vote is None:
        best = np.argmax(p, axis=2)                                     # first index on a tie
        vote = np.stack([(best == k).sum(axis=0) for k in range(K)], axis=1) / float(S)
    return dict(H=H, p_mean=p_mean, vote=vote, total=total, aleatoric=aleatoric, epistemic=np.maximum(total - aleatoric, 0.0),
                confidence=p_mean.max(axis=1), variation_ratio=1.0 - vote.max(axis=1), disagreement=1.0 - (vote * vote).sum(axis=1))


def mean_kl(p):
    """The mean over the samples of KL(p_s || p_mean) per row -> [N] float64 (the mutual information, computed the other way)."""
    p = np.asarray(p, dtype=np.float64)
    pm = p.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0.0, p * (np.log(p) - np.log(pm)[None]), 0.0)
    return t.sum(axis=2).mean(axis=0)


def regression(f, eta, centre=None):
    """Every regression quantity from expanded outputs f [S, N, O] and eta [S]; `centre` [N, O]: the mean the squares are taken
    around (None = the float64 mean of f)."""
    f = np.asarray(f, dtype=np.float64)
    mean = _mean0(f)
    c = mean if centre is None else np.asarray(centre, dtype=np.float64)
    ev = _mean0((f - c[None]) ** 2)
    av = float(_mean0(np.exp(np.asarray(eta, dtype=np.float32).astype(np.float64))))
    return dict(pred_mean=mean, epistemic_var=ev, aleatoric_var=av, total_var=ev + av, epistemic_share=ev / (ev + av),
                sd=np.sqrt(_mean0((f - mean[None]) ** 2)))


def risk_coverage(score, loss):
    """Brute force: the rows in ascending score, ties in row order; risk[j] = the mean loss of the first j + 1."""
    score, loss = [float(v) for v in score], [float(v) for v in loss]
    N = len(score)

    def curve(key):
        order = sorted(range(N), key=lambda i: (key[i], i))
        return [sum(loss[i] for i in order[:j + 1]) / (j + 1) for j in range(N)]
    risk, best = curve(score), curve(loss)
    aurc, opt = sum(risk) / N, sum(best) / N
    return dict(coverage=[(j + 1) / N for j in range(N)], risk=risk, aurc=aurc, aurc_optimal=opt, e_aurc=aurc - opt)


def more_uncertain(a, b):
    """P(a row of b has a larger score than a row of a), ties half, over all pairs."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((b[None, :] > a[:, None]).sum() + 0.5 * (b[None, :] == a[:, None]).sum()) / (a.size * b.size))
