"""Float64 oracle of ptnn_lfo and of the leave-future-out walk (Buerkner, Gabry & Vehtari 2020), in plain
numpy on top of elpd_ref.psis, which stays the single statement of the Pareto smoothing."""
import numpy as np

from elpd_ref import _logsumexp, psis


def lfo_rows(ll, n_fit, origins, block=1, multiplicity=None, r_eff=1.0):
    """Per origin i of the ordered rows of ll [n_samples, n_rows] (sample s counted multiplicity[s] times, conditioned on rows
    [0, n_fit)): C[s, j] = sum of ll[s, r] over r < j in ascending row order, lr = C[:, i] - C[:, n_fit],
    t = C[:, i + block] - C[:, i], elpd_lfo = logsumexp(psis(lr) + t) -> dict(elpd_lfo, khat, tail_len)."""
    ll = np.asarray(ll, np.float64)
    if multiplicity is not None:
        ll = np.repeat(ll, np.asarray(multiplicity, np.int64), axis=0)
    S, N = ll.shape
    C = np.concatenate([np.zeros((S, 1)), np.cumsum(ll, axis=1)], axis=1)
    og = np.asarray(origins, np.int64).reshape(-1)
    assert 0 < n_fit <= N and block >= 1 and np.all(og > 0) and np.all(og + block <= N)
    out = dict(elpd_lfo=np.empty(og.size), khat=np.empty(og.size), tail_len=np.empty(og.size, np.int64))
    for k, i in enumerate(og):
        lw, khat, T = psis(C[:, i] - C[:, n_fit], r_eff)
        out["elpd_lfo"][k] = _logsumexp(lw + (C[:, i + block] - C[:, i]))
        out["khat"][k] = khat
        out["tail_len"][k] = T
    return out


def walk_expected(origins, n_fit, khat_of, k_threshold, refit=True, max_refits=None):
    """What the walk must do, one origin at a time: origins >= n_fit ascending, then origins < n_fit descending, each side from
    the first fit; an origin other than the current fit whose khat_of(current fit, origin) is not <= the threshold (+inf included)
    becomes the new fit (while
    refits are allowed and left).  -> (fit_origin of every ascending distinct origin, refit origins in walk order)."""
    og = sorted({int(i) for i in origins})
    fit_of, refits = {}, []
    for order in ([i for i in og if i >= n_fit], [i for i in reversed(og) if i < n_fit]):
        fit = n_fit
        for i in order:
            if i != fit and not khat_of(fit, i) <= k_threshold and refit and (max_refits is None or len(refits) < max_refits):
                fit = i
                refits.append(i)
            fit_of[i] = fit
    return np.array([fit_of[i] for i in og], np.int64), refits
