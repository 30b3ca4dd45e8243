"""float64 oracle of the posterior predictive checks (ptnn_ppc / predictive_check): the statistics of
include/ptnn.h restated from given network outputs f / p, eta, targets and draws, the draws themselves from philox.py (stream
STREAM_PPC), and the reduction over the occurrences.  No GPU, no forward pass: the tests feed it the device's own outputs."""
import numpy as np

from ptnn_amd import philox

REG_FIXED = ("mean", "sd", "min", "max", "chi2", "max_abs_resid", "ljung_box")
CLS_FIXED = ("deviance", "accuracy")


def normals(seed, i, n_rows):
    """z[i, :]: component n % 4 of philox4x32_10(n / 4, i, 0, STREAM_PPC, seed), Box-Muller on (x0, x1) and (x2, x3)."""
    return philox.normals(n_rows, i, 0, philox.STREAM_PPC, seed)


def uniforms(seed, i, n_rows):
    """u[i, :]: uniform23 of component n % 4 of philox4x32_10(n / 4, i, 0, STREAM_PPC, seed); exact in float32."""
    x = philox.philox4x32(np.arange((n_rows + 3) // 4), i, 0, philox.STREAM_PPC, seed)
    return philox.uniform23(np.stack(x, axis=-1).reshape(-1)[:n_rows])


def acf(v, k):
    d = np.asarray(v, np.float64) - np.mean(v)
    return float(np.sum(d[k:] * d[:len(d) - k]) / np.sum(d * d))


def level_stats(v):
    v = np.asarray(v, np.float64)
    return [float(np.mean(v)), float(np.std(v)), float(np.min(v)), float(np.max(v))]


def resid_stats(e, lags):
    e = np.asarray(e, np.float64)
    N = len(e)
    r = [acf(e, k) for k in lags]
    lb = N * (N + 2) * sum(rk * rk / (N - k) for rk, k in zip(r, lags))
    return [float(np.sum(e * e)), float(np.max(np.abs(e))), float(lb)] + r


def regression(f, eta, y, z, lags):
    """T of every occurrence: f [M, N] outputs, eta [M], targets y [N], draws z [M, N] -> (t_obs, t_rep) [M, 7 + len(lags)]."""
    f, z, y = np.asarray(f, np.float64), np.asarray(z, np.float64), np.asarray(y, np.float64)
    tau = np.exp(0.5 * np.asarray(eta, np.float64))
    t_obs, t_rep = [], []
    for i in range(f.shape[0]):
        t_obs.append(level_stats(y) + resid_stats((y - f[i]) / tau[i], lags))
        t_rep.append(level_stats(f[i] + tau[i] * z[i]) + resid_stats(z[i], lags))
    return np.array(t_obs), np.array(t_rep)


def draw_classes(p, u):
    """p [N, O] class probabilities, u [N] -> the smallest class k with sum_{j<=k} p_j > u sum_j p_j, else the last class."""
    p = np.asarray(p, np.float64)
    cum = np.cumsum(p, axis=1)                               # sequential in class order
    hit = cum > (np.asarray(u, np.float64) * cum[:, -1])[:, None]
    return np.where(hit.any(axis=1), np.argmax(hit, axis=1), p.shape[1] - 1).astype(np.int64)


def class_stats(p, label):
    p = np.asarray(p, np.float64)
    label = np.asarray(label, np.int64)
    with np.errstate(divide="ignore"):
        dev = -2.0 * float(np.sum(np.log(p[np.arange(len(label)), label])))
    acc = float(np.mean(np.argmax(p, axis=1) == label))
    return [dev, acc] + [float(np.sum(label == k)) for k in range(p.shape[1])]


def classification(p, y, u):
    """p [M, N, O], labels y [N], uniforms u [M, N] -> (t_obs, t_rep) [M, 2 + O], y_rep [M, N]."""
    t_obs, t_rep, y_rep = [], [], []
    for i in range(len(p)):
        lab = draw_classes(p[i], u[i])
        y_rep.append(lab)
        t_obs.append(class_stats(p[i], y))
        t_rep.append(class_stats(p[i], lab))
    return np.array(t_obs), np.array(t_rep), np.array(y_rep)


def reduce(t_obs, t_rep):
    """The reduction over the occurrences, per statistic; an occurrence with a non-finite T on either side is left out."""
    t_obs, t_rep = np.asarray(t_obs, np.float64), np.asarray(t_rep, np.float64)
    out = {k: [] for k in ("n_defined", "n_greater", "n_equal", "mean_obs", "mean_rep", "var_rep", "p_value")}
    for j in range(t_obs.shape[1]):
        ok = np.isfinite(t_obs[:, j]) & np.isfinite(t_rep[:, j])
        o, r = t_obs[ok, j], t_rep[ok, j]
        nd, ng, ne = int(ok.sum()), int(np.sum(r > o)), int(np.sum(r == o))
        out["n_defined"].append(nd); out["n_greater"].append(ng); out["n_equal"].append(ne)
        out["mean_obs"].append(np.mean(o) if nd else np.nan); out["mean_rep"].append(np.mean(r) if nd else np.nan)
        out["var_rep"].append(np.var(r) if nd else np.nan)
        out["p_value"].append((ng + 0.5 * ne) / nd if nd else np.nan)
    return {k: np.array(v) for k, v in out.items()}


def check_regression(f, eta, counts, y, lags, seed):
    """The whole check of distinct outputs f [U, N] with eta [U] and multiplicities counts [U] -> (names, reduce() dict)."""
    rep = np.repeat(np.arange(len(counts)), counts)
    z = np.stack([normals(seed, i, len(y)) for i in range(len(rep))])
    t_obs, t_rep = regression(np.asarray(f)[rep], np.asarray(eta)[rep], y, z, lags)
    return list(REG_FIXED) + [f"resid_acf[{k}]" for k in lags], reduce(t_obs, t_rep)


# The known-answer pair (tests/test_ppc_cpu.py, tests/test_gpu_ppc.py): one vector with constant output repeated KNOWN_M times on
# KNOWN_N rows, targets y = f + tau * noise.  "iid": independent standard normals -- the model is right; "ar1": a stationary AR(1)
# series of unit variance with rho = 0.8 -- the marginal distribution is the model's, the independence is not.
KNOWN_M, KNOWN_N, KNOWN_ETA, KNOWN_RHO = 2000, 300, -3.0, 0.8
KNOWN_NOISE_SEED = {"iid": 105, "ar1": 202}          # numpy default_rng seeds of the noise (chosen: see test_ppc_cpu.py)
KNOWN_DRAW_SEED = 20260101                            # Philox key of the replicates
KNOWN_LAGS = (1, 2, 3, 4, 5)


def known_noise(case):
    g = np.random.default_rng(KNOWN_NOISE_SEED[case]).standard_normal(KNOWN_N)
    if case == "iid":
        return g
    v = np.empty(KNOWN_N)
    v[0] = g[0]
    for n in range(1, KNOWN_N):
        v[n] = KNOWN_RHO * v[n - 1] + np.sqrt(1.0 - KNOWN_RHO ** 2) * g[n]
    return v
