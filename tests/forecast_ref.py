"""Float64 oracle of ptnn_forecast: the recursion y_k = f_w(window_{k-1}) (+ exp(eta / 2) z_k),
window_k = (window_{k-1}[1:], y_k), written on the oracle's forward pass, with the noise drawn from philox.normals exactly as the
device's counter layout defines it."""
import numpy as np

import parity  # noqa: F401  (puts the oracle on sys.path)
from parity import orc
from ptnn_amd import philox


def noise_draws(horizon, i, r, seed):
    """z_k, k = 0 .. horizon - 1, of trajectory i at origin r: philox4x32_10(k >> 2, i, r, STREAM_FORECAST, seed), Box-Muller on
    (x0, x1) and (x2, x3), component k & 3."""
    return philox.normals(horizon, i, r, philox.STREAM_FORECAST, seed)


def end_window(rows, n_in):
    """The window right after the data: the last row's inputs shifted by one with its target appended (rows[-1, 1:n_in+1])."""
    rows = np.asarray(rows)
    return np.asarray(rows[-1, 1:n_in + 1], dtype=np.float64)


def trajectories(w, origins, horizon, topo, eta=None, seed=0, traj_index=None):
    """Forecast paths [n_vectors, n_origins, horizon] (float64) of the weight vectors w [n, P] from origin windows
    [n_origins, n_in]; with eta [n] each step adds exp(eta / 2) z_k of noise_draws(horizon, traj_index[v], r, seed) (traj_index
    defaults to 0 .. n - 1)."""
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    win0 = np.atleast_2d(np.asarray(origins, dtype=np.float64))[:, :topo[0]]
    n, R = w.shape[0], win0.shape[0]
    idx = np.arange(n) if traj_index is None else np.asarray(traj_index)
    out = np.empty((n, R, horizon))
    for v in range(n):
        win = win0.copy()
        z = None
        if eta is not None:
            sd = np.exp(0.5 * np.float64(np.float32(eta[v])))
            z = np.stack([noise_draws(horizon, int(idx[v]), r, seed) for r in range(R)])          # [R, horizon]
        for k in range(horizon):
            y = orc.forward(win, w[v], topo)[1][:, 0]
            if z is not None:
                y = y + sd * z[:, k]
            out[v, :, k] = y
            win = np.concatenate([win[:, 1:], y[:, None]], axis=1)
    return out


def teacher_windows(origin, path, k, n_in):
    """The window step k (0-based) of a trajectory reads: the origin's last n_in - k values followed by the path's first k
    outputs (the last n_in of them once k >= n_in).  origin [n_in], path [>= k]."""
    full = np.concatenate([np.asarray(origin, np.float64), np.asarray(path[:k], np.float64)])
    return full[k:k + n_in]
