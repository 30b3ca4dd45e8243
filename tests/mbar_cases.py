"""The host-U cases of tests/test_gpu_mbar.py: a three-dimensional Gaussian ladder (rung k draws x ~ N(0, I / (1 + beta_k)), U =
-|x|^2 / 2; the prior state draws at beta = 0), at the smallest sizes at which the kernels of ptnn_dev_mbar.hpp take another path."""
import numpy as np

# name: (rungs, draws per rung, prior draws): K = rungs + 1 states
SIZES = {
    "K2_one_rung_and_prior": (1, 9, 6),            # the smallest ladder
    "K3_less_than_a_wave": (2, 5, 7),              # 5 draws per rung
    "K5_past_a_work_group": (4, 257, 40),          # 257 rows of a rung: one past a work-group, tail lanes
    "K65_past_a_gram_tile": (64, 70, 70),          # 65 states: one past a 64 x 64 Gram tile on both axes
}


def case(name, with_b, with_mult):
    """-> dict(betas [R], u [R, n], b [R, n] or None, multiplicity [R, n] int32 or None, u_prior [m], b_prior [m] or None)."""
    R, n, m = SIZES[name]
    rng = np.random.default_rng(1000 + R * 7 + n)
    betas = np.array([1.0]) if R == 1 else np.geomspace(0.02, 1.0, R)
    x = rng.standard_normal((R, n, 3)) / np.sqrt(1.0 + betas)[:, None, None]
    u = -0.5 * np.sum(x * x, axis=2)
    xp = rng.standard_normal((m, 3))
    up = -0.5 * np.sum(xp * xp, axis=1)
    mult = ((np.arange(R * n) * 7 + 3) % 4).astype(np.int32).reshape(R, n) if with_mult else None     # zeros included, >= 4 per rung
    return dict(betas=betas, u=u, b=u / 6.0 if with_b else None, multiplicity=mult, u_prior=up, b_prior=up / 6.0 if with_b else None)
