"""Convergence diagnostics, host side (no GPU): known answers of the float64 oracle (tests/convergence_ref.py), a hand-worked
case, the degenerate cases, the exported entry point and its argument checks, which run before anything touches a device, and the
refusals of convergence_diagnostics."""
import ctypes as C
import math

import numpy as np
import pytest

import convergence_ref as cr


def _ar1(phi, C_, n, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((C_, n))
    y = np.empty((C_, n))
    y[:, 0] = e[:, 0] / math.sqrt(1 - phi * phi)
    for i in range(1, n):
        y[:, i] = phi * y[:, i - 1] + e[:, i]
    return y


def test_iid_normal():
    x = np.random.default_rng(1).standard_normal((4, 20000))
    r = cr.diagnose(x)
    assert abs(r["ess"] / 80000 - 1) < 0.1
    assert r["r_hat"] < 1.01


def test_ar1_positive():
    phi, N = 0.9, 4 * 20000
    r = cr.diagnose(_ar1(phi, 4, 20000, 2))
    assert abs(r["ess"] / (N * (1 - phi) / (1 + phi)) - 1) < 0.1


def test_ar1_negative_and_the_clamp():
    N = 4 * 20000
    r = cr.diagnose(_ar1(-0.5, 4, 20000, 3))
    assert r["ess"] > N
    assert r["ess"] < N * math.log10(N)                     # tau ~ 1/3 lies above the clamp 1 / log10(M h)
    r = cr.diagnose(_ar1(-0.95, 4, 20000, 4))               # tau ~ 0.026: the clamp decides
    assert r["ess"] == pytest.approx(N * math.log10(N), rel=1e-14)


def test_shifted_means():
    x = np.random.default_rng(5).standard_normal((4, 2000)) + np.arange(4)[:, None] * 0.5
    assert cr.diagnose(x)["r_hat"] > 1.1


def test_hand_worked_n5():
    """One chain of 5 draws: h = 2, the middle draw (100) dropped; M = 2 split chains [1, 3] and [2, 6]."""
    x = np.array([[1.0, 3.0, 100.0, 2.0, 6.0]])
    r = cr.diagnose(x)
    # split means 2 and 4; gamma_0 = (1 + 1) / 2 = 1 and (4 + 4) / 2 = 4; s^2 = 2 and 8: W = 5
    # var(means, ddof 1) = 2: var+ = 5 * 1/2 + 2 = 4.5; r_hat = sqrt(0.9)
    assert r["r_hat"] == pytest.approx(math.sqrt(4.5 / 5), rel=1e-15)
    # gamma_1 = (-1 * 1) / 2 = -0.5 and (-2 * 2) / 2 = -2: rho_1 = 1 - (5 + 1.25) / 4.5
    assert r["rho"][1] == pytest.approx(1 - 6.25 / 4.5, rel=1e-15)
    # h = 2 <= 4: no pair loop, max_t = -1, tau = -1 + 0 + rho[0] = 0 -> the clamp 1 / log10(4)
    assert r["trunc_lag"] == -1
    assert r["ess"] == pytest.approx(4 * math.log10(4), rel=1e-15)
    # pooled over all five draws, the middle one included
    assert r["mean"] == pytest.approx(22.4) and r["var"] == pytest.approx(np.var(x, ddof=1))


def test_n4_clamp():
    r = cr.diagnose(np.array([[0.0, 1.0, 0.5, 2.0], [1.0, 0.0, 3.0, 1.0]]))
    assert r["trunc_lag"] == -1 and r["ess"] == pytest.approx(8 * math.log10(8), rel=1e-15)


def test_degenerate():
    r = cr.diagnose(np.full((3, 10), 2.5))
    assert math.isnan(r["r_hat"]) and math.isnan(r["ess"]) and np.all(np.isnan(r["ess_chain"]))
    x = np.repeat(np.array([[1.0], [2.0], [4.0]]), 10, axis=1)          # every split chain constant, the chains differ
    r = cr.diagnose(x)
    assert r["r_hat"] == math.inf
    assert np.isfinite(r["ess"]) and r["ess"] > 0
    assert np.all(np.isnan(r["ess_chain"]))                           # one chain alone: var+ = 0


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def test_library_exports_convergence(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_convergence is not None and "ptnn_convergence" in _lib.SYMBOLS
    assert C.sizeof(_lib.ConvergenceSpec) > 0


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.ConvergenceSpec()
    s.struct_bytes = C.sizeof(_lib.ConvergenceSpec)
    s.thin, s.nsteps = 1, 10
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_convergence(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_convergence_rejects_bad_arguments_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    d = np.zeros(64, np.float32)
    dp = d.ctypes.data_as(C.POINTER(C.c_float))
    rho = np.zeros(8)
    rp = rho.ctypes.data_as(C.POINTER(C.c_double))
    cases = [
        (None, "null"),
        (_spec(struct_bytes=8), "struct_bytes"),
        (_spec(thin=0), "thin"),
        (_spec(replicas=np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), n_replicas=0), "n_replicas"),
        (_spec(params=np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), n_params=-1), "n_params"),
        (_spec(scalars=1 << _lib.TR_ACCEPT), "TR_ACCEPT"),
        (_spec(scalars=1 << _lib.TR_LOGALPHA), "scalars"),
        (_spec(scalars=(1 << _lib.TR_LIKEH) | (1 << _lib.TR_SRC)), "scalars"),
        (_spec(draws=dp, n_chains=0, n_draws=4, n_quantities=1), "n_chains"),
        (_spec(draws=dp, n_chains=1, n_draws=3, n_quantities=1), "n_draws"),
        (_spec(draws=dp, n_chains=1, n_draws=4, n_quantities=0), "n_quantities"),
        (_spec(n_lags=-1), "n_lags"),
        (_spec(n_lags=2), "rho is NULL"),
        (_spec(rho=rp), "n_lags = 0"),
    ]
    for spec, want in cases:
        rc, msg = _err(lib, spec)
        assert rc < 0 and want in msg, (want, msg)
    # consistent requests reach the handle check
    for spec in (_spec(), _spec(scalars=31), _spec(draws=dp, n_chains=2, n_draws=4, n_quantities=8)):
        rc, msg = _err(lib, spec)
        assert rc < 0 and "null handle" in msg


def test_convergence_diagnostics_refusals(pt, tmp_path):
    from ptnn_amd import _lib
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    data = np.random.default_rng(0).random((40, 5))
    p = ParallelTempering(True, 0.1, data, data, [4, 5, 1], 4, 2, 400, 10, 0.5, str(tmp_path), seed=1, write_files=False)
    with pytest.raises(ValueError, match="initialize_chains"):
        p.convergence_diagnostics()

    class Sharded:                        # stands in for a ladder sharded over several devices
        pass
    p._sampler = Sharded()
    with pytest.raises(ValueError, match="one GPU"):
        p.convergence_diagnostics(draws=np.zeros((2, 8, 1)))
    # a handle-shaped stand-in: the refusals below come before any call into it
    p._sampler = _lib.Sampler.__new__(_lib.Sampler)
    p._finished, p.burn_in = False, 0.5
    with pytest.raises(ValueError, match="finished run_chains"):
        p.convergence_diagnostics()
    p._finished = True
    with pytest.raises(ValueError, match="draws must be"):
        p.convergence_diagnostics(draws=np.zeros((8, 1)))
    with pytest.raises(ValueError, match="chains"):
        p.convergence_diagnostics(chains=[4])
    with pytest.raises(ValueError, match="params"):
        p.convergence_diagnostics(params=[p.num_param])
    with pytest.raises(ValueError, match="scalar 'acc_train'"):
        p.convergence_diagnostics(scalars=("acc_train",))
    with pytest.raises(ValueError, match="no quantity"):
        p.convergence_diagnostics(params=[], scalars=())
    p.label_swap = True
    with pytest.raises(ValueError, match="label_swap"):
        p.convergence_diagnostics()
    p.label_swap = False
    p.trace_capacity = 16
    with pytest.raises(ValueError, match="trace_capacity"):
        p.convergence_diagnostics()
    p._sampler = None
