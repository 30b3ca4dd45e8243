"""Log evidence at every compiled shape (PTNN_SHAPES): a short run per (task, n_in, n_out), every rung draw's U and the first prior
draws' U against the float64 oracle."""
import warnings

import numpy as np
import pytest

import evidence_ref as ref
from parity import orc

pytestmark = pytest.mark.gpu

import __graft_entry__  # noqa: E402

SHAPES = list(__graft_entry__.SHAPES)


@pytest.mark.parametrize("task,n_in,n_out", SHAPES)
def test_evidence_every_shape(task, n_in, n_out, tmp_path):
    from ptnn_amd import philox
    rng = np.random.default_rng(100 * n_in + n_out)
    x = rng.random((40, n_in))
    y = rng.integers(0, n_out, 40).astype(np.float64) if task == orc.TASK_CLS else rng.random(40)
    data = np.column_stack([x, y])
    topo = (n_in, 5, n_out)
    R, S = 4, 60
    if task == orc.TASK_REG:
        from ptnn_amd.pt_timeseries_regression import ParallelTempering
        pt = ParallelTempering(False, 0.1, data, data, list(topo), R, 10, R * S, 5, 0.5, str(tmp_path), seed=7, write_files=False)
    else:
        from ptnn_amd.pt_classification import ParallelTempering
        pt = ParallelTempering(False, 0.1, data, data, list(topo), R, 10, R * S, 5, str(tmp_path), seed=7, write_files=False)
    pt.initialize_chains(0.2)
    pt.run_chains()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev = pt.log_evidence(prior_draws=256, return_draws=True)
    step0, end = int(S * 0.2), pt._pt_switch_step()
    betas = np.array([1.0 / float(np.float32(T)) for T in pt.temperatures])
    order = np.argsort(betas, kind="stable")
    W = pt._sampler.traces(step0, end - step0)["pos_w"][order]
    P = W.shape[2]
    U = np.concatenate(ev.u_draws)
    np.testing.assert_allclose(U, ref.u_and_b_batched(task, data, W.reshape(-1, P), topo)[0], rtol=1e-5, atol=1e-4)
    Wp = np.stack([philox.prior_weights(pt.seed, i, P, 5.0) for i in range(32)])
    np.testing.assert_allclose(ev.u_prior_draws[:32], ref.u_and_b_batched(task, data, Wp, topo)[0], rtol=1e-4, atol=1e-3)
    assert np.isfinite(ev.log_z_ss) and np.isfinite(ev.log_z_ti)
