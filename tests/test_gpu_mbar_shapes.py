"""MBAR at every compiled shape (PTNN_SHAPES): a short run per (task, n_in, n_out), a finite log Z, weights that sum to 1, and
resampled vectors that posterior_predictive accepts."""
import warnings

import numpy as np
import pytest

from parity import orc

pytestmark = pytest.mark.gpu

import __graft_entry__  # noqa: E402

SHAPES = list(__graft_entry__.SHAPES)


@pytest.mark.parametrize("task,n_in,n_out", SHAPES)
def test_mbar_every_shape(task, n_in, n_out, tmp_path):
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
        rw = pt.rung_reweighting(prior_draws=256, resample=16)
    assert np.isfinite(rw.log_z_mbar) and np.isfinite(rw.se_log_z_mbar) and np.all(np.isfinite(rw.free_energy))
    assert rw.log_weights.shape == (R, pt._pt_switch_step() - int(S * 0.2)) and rw.prior_log_weights.shape == (256,)
    assert np.exp(rw.log_weights).sum() + np.exp(rw.prior_log_weights).sum() == pytest.approx(1.0, abs=1e-9)
    assert rw.vectors.shape == (16, pt.num_param) and (rw.eta is None) == (task == orc.TASK_CLS)
    pp = pt.posterior_predictive("test", weights=rw.vectors)
    assert pp.n_samples == 16 and np.all(np.isfinite(pp.mean))
