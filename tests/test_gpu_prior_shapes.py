"""The prior predictive check at the other compiled shapes: the per-column results, saturation counts, function statistics,
counts and the independence of the block size (checks 2-6 of tests/test_gpu_prior.py) on a classification with three classes
and four scales, a two-class net with many inputs, the wide layout (H > 64: one vector per forward work-group) and a second
regression.  70 rows of parity.datasets() each, on the handle initialize_chains() makes."""
import numpy as np
import pytest

import parity
import prior_ref as ref
from parity import orc
from test_gpu_predict import _pt
from test_gpu_prior import N_DRAWS, N_ROWS, _run, check_blocks, check_columns, check_saturation, check_statistics

pytestmark = pytest.mark.gpu

# (task, topology, train rows (stacked where one set is short), scales, draws)
CASES = {
    "iris_4_12_3": (orc.TASK_CLS, (4, 12, 3), ("iris_train",), (0.25, 1.0, 4.0, 25.0), N_DRAWS),
    "ions_34_50_2": (orc.TASK_CLS, (34, 50, 2), ("ions_train",), (1.0, 25.0), N_DRAWS),
    "synth_32_96_1": (orc.TASK_REG, (32, 96, 1), ("synth32_train", "synth32_test"), (1.0, 25.0), 40),
    "sunspot5_5_7_1": (orc.TASK_REG, (5, 7, 1), ("sunspot5_train",), (1.0, 25.0), N_DRAWS),
}


@pytest.mark.parametrize("key", list(CASES))
def test_shape(key, tmp_path, monkeypatch):
    task, topo, sets, scales, n = CASES[key]
    d = parity.datasets()
    kw = dict(lr=0.01, maxtemp=10) if task == orc.TASK_CLS else {}
    pt = _pt(task, topo, d[sets[0]], d[sets[0].replace("train", "test")], 4, 20, tmp_path, **kw)
    x = np.ascontiguousarray(np.vstack([np.asarray(d[s]) for s in sets])[:N_ROWS, :topo[0] + 1], dtype=np.float32)
    assert x.shape == (N_ROWS, topo[0] + 1)
    res = _run(pt, x, scales, n=n)
    O = topo[2]
    assert res.sigma_squared == scales and res.mean.shape == (len(scales), N_ROWS, O) and res.samples.shape == (len(scales), n, N_ROWS, O)
    assert res.names == (list(ref.REG_STATS) if task == orc.TASK_REG else list(ref.CLS_FIXED) + [f"class_share[{k}]" for k in range(O)])
    check_columns(pt, x, res)
    check_saturation(res)
    check_statistics(pt, x, res)
    whole = check_blocks(pt, x, scales, monkeypatch, n=n)
    assert np.array_equal(whole["t_draw"], res.t_draw, equal_nan=True) and np.array_equal(whole["mean"], res.mean)
    if task == orc.TASK_CLS:
        shares = np.stack([res.t_draw[:, :, 4 + k] for k in range(O)], axis=-1)
        np.testing.assert_allclose(shares.sum(axis=-1), 1.0, rtol=1e-12)                 # every row has one argmax
        np.testing.assert_allclose(res.vote.sum(axis=-1), 1.0, rtol=1e-12)
