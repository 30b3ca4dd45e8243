"""Posterior predictive checks (ptnn_ppc) at other compiled shapes: the draws, the reduction over the rows and the reduction over
the occurrences (checks 1-3 of tests/test_gpu_ppc.py) on a narrow classifier, the matrix-core classifier, the wide layout with
compact traces and a 5-input regression, from short runs."""
import numpy as np
import pytest

import parity
from parity import orc
from test_gpu_elpd import _pt
from test_gpu_ppc import LAGS, _low, _same, _targets, check_classification, check_regression

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,topo,R,S", [("iris", (4, 12, 3), 4, 200), ("ions", (34, 50, 2), 4, 120)])
def test_classifier_shapes(name, topo, R, S, tmp_path, monkeypatch):
    d = parity.datasets()
    tr, te = d[name + "_train"], d[name + "_test"]
    pt = _pt(orc.TASK_CLS, topo, tr, te, R, S, tmp_path, lr=0.01, maxtemp=10)
    res = pt.run_chains()
    for data, rows in (("train", tr), ("test", te)):
        out, _ = check_classification(pt, data, rows[:, topo[0]].astype(np.int64))
        assert out["n_samples"] == R * (S // 2)
    # blocks of distinct vectors, and the vectors as host input
    monkeypatch.setenv("PTNN_PPC_SCRATCH_BYTES", str(4 * len(te) * topo[2] * 3))
    _same(_low(pt, "test"), out)
    _same(_low(pt, "test", weights=res[0].T), out)


def test_wide_net_compact_traces(tmp_path, monkeypatch):
    d = parity.datasets()
    R, S, topo = 4, 300, (32, 96, 1)
    pt = _pt(orc.TASK_REG, topo, d["synth32_train"], d["synth32_test"], R, S, tmp_path)
    assert pt._sampler.describe()["compact_traces"] == 1
    pt.run_chains()
    # eta is recorded from a chain's first accepted step on: the selection starts behind the last chain's
    accepted = np.ascontiguousarray(pt._sampler.trace_rows()[:, :, 5]).view(np.int32) > 0
    assert accepted[:, -1].all()
    step0 = max(S // 2, int(np.argmax(accepted, axis=1).max()))
    print("selection from row", step0)
    sel = dict(burn_in=(step0 + 0.5) / S)
    eta = pt._sampler.eta_trace()[:, step0:].reshape(-1)
    w = pt._sampler.traces(step0, S - step0)["pos_w"].reshape(-1, pt.num_param)
    for data in ("train", "test"):
        out, _ = check_regression(pt, data, _targets(d["synth32_" + data], 32), eta, LAGS, **sel)
    _same(_low(pt, "test", lags=LAGS, weights=w, eta=eta), out)
    monkeypatch.setenv("PTNN_PPC_SCRATCH_BYTES", str(4 * len(d["synth32_test"]) * 5))
    _same(_low(pt, "test", lags=LAGS, **sel), out)


def test_five_input_regression(tmp_path):
    d = parity.datasets()
    R, S = 4, 200
    pt = _pt(orc.TASK_REG, (5, 7, 1), d["sunspot5_train"], d["sunspot5_test"], R, S, tmp_path)
    res = pt.run_chains()
    eta = pt._sampler.eta_trace()[:, S // 2:].reshape(-1)
    for data in ("train", "test"):
        out, _ = check_regression(pt, data, _targets(d["sunspot5_" + data], 5), eta, (1, 2, 50, 197))
    _same(_low(pt, "test", lags=(1, 2, 50, 197), weights=res[0].T, eta=eta), out)
