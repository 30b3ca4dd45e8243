"""Power-scaling sensitivity (ptnn_powerscale) at every compiled shape of PTNN_SHAPES: one small call per (task, n_in, n_out),
host vectors through weights= (no sampling run), each against the float64 oracle; 32-96-1 and 34-50-2, where the weights
dominate the quantities, among them."""
import numpy as np
import pytest

from parity import orc
from test_gpu_analysis_shapes import _make, _vectors
from test_gpu_powerscale import _low, _same, check_oracle

pytestmark = pytest.mark.gpu

REG, CLS = orc.TASK_REG, orc.TASK_CLS
CASES = [(REG, (4, 5, 1)), (REG, (5, 7, 1)), (REG, (32, 96, 1)), (CLS, (4, 12, 3)), (CLS, (34, 50, 2)), (CLS, (9, 6, 2)),
         (CLS, (11, 8, 10)), (CLS, (20, 6, 2)), (CLS, (16, 8, 10)), (CLS, (6, 7, 18))]


def test_cases_cover_every_compiled_shape():
    import __graft_entry__ as g
    assert sorted({(t, topo[0], topo[2]) for t, topo in CASES}) == sorted(g.SHAPES)


@pytest.mark.parametrize("task,topo", CASES, ids=[f"{'cls' if t else 'reg'}-{i}-{h}-{o}" for t, (i, h, o) in CASES])
def test_against_the_oracle(task, topo, tmp_path, monkeypatch):
    pt, train, test = _make(task, topo, tmp_path, seed=sum(topo))
    U = 150
    w = _vectors(topo, U, seed=7 + topo[1], spread=0.2)
    rng = np.random.default_rng(topo[0])
    c = rng.integers(1, 4, U).astype(np.int32)
    e = rng.normal(-3.0, 0.3, U).astype(np.float32) if task == REG else None
    out = _low(pt, "test", weights=(w, c), eta=e)
    check_oracle(pt, "test", w, e, c, out)
    own = np.repeat(np.arange(U), c)
    _same(_low(pt, "test", weights=w[own], eta=None if e is None else e[own]), out)
    monkeypatch.setenv("PTNN_POWERSCALE_SCRATCH_BYTES", str((8 * 256 + 4 * U) * 5))
    _same(_low(pt, "test", weights=(w, c), eta=e), out)
