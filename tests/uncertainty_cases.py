"""The cases of the predictive uncertainty tests.  Classification: the grid of tests/report_cases.py (seven shapes, 53 test rows,
65 vectors, the float64 oracle's probabilities) with the multiplicities 0..3 the classification report's tests use.  Regression:
at the three compiled input widths the data and vectors of tests/test_gpu_analysis_shapes.py (`_data`, `_vectors`), eta from
uniform(-6, -3), the oracle's outputs.  No device."""
import functools

import numpy as np

import report_cases
from parity import orc

CLS_SHAPES, CLS_IDS = report_cases.SHAPES, report_cases.IDS
REG_SHAPES = [(4, 5, 1), (5, 256, 1), (32, 7, 1)]     # every compiled regression shape has one output
REG_IDS = ["-".join(map(str, t)) for t in REG_SHAPES]
MARGIN = report_cases.MARGIN            # the forward tolerance tests/test_gpu_analysis_shapes.py enforces
P_MIN = 0.03                            # no oracle probability of the grid lies below it (tests/test_uncertainty_cpu.py)
MI_MIN = 1e-3                           # no row's oracle mutual information lies below it


def multiplicities(n, seed=13):
    """n multiplicities in 0..3, entry 1 zero and entry 0 at least 1."""
    mult = np.random.default_rng(seed).integers(0, 4, n).astype(np.int32)
    mult[1], mult[0] = 0, max(mult[0], 1)
    return mult


@functools.lru_cache(maxsize=None)
def regression_case(topo):
    """(train, test, W [65, P] float32, eta [65] float32, oracle outputs [65, 53, O] float64); shared, not to be written to."""
    from test_gpu_analysis_shapes import _data, _vectors
    from test_gpu_predict import _outputs
    train, test = _data(orc.TASK_REG, topo, report_cases.DATA_SEED)
    W = _vectors(topo, report_cases.N_VECTORS, report_cases.VECTOR_SEED)
    eta = np.random.default_rng(14).uniform(-6.0, -3.0, len(W)).astype(np.float32)
    f = _outputs(orc.TASK_REG, test[:, :topo[0]], W.T.astype(np.float64), topo)
    for a in (train, test, W, eta, f):
        a.setflags(write=False)
    return train, test, W, eta, f
