"""Coalition values (ptnn_coalition_values) on the GPU at every compiled shape: shapley_forward_kernel<TASK, I, O> against the
float64 reference under the derived bound of tests/shapley_ref.py, with single-coalition identity tables so that every value
v[n, S, o] is looked at on its own.

Per case: 3 explained rows; 5 vectors, two of them equal (4 distinct); the masks empty, full, alternating bits, the top bit only
and one random; B = 1, 3 (idle lanes), 64 (one full chunk), 65 (the chunk seam) and 130 (three chunks) background rows.  Every
case prints its worst err / bound."""
import os
import re

import numpy as np
import pytest

import shapley_ref as ref
from parity import orc
from test_gpu_analysis_shapes import _make, _vectors

pytestmark = pytest.mark.gpu

REG, CLS = orc.TASK_REG, orc.TASK_CLS
SHAPES = [(REG, 4, 1), (REG, 5, 1), (REG, 32, 1), (CLS, 4, 3), (CLS, 34, 2), (CLS, 9, 2), (CLS, 11, 10), (CLS, 20, 2), (CLS, 16, 10), (CLS, 6, 18)]
CASES = [(t, (i, h, o)) for t, i, o in SHAPES for h in (1, 5, 13)] + [(REG, (32, 70, 1))]
BACKGROUNDS = (1, 3, 64, 65, 130)


def masks_of(I, rng):
    full = (1 << I) - 1
    return np.array([0, full, 0x5555555555555555 & full, 1 << (I - 1), int(rng.integers(1, full))], np.uint64)


def test_cases_are_the_compiled_shapes():
    hpp = open(os.path.join(os.path.dirname(__file__), "..", "parallel-tempering-neural-net_amd", "csrc", "ptnn_shapes.hpp")).read()
    line = re.search(r"^#define PTNN_SHAPES\(X\)(.*)$", hpp, re.M).group(1)
    assert {tuple(map(int, m)) for m in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", line)} == set(SHAPES)
    for shape in SHAPES:
        assert {topo[1] for t, topo in CASES if (t, topo[0], topo[2]) == shape} >= {1, 5, 13}


@pytest.mark.parametrize("task,topo", CASES, ids=[f"{'cls' if t else 'reg'}-{i}-{h}-{o}" for t, (i, h, o) in CASES])
def test_values_at_every_compiled_shape(task, topo, tmp_path):
    I, H, O = topo
    seed = I * 1000 + H * 10 + O
    pt, train, test = _make(task, topo, tmp_path, seed)
    rng = np.random.default_rng(seed + 1)
    Wd = _vectors(topo, 4, seed + 2)
    W = Wd[[0, 1, 1, 2, 3]]                                             # two equal neighbours: one distinct vector, counted twice
    X32 = test[:3, :I].astype(np.float32)
    masks = masks_of(I, rng)
    coef = np.eye(5)
    worst = 0.0
    for B in BACKGROUNDS:
        bg32 = train[:B, :I].astype(np.float32)
        out = pt._sampler.coalition_values(X32, background=bg32, masks=masks, coef=coef, w=W, samples=True)
        s = out["samples"]
        assert s.shape == (5, 3, O, 5) and out["n_samples"] == 5 and out["n_distinct"] == 4
        assert np.array_equal(s[1], s[2])
        for k, u in enumerate((0, 1, 3, 4)):
            bound, want = ref.error_bound(X32, bg32, Wd[k], topo, task, masks, coef)
            err = np.abs(s[u].astype(np.float64) - want)
            ratio = float(np.max(err / bound))
            worst = max(worst, ratio)
            assert np.all(err <= bound), (B, k, ratio)
        if task == CLS:
            assert np.max(np.abs(s.astype(np.float64).sum(axis=2) - 1.0)) <= 1e-6
        # the full coalition is the net's own output on the row, whatever the background: the same bits for every B (a partial
        # sum k f of equal fp32 values has at most 33 bits, so the double sums and the division by B are exact)
        if B == BACKGROUNDS[0]:
            own = s[:, :, :, 1].copy()
        else:
            assert np.array_equal(s[:, :, :, 1], own)
    print(f"coalition values {'cls' if task else 'reg'}-{I}-{H}-{O}: worst err / bound = {worst:.4f}")
