"""The per-shape forward kernels of the analysis calls (csrc/ptnn_dev_{predict,sensitivity,pd,shapley,ale,forecast}.hpp) held BIT
FOR BIT, at every compiled shape, to digests recorded before their common pieces were gathered into csrc/ptnn_dev_net.hpp
(tests/golden/forward_bits_parent.json, written by `profiles/tools/record_analysis_bits.py forward` with the library of the commit
before that change): the shared pieces may change how the source reads, never an operation, its order, a barrier or an LDS address.

A case is a (task, n_in, n_out) of PTNN_SHAPES at one of the three hidden widths test_gpu_analysis_shapes.OUTPUT_CASES lists for
it: H < 4 (waves without a hidden unit), the problem table's H, and a wide H where NV drops to 1 or 2 and the LDS request is
largest.  65 data rows (one full 64-row tile and one with a single live lane) and 17 distinct host-given vectors -- more than every
*_MAX_NV, so every kernel runs at least two vector groups, the last ragged -- with multiplicities 0 .. 3, one of them 0.  Per case
one call each of predict, sensitivity, partial_dependence (inputs 0 and I - 1, 18 grid values: more than one grid tile at every
n_out, the last ragged), coalition_values (65 background rows: two lane chunks), accumulated_effects (first-order terms on inputs
0 and I - 1 and the pair (0, I - 1), then the pair (I - 1, 0) in a call of its own -- one call refuses a pair given in both
orders -- on the edited rows of test_gpu_ale._design) and, on the regression shapes, forecast (horizon 6, noise off).  The golden
file holds one SHA-256 per output of every call, over the output's dtype, shape and bytes, and the digest of each case's inputs.
predict's samples are also held to the float64 oracle at
test_outputs_at_every_compiled_shape's bound, so a golden recorded from a broken build fails here on its own account; the other
calls are held to float64 at these shapes by their own test files."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import parity
from parity import orc
from test_gpu_ale import _design
from test_gpu_analysis_shapes import OUTPUT_CASES, _data, _vectors
from test_gpu_predict import _outputs, _pt
from test_gpu_shapley_shapes import masks_of

pytestmark = pytest.mark.gpu

GOLDEN_FILE = "forward_bits_parent.json"
REG, CLS = orc.TASK_REG, orc.TASK_CLS
N_ROWS, N_VECTORS, N_GRID, N_TERMS, HORIZON = 65, 17, 18, 4, 6


def _first_three():
    """The first three rows OUTPUT_CASES lists per (task, n_in, n_out)."""
    seen, cases = {}, []
    for task, topo in OUTPUT_CASES:
        shape = (task, topo[0], topo[2])
        seen[shape] = seen.get(shape, 0) + 1
        if seen[shape] <= 3:
            cases.append((task, topo))
    return cases


CASES = _first_three()


def case_id(task, topo):
    return f"{'cls' if task else 'reg'}-{topo[0]}-{topo[1]}-{topo[2]}"


def test_cases_are_three_widths_of_every_compiled_shape():
    hpp = open(os.path.join(os.path.dirname(__file__), "..", "parallel-tempering-neural-net_amd", "csrc", "ptnn_shapes.hpp")).read()
    line = re.search(r"^#define PTNN_SHAPES\(X\)(.*)$", hpp, re.M).group(1)
    shapes = {tuple(map(int, m)) for m in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", line)}
    assert {(t, topo[0], topo[2]) for t, topo in CASES} == shapes and len(CASES) == 3 * len(shapes)
    for shape in shapes:
        hs = [topo[1] for t, topo in CASES if (t, topo[0], topo[2]) == shape]
        assert hs[0] < 4 and hs[2] > 64, shape


def inputs_of(task, topo):
    """(train rows [65, I + 1], distinct vectors [17, P] fp32, eta [17] fp32 or None, multiplicities [17] in 0 .. 3, one of them 0)."""
    I, H, O = topo
    seed = I * 1000 + H * 10 + O
    train, _ = _data(task, topo, seed, n_tr=N_ROWS, n_te=N_ROWS)
    w = _vectors(topo, N_VECTORS, seed + 1)
    rng = np.random.default_rng(seed + 2)
    mult = rng.integers(0, 4, N_VECTORS).astype(np.int32)
    mult[1] = 0
    mult[0] = max(mult[0], 1)
    eta = rng.normal(-3.0, 0.3, N_VECTORS).astype(np.float32) if task == REG else None
    return train, w, eta, mult


def run_calls(pt, task, topo):
    """{call: the binding's whole result} of one case."""
    I, H, O = topo
    s = pt._sampler
    train, w, eta, mult = inputs_of(task, topo)
    M = int(mult.sum())
    ranks = (0, M // 2, M - 1)
    src = dict(w=w, multiplicity=mult, ranks=ranks, samples=True)
    X32 = train[:, :I].astype(np.float32)
    ends = [0, I - 1]
    grid = np.percentile(X32.astype(np.float64), np.linspace(5, 95, N_GRID), axis=0).T.astype(np.float32)[ends]     # [2, N_GRID]
    rng = np.random.default_rng(I * 1000 + H * 10 + O + 3)
    masks = masks_of(I, rng)
    coef = rng.normal(0.0, 1.0, (masks.size, N_TERMS))
    # the edited rows and the pair edges of test_gpu_ale's design: (u of I - 1, v of 0); first-order edges by its recipe
    Xd, _, _, _, _, pair_edges = _design(X32, I, O)
    u, v = pair_edges[0]
    edges = np.stack([np.percentile(Xd[:, j].astype(np.float64), [10, 40, 70, 90]).astype(np.float32) for j in ends])
    out = {}
    out["predict"] = s.predict("train", vote=task == CLS, **src)
    out["sensitivity"] = s.sensitivity("train", ranks2=ranks, sample_abs=True, **src)
    out["partial_dependence"] = s.partial_dependence("train", inputs=ends, grid=grid, ranks2=ranks, ice_mean=True, sample_pd=True,
                                                     sample_range=True, **src)
    out["coalition_values"] = s.coalition_values("train", background=X32, masks=masks, coef=coef, ranks2=ranks, counts=True,
                                                 sample_abs=True, **src)
    ale = dict(ranks2=ranks, local_mean=True, sample_ale=True, sample_range=True, sample_ale2=True, sample_inter=True, **src)
    out["accumulated_effects"] = s.accumulated_effects(Xd, inputs=ends, edges=edges, pairs=[(0, I - 1)], edges2=np.stack([v, u])[None], **ale)
    out["accumulated_effects_swapped"] = s.accumulated_effects(Xd, pairs=[(I - 1, 0)], edges2=np.stack([u, v])[None], **ale)
    if task == REG:
        out["forecast"] = s.forecast(HORIZON, "train", eta=eta, noise=False, **src)
    return out


def sha(*arrays):
    """SHA-256 over the dtype, shape and bytes of every array that is not None."""
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def digests(task, topo, out):
    """What the golden file holds of a case: {"inputs": digest, "<call>.<output>": digest}; an output not produced is left out."""
    d = {"inputs": sha(*inputs_of(task, topo))}
    for call, res in out.items():
        for name, v in res.items():
            if v is not None:
                d[f"{call}.{name}"] = sha(np.asarray(v))
    return d


def record():
    """Everything the golden file holds: {case id: digests}."""
    import tempfile
    rec = {}
    for task, topo in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            rec[case_id(task, topo)] = digests(task, topo, run_calls(_handle(task, topo, tmp), task, topo))
    return rec


def _handle(task, topo, tmp_path):
    train = inputs_of(task, topo)[0]
    kw = dict(lr=0.01, maxtemp=10) if task == CLS else {}
    return _pt(task, topo, train, train, 4, 20, tmp_path, **kw)          # no run: every sample is host-given


_GOLDEN = {}


def golden():
    if not _GOLDEN:
        _GOLDEN.update(json.load(open(os.path.join(parity.GOLDEN, GOLDEN_FILE))))
    return _GOLDEN


@pytest.mark.parametrize("task,topo", CASES, ids=[case_id(t, topo) for t, topo in CASES])
def test_forward_outputs_equal_the_parent_commit(task, topo, tmp_path):
    I, H, O = topo
    out = run_calls(_handle(task, topo, tmp_path), task, topo)
    train, w, _, mult = inputs_of(task, topo)
    # predict's samples against the float64 oracle (test_outputs_at_every_compiled_shape's bound)
    want = np.repeat(_outputs(task, train[:, :I], w.T.astype(np.float64), topo), mult, axis=0)
    assert out["predict"]["samples"].shape == want.shape
    assert np.max(np.abs(out["predict"]["samples"] - want)) <= 1e-5
    got, rec = digests(task, topo, out), golden()[case_id(task, topo)]
    assert got["inputs"] == rec["inputs"], "the inputs are not the recorded ones"
    differ = sorted(k for k in got if k in rec and got[k] != rec[k])
    assert not differ, f"outputs whose bits differ from the recording: {differ}"
    assert sorted(got) == sorted(rec), "the outputs are not the recorded set"
