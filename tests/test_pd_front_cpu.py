"""The Python front of partial_dependence (no GPU), on the two drop-in classes of tests/test_analysis_front_cpu.py with its
recording stand-in for `_lib.Sampler`, taught the one call more: valid calls over every sample source and rows argument, the
arguments the sampler receives, what comes back, every refusal and the order of the checks, and the object states (no handle, a
sharded ladder, label_swap, a streamed trace, an unfinished run).  The last test asserts that the cases reach every `raise` of
effects.py."""
import ast
import inspect
import sys

import numpy as np
import pytest

import test_analysis_front_cpu as front
from test_analysis_front_cpu import BAD_ROWS, BAD_W, CLS_ROWS, MANY_PCTS, MULT, REG_P, REG_ROWS, STATES, TRACE_FAULTS, W, WC, fill

from ptnn_amd import effects, parallel_tempering as pt_module  # noqa: E402


class PdStandIn(front.StandIn):
    def partial_dependence(self, *args, **kw):
        self._log("partial_dependence", args, kw)
        n, O, M = self._n_rows(args[0]), self.O, self._count(kw)
        A, G = np.asarray(kw["grid"]).shape
        k, k2 = len(kw["ranks"]), len(kw["ranks2"])
        sr = fill((M, A, O), 6, dtype=np.float32)
        return dict(ice_mean=fill((n, A, G, O), 1) if kw["ice_mean"] else None,
                    ice_order_stats=fill((k, n, A, G, O), 2, dtype=np.float32) if k else None, pd_mean=fill((A, G, O), 3),
                    pd_order_stats=fill((k2, A, G, O), 4, dtype=np.float32) if k2 else None, range_mean=fill((A, O), 5),
                    range_order_stats=fill((k2, A, O), 7, dtype=np.float32) if k2 else None,
                    sample_pd=fill((M, A, G, O), 8, dtype=np.float32) if kw["sample_pd"] else None,
                    sample_range=sr if kw["sample_range"] else None,
                    samples=fill((M, n, A, G, O), 9, dtype=np.float32) if kw["samples"] else None, n_samples=M, n_distinct=-(-M // 2))


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(PdStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.partial_dependence(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).partial_dependence(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


# ---- valid calls
TRACE = [("all", {}, dict(replicas=None, step0=10, nsteps=30, thin=1), 120),
         ("cold_thin", dict(chains="cold", thin=3), dict(replicas=[1], step0=10, nsteps=30, thin=3), 10),
         ("list_burn_in", dict(chains=[2, 0], burn_in=0.5, thin=2), dict(replicas=[2, 0], step0=20, nsteps=20, thin=2), 20),
         ("burn_in_zero", dict(burn_in=0), dict(replicas=None, step0=0, nsteps=40, thin=1), 160)]


@pytest.mark.parametrize("name, kw, source, M", TRACE, ids=[t[0] for t in TRACE])
def test_trace_sources(name, kw, source, M):
    pt, calls, pd = run("reg", **kw)
    (tag, fn, args, got), = calls
    assert (tag, fn, args) == ("self", "partial_dependence", ["train"])
    want = dict(source, inputs=np.arange(4, dtype=np.int32), ranks=[], ice_mean=False, sample_pd=True, sample_range=True, samples=False)
    spots, ranks = pt._band_ranks(M, [5, 95])
    want.update(ranks2=ranks, grid=effects.pd_grid(np.asarray(pt.traindata)[:, :4], None, 16, (5, 95))[1])
    assert got == front.enc(want)
    assert pd.n_samples == M and pd.n_distinct == -(-M // 2)
    assert pd.inputs.dtype == np.int64 and pd.inputs.tolist() == [0, 1, 2, 3]
    assert pd.grid.dtype == np.float64 and np.array_equal(pd.grid, want["grid"].astype(np.float64))
    assert np.array_equal(pd.pd_mean, fill((4, 16, 1), 3)) and np.array_equal(pd.effect_range, fill((4, 1), 5))
    assert pd.ice_mean is None and pd.ice_percentiles == {} and pd.samples is None
    assert np.array_equal(pd.sample_pd, fill((M, 4, 16, 1), 8, dtype=np.float32))
    stats, rstats = fill((len(ranks), 4, 16, 1), 4, dtype=np.float32), fill((len(ranks), 4, 1), 7, dtype=np.float32)
    for q in (5, 95):
        assert np.array_equal(pd.pd_percentiles[q], pt._bands(stats, [5, 95], spots, ranks)[q])
        assert np.array_equal(pd.effect_range_percentiles[q], pt._bands(rstats, [5, 95], spots, ranks)[q])
    sr = fill((M, 4, 1), 6, dtype=np.float32)
    assert np.array_equal(pd.top_prob, np.stack([(np.argmax(sr, axis=1) == a).sum(axis=0) for a in range(4)]) / M)
    assert pd.top_prob.shape == (4, 1) and abs(pd.top_prob.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("key, w", [("reg", W), ("cls", WC)], ids=["reg", "cls"])
def test_weight_sources(key, w):
    for weights, M, mult in ((w, 6, None), (w.T, 6, None), ((w, MULT), 8, MULT)):
        pt, calls, pd = run(key, "test", weights=weights, inputs=[3, 1], grid=[0.25, 0.5, 0.75], percentiles=[50])
        (_, fn, args, got), = calls
        O = 1 if key == "reg" else 3
        assert args == ["test"] and pd.n_samples == M and pd.pd_mean.shape == (2, 3, O) and pd.top_prob.shape == (2, O)
        spots, ranks = pt._band_ranks(M, [50])
        assert got == front.enc(dict(w=np.asarray(w), multiplicity=mult, inputs=np.array([3, 1], np.int32), ranks=[], ranks2=ranks,
                                     grid=np.array([[0.25, 0.5, 0.75]] * 2, np.float32), ice_mean=False, sample_pd=True, sample_range=True,
                                     samples=False))
        assert pd.inputs.tolist() == [3, 1] and pd.grid.tolist() == [[0.25, 0.5, 0.75]] * 2


def test_rows_and_options():
    # "test": the integer grid comes from the test rows' columns
    pt, calls, pd = run("reg", "test", grid=3, grid_range=(0, 100), inputs=[2])
    assert calls[0][2] == ["test"]
    col = np.asarray(pt.testdata)[:, 2]
    assert np.array_equal(pd.grid[0], np.percentile(col, [0, 50, 100]).astype(np.float32).astype(np.float64))
    # rows with extra columns: cut to n_in, float32, and the grid from them
    for key, rows in (("reg", REG_ROWS), ("cls", CLS_ROWS)):
        pt, calls, pd = run(key, rows, grid=4)
        x = np.ascontiguousarray(rows[:, :4], dtype=np.float32)
        assert calls[0][2] == front.enc([x])
        assert np.array_equal(pd.grid, effects.pd_grid(x, None, 4, (5, 95))[1].astype(np.float64))
    # ice and samples: the same ranks for both sets of order statistics, every output asked for
    pt, calls, pd = run("cls", "train", ice=True, return_samples=True, percentiles=[0, 50, 100, 12.5], grid=[[0.0], [1.0]], inputs=[0, 3], chains="cold")
    got = dict(calls[0][3]["d"])
    spots, ranks = pt._band_ranks(30, [0, 50, 100, 12.5])
    assert got["'ranks'"] == got["'ranks2'"] == front.enc(ranks) and got["'ice_mean'"] is True and got["'samples'"] is True
    assert pd.ice_mean.shape == (30, 2, 1, 3) and sorted(pd.ice_percentiles) == [0, 12.5, 50, 100] and pd.samples.shape == (30, 30, 2, 1, 3)
    stats = fill((len(ranks), 30, 2, 1, 3), 2, dtype=np.float32)
    assert np.array_equal(pd.ice_percentiles[12.5], pt._bands(stats, [0, 50, 100, 12.5], spots, ranks)[12.5])
    # no percentiles: no ranks at all, empty bands
    pt, calls, pd = run("reg", percentiles=(), ice=True)
    got = dict(calls[0][3]["d"])
    assert got["'ranks'"] == got["'ranks2'"] == [] and got["'ice_mean'"] is True
    assert pd.pd_percentiles == {} and pd.effect_range_percentiles == {} and pd.ice_percentiles == {} and pd.ice_mean is not None
    assert type(pd).__name__ in dir(pt_module) and pt_module.PartialDependence is effects.PartialDependence
    assert "lags" in pt_module.ParallelTemperingBase.partial_dependence.__doc__


# ---- refusals, and the order of the checks
FAULTS = [
    ("x_unknown_name", ("valid",), {}, "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_1d", (fill(4, 1),), {}, "x must be 2-D"), ("x_too_few_columns", (BAD_ROWS,), {}, "at least n_in = 4 columns"),
    ("input_out_of_range", (), dict(inputs=[0, 4]), r"integer indices in \[0, 4\)"), ("input_negative", (), dict(inputs=[-1]), "integer indices"),
    ("inputs_empty", (), dict(inputs=[]), "integer indices"), ("input_not_an_integer", (), dict(inputs=[1.0]), "integer indices"),
    ("input_twice", (), dict(inputs=[2, 2]), "given twice"),
    ("grid_zero", (), dict(grid=0), "grid = 0 values"), ("grid_65", (), dict(grid=65), "grid = 65 values"),
    ("grid_range_not_a_pair", (), dict(grid_range=(5, 50, 95)), "must be a pair"), ("grid_range_reversed", (), dict(grid_range=(95, 5)), "0 <= lo <= hi <= 100"),
    ("grid_range_above_100", (), dict(grid_range=(5, 100.5)), "0 <= lo <= hi <= 100"),
    ("grid_wrong_rows", (), dict(grid=np.zeros((3, 5))), r"\[4, G\]"), ("grid_3d", (), dict(grid=np.zeros((4, 5, 1))), r"\[4, G\]"),
    ("grid_array_65", (), dict(grid=np.zeros(65)), "grid = 65 values"), ("grid_array_empty", (), dict(grid=[]), "grid = 0 values"),
    ("grid_nan", (), dict(grid=[0.0, np.nan]), r"grid\[0, 1\] = nan \(input 0\)"),
    ("grid_inf", (), dict(inputs=[3], grid=[[np.inf]]), r"grid\[0, 0\] = inf \(input 3\)"),
    ("grid_past_float32", (), dict(grid=[-1e39]), r"grid\[0, 0\] = -inf"),
    ("percentile_above_100", (), dict(percentiles=[5, 101]), "percentiles must lie in"), ("percentile_negative", (), dict(percentiles=[-1]), "percentiles must lie in"),
    *[(n, (), k, "weights must be" if "weights" in k else "chains") for n, k in BAD_W + TRACE_FAULTS],
    ("no_sample_trace", (), dict(burn_in=1.0), "holds no sample"), ("no_sample_multiplicities", (), dict(weights=(W, [0] * 6)), "holds no sample"),
    ("too_many_percentiles", (), dict(percentiles=MANY_PCTS), "at most 16"),
    # pairs: the order of the checks
    ("x_unknown_name_and_input_twice", ("valid",), dict(inputs=[2, 2]), "x must be"), ("input_twice_and_grid_zero", (), dict(inputs=[2, 2], grid=0), "given twice"),
    ("grid_zero_and_grid_range_reversed", (), dict(grid=0, grid_range=(95, 5)), "grid = 0 values"),
    ("grid_nan_and_percentile_above_100", (), dict(grid=[np.nan], percentiles=[101]), "not a finite"),
    ("percentile_above_100_and_weights_1d", (), dict(percentiles=[101], weights=fill(REG_P, 1)), "percentiles must lie in"),
    ("weights_1d_and_too_many_percentiles", (), dict(weights=fill(REG_P, 1), percentiles=MANY_PCTS), "weights must be"),
    ("chains_empty_and_too_many_percentiles", (), dict(chains=[], percentiles=MANY_PCTS), "chains"),
]


@pytest.mark.parametrize("name, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, args, kw, text):
    refused("reg", text, *args, **kw)


STATE_TEXT = {"none": "partial_dependence needs the chains' device handle", "sharded": "partial_dependence runs on one GPU",
              "label": "label_swap=True", "cap": "trace_capacity = 5 < NumSamples = 40", "unfinished": "no finished run_chains"}


@pytest.mark.parametrize("state", STATES)
def test_object_states(state):
    refused(f"reg_{state}", STATE_TEXT[state])
    # the handle comes first, before the rows; the trace's state last, after the percentiles
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "x must be", "valid")
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "percentiles must lie in", percentiles=[101])
    if state in ("none", "sharded"):
        refused(f"reg_{state}", STATE_TEXT[state], weights=W)
    else:                                                               # weights= need no finished trace
        _, calls, pd = run(f"reg_{state}", weights=W)
        assert len(calls) == 1 and pd.n_samples == 6
    if state == "cap":
        refused("reg_cap_unfinished", STATE_TEXT["cap"])


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(effects)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) >= 8
    hit = set()

    def local(frame, event, arg):
        if event == "line":
            hit.add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code.co_filename == path else None
    before = sys.gettrace()
    sys.settrace(tracer)
    try:
        for _, args, kw, text in FAULTS:
            refused("reg", text, *args, **kw)
    finally:
        sys.settrace(before)
    missed = {t for ln, t in sites.items() if ln not in hit}
    print(f"{len(sites)} raise sites in effects.py, {len(sites) - len(missed)} reached")
    assert missed == set()
