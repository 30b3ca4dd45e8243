"""The Python front of shapley_values (no GPU), on the two drop-in classes of tests/test_analysis_front_cpu.py with its recording
stand-in for `_lib.Sampler`, taught the one call more: valid calls over every sample source, rows and background argument, the
arguments the sampler receives, what comes back, every refusal and the order of the checks, and the object states (no handle, a
sharded ladder, label_swap, a streamed trace, an unfinished run).  The last test asserts that the cases here and the table
refusals of tests/test_shapley_cpu.py reach every `raise` of shapley.py."""
import ast
import inspect
import sys

import numpy as np
import pytest

import test_analysis_front_cpu as front
from test_analysis_front_cpu import BAD_ROWS, BAD_W, CLS_ROWS, MANY_PCTS, MULT, REG_P, REG_ROWS, STATES, TRACE_FAULTS, W, WC, fill
from test_shapley_cpu import TABLE_FAULTS

from ptnn_amd import effects, parallel_tempering as pt_module, shapley  # noqa: E402


class ShapStandIn(front.StandIn):
    def coalition_values(self, *args, **kw):
        self._log("coalition_values", args, kw)
        n, O, M = self._n_rows(args[0]), self.O, self._count(kw)
        T = np.asarray(kw["coef"]).shape[1]
        k, k2 = len(kw["ranks"]), len(kw["ranks2"])
        return dict(mean=fill((n, O, T), 1, -1, 1), order_stats=fill((k, n, O, T), 2, dtype=np.float32) if k else None,
                    pos_count=fill((n, O, T), 3, 0, M, np.int64) if kw["counts"] else None,
                    neg_count=fill((n, O, T), 4, 0, M, np.int64) if kw["counts"] else None, abs_mean=fill((O, T), 5),
                    abs_order_stats=fill((k2, O, T), 6, dtype=np.float32) if k2 else None,
                    sample_abs=fill((M, O, T), 7, dtype=np.float32) if kw["sample_abs"] else None,
                    samples=fill((M, n, O, T), 8, dtype=np.float32) if kw["samples"] else None, n_samples=M, n_distinct=-(-M // 2))


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(ShapStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.shapley_values(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).shapley_values(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def _background(rows, nb=64):
    rows = np.ascontiguousarray(np.asarray(rows)[:, :4], dtype=np.float32)
    if rows.shape[0] > nb:
        rows = np.ascontiguousarray(rows[np.rint(np.linspace(0, rows.shape[0] - 1, nb)).astype(np.int64)])
    return rows


# ---- valid calls
TRACE = [("all", {}, dict(replicas=None, step0=10, nsteps=30, thin=1), 120),
         ("cold_thin", dict(chains="cold", thin=3), dict(replicas=[1], step0=10, nsteps=30, thin=3), 10),
         ("list_burn_in", dict(chains=[2, 0], burn_in=0.5, thin=2), dict(replicas=[2, 0], step0=20, nsteps=20, thin=2), 20),
         ("burn_in_zero", dict(burn_in=0), dict(replicas=None, step0=0, nsteps=40, thin=1), 160)]


@pytest.mark.parametrize("name, kw, source, M", TRACE, ids=[t[0] for t in TRACE])
def test_trace_sources(name, kw, source, M):
    pt, calls, sv = run("reg", **kw)
    (tag, fn, args, got), = calls
    assert (tag, fn, args) == ("self", "coalition_values", ["test"])
    masks, coef = shapley.shapley_table(4)
    bg = _background(pt.traindata)
    spots, ranks = pt._band_ranks(M, [5, 95])
    want = dict(source, background=bg, masks=masks, coef=coef, ranks=ranks, ranks2=ranks, counts=True, sample_abs=True, samples=False)
    assert got == front.enc(want)
    n = np.asarray(pt.testdata).shape[0]
    assert sv.method == "exact" and sv.n_coalitions == 16 and np.array_equal(sv.background, bg) and sv.background.dtype == np.float32
    assert sv.n_samples == M and sv.n_distinct == -(-M // 2) and sv.samples is None
    mean = fill((n, 1, 6), 1, -1, 1)
    assert np.array_equal(sv.phi_mean, mean[:, :, :4]) and np.array_equal(sv.base, mean[0, :, 4]) and np.array_equal(sv.fx_mean, mean[:, :, 5])
    assert sv.efficiency_gap == float(np.max(np.abs(mean[:, :, :4].sum(axis=2) - (mean[:, :, 5] - mean[:, :, 4]))))
    assert np.array_equal(sv.prob_positive, fill((n, 1, 6), 3, 0, M, np.int64)[:, :, :4] / np.float64(M))
    assert np.array_equal(sv.importance, fill((1, 6), 5)[:, :4])
    sa = fill((M, 1, 6), 7, dtype=np.float32)[:, :, :4]
    assert np.array_equal(sv.sample_importance, sa) and sv.sample_importance.flags.c_contiguous
    assert np.array_equal(sv.top_prob, np.stack([(np.argmax(sa, axis=2) == i).sum(axis=0) for i in range(4)], axis=1) / M)
    stats, astats = fill((len(ranks), n, 1, 6), 2, dtype=np.float32), fill((len(ranks), 1, 6), 6, dtype=np.float32)
    for q in (5, 95):
        band = pt._bands(stats, [5, 95], spots, ranks)[q]
        assert np.array_equal(sv.phi_percentiles[q], band[:, :, :4]) and np.array_equal(sv.base_percentiles[q], band[0, :, 4])
        assert np.array_equal(sv.importance_percentiles[q], pt._bands(astats, [5, 95], spots, ranks)[q][:, :4])


@pytest.mark.parametrize("key, w", [("reg", W), ("cls", WC)], ids=["reg", "cls"])
def test_weight_sources(key, w):
    orders = np.array([[3, 1, 0, 2], [2, 0, 1, 3], [0, 1, 2, 3]])
    for weights, M, mult in ((w, 6, None), (w.T, 6, None), ((w, MULT), 8, MULT)):
        pt, calls, sv = run(key, "train", "test", weights=weights, permutations=orders, percentiles=[50], max_background=5)
        (_, fn, args, got), = calls
        O = 1 if key == "reg" else 3
        masks, coef = shapley.shapley_table(4, permutations=orders)
        bg = _background(pt.testdata, 5)
        assert bg.shape == (5, 4)
        spots, ranks = pt._band_ranks(M, [50])
        assert args == ["train"] and got == front.enc(dict(w=np.asarray(w), multiplicity=mult, background=bg, masks=masks, coef=coef, ranks=ranks,
                                                          ranks2=ranks, counts=True, sample_abs=True, samples=False))
        n = np.asarray(pt.traindata).shape[0]
        assert sv.method == "permutation" and sv.n_coalitions == masks.size and sv.n_samples == M
        assert sv.phi_mean.shape == (n, O, 4) and sv.base.shape == (O,) and sv.fx_mean.shape == (n, O) and sv.top_prob.shape == (O, 4)
        assert sv.importance.shape == (O, 4) and sv.sample_importance.shape == (M, O, 4) and sorted(sv.phi_percentiles) == [50]


def test_rows_and_options():
    # rows with extra columns: cut to n_in, float32; a background array likewise, small enough to be taken whole
    for key, rows in (("reg", REG_ROWS), ("cls", CLS_ROWS)):
        pt, calls, sv = run(key, rows, rows[:7], chains="cold")
        x = np.ascontiguousarray(rows[:, :4], dtype=np.float32)
        assert calls[0][2] == front.enc([x]) and np.array_equal(sv.background, x[:7])
    # the deterministic subsample: rows at np.rint(np.linspace(0, n - 1, max_background))
    pt, calls, sv = run("reg", "test", "train", max_background=3)
    tr = np.asarray(pt.traindata)
    assert np.array_equal(sv.background, tr[[0, int(np.rint((tr.shape[0] - 1) / 2)), tr.shape[0] - 1], :4].astype(np.float32))
    # method and seed reach the table; samples on request; no percentiles: no ranks, empty bands
    pt, calls, sv = run("cls", method="permutation", n_permutations=4, seed=9, return_samples=True, percentiles=())
    got = dict(calls[0][3]["d"])
    masks, coef = shapley.shapley_table(4, "permutation", 4, 9)
    assert got["'masks'"] == front.enc(masks) and got["'coef'"] == front.enc(coef) and got["'samples'"] is True
    assert got["'ranks'"] == got["'ranks2'"] == []
    assert sv.method == "permutation" and sv.phi_percentiles == {} and sv.base_percentiles == {} and sv.importance_percentiles == {}
    assert sv.samples.shape == (sv.n_samples, np.asarray(pt.testdata).shape[0], 3, 6)
    assert run("reg", method="exact")[2].method == "exact"
    assert type(sv).__name__ in dir(pt_module) and pt_module.ShapleyValues is shapley.ShapleyValues is effects.ShapleyValues
    doc = pt_module.ParallelTemperingBase.shapley_values.__doc__
    assert "lags" in doc and "never produced" in doc and "error is not reported" in doc


# ---- refusals, and the order of the checks
NAN_BG = fill((5, 4), 2)
NAN_BG[3, 1] = np.nan
FAULTS = [
    ("x_unknown_name", ("valid",), {}, "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_1d", (fill(4, 1),), {}, "x must be 2-D"), ("x_too_few_columns", (BAD_ROWS,), {}, "at least n_in = 4 columns"),
    ("background_unknown_name", ("test", "valid"), {}, "background must be 'train', 'test' or an array, not 'valid'"),
    ("background_too_few_columns", ("test", BAD_ROWS), {}, "background must be 2-D with at least n_in = 4 columns"),
    ("background_empty", ("test", np.zeros((0, 4))), {}, "background holds no row"),
    ("background_nan", ("test", NAN_BG), {}, r"background\[3, 1\] = nan is not a finite float32"),
    ("background_inf", ("test", np.full((2, 4), -np.inf)), {}, r"background\[0, 0\] = -inf"),
    ("max_background_zero", (), dict(max_background=0), r"max_background = 0 must be an integer in \[1, 256\]"),
    ("max_background_257", (), dict(max_background=257), "max_background = 257"),
    ("max_background_fraction", (), dict(max_background=2.5), "max_background = 2.5"),
    *[(f"table_{k}", (), {a: b for a, b in kw.items() if a != "n_in"}, text) for k, (kw, text) in enumerate(TABLE_FAULTS) if "n_in" not in kw],
    ("percentile_above_100", (), dict(percentiles=[5, 101]), "percentiles must lie in"), ("percentile_negative", (), dict(percentiles=[-1]), "percentiles must lie in"),
    *[(n, (), k, "weights must be" if "weights" in k else "chains") for n, k in BAD_W + TRACE_FAULTS],
    ("no_sample_trace", (), dict(burn_in=1.0), "holds no sample"), ("no_sample_multiplicities", (), dict(weights=(W, [0] * 6)), "holds no sample"),
    ("too_many_percentiles", (), dict(percentiles=MANY_PCTS), "at most 16"),
    # pairs: the order of the checks
    ("x_unknown_name_and_background_unknown_name", ("valid", "valid"), {}, "x must be"),
    ("background_nan_and_max_background_zero", ("test", NAN_BG), dict(max_background=0), "max_background = 0"),
    ("background_nan_and_method_unknown", ("test", NAN_BG), dict(method="kernel"), "not a finite"),
    ("method_unknown_and_percentile_above_100", (), dict(method="kernel", percentiles=[101]), "method = 'kernel'"),
    ("percentile_above_100_and_weights_1d", (), dict(percentiles=[101], weights=fill(REG_P, 1)), "percentiles must lie in"),
    ("weights_1d_and_too_many_percentiles", (), dict(weights=fill(REG_P, 1), percentiles=MANY_PCTS), "weights must be"),
    ("chains_empty_and_too_many_percentiles", (), dict(chains=[], percentiles=MANY_PCTS), "chains"),
]


@pytest.mark.parametrize("name, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, args, kw, text):
    refused("reg", text, *args, **kw)


STATE_TEXT = {"none": "shapley_values needs the chains' device handle", "sharded": "shapley_values runs on one GPU",
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
        _, calls, sv = run(f"reg_{state}", weights=W)
        assert len(calls) == 1 and sv.n_samples == 6
    if state == "cap":
        refused("reg_cap_unfinished", STATE_TEXT["cap"])


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(shapley)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) >= 10
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
        for kw, text in TABLE_FAULTS:
            table = dict(n_in=4, method="auto", n_permutations=32, seed=0, permutations=None)
            table.update(kw)
            with pytest.raises(ValueError, match=text):
                shapley.shapley_table(**table)
    finally:
        sys.settrace(before)
    missed = {t for ln, t in sites.items() if ln not in hit}
    print(f"{len(sites)} raise sites in shapley.py, {len(sites) - len(missed)} reached")
    assert missed == set()
