"""The Python front of posterior_modes (no GPU), on the two drop-in classes of tests/test_analysis_front_cpu.py with its recording
stand-in for `_lib.Sampler`, taught the one call more: valid calls over every sample source, the keywords the sampler receives
(radius_sq_sum formed in double among them), what comes back, every refusal and the order of the checks, and the object states (no
handle, a sharded ladder, label_swap, a streamed trace, an unfinished run).  The last test asserts that the cases here reach every
`raise` of modes.py."""
import ast
import inspect
import math
import sys

import numpy as np
import pytest

import modes_ref as ref
import test_analysis_front_cpu as front
from test_analysis_front_cpu import BAD_ROWS, BAD_W, CLS_ROWS, MULT, REG_P, REG_ROWS, STATES, TRACE_FAULTS, W, WC, fill

from ptnn_amd import modes, parallel_tempering as pt_module  # noqa: E402

VALUES = np.concatenate([fill((4, 3), 21, 0.1, 0.12, np.float32), fill((4, 3), 22, 0.8, 0.82, np.float32)])     # two clumps of four
DISTINCT = 5


def canned(n_items, mult, n, near_sq, F=None):
    """What a device would return for `n_items` items that fall on DISTINCT samples in turn: two clumps in the outputs."""
    U = min(DISTINCT, n_items) if F is None else len(F)
    item = np.arange(n_items) % U
    count = np.bincount(item, weights=np.ones(n_items) if mult is None else np.maximum(mult, 0), minlength=U).astype(np.int32)
    if F is None:
        F = (fill((U, n), 3, 0.0, 0.004) + np.where(np.arange(U) % 2 == 0, 0.2, 0.7)[:, None]).astype(np.float32)
    sq = ref.sq_longdouble(F).astype(np.float64)
    rho, delta, parent = ref.density_peaks(sq, count, near_sq)
    return dict(rho=rho, delta_sq=delta, parent=parent.astype(np.int32), count=count, item_sample=item.astype(np.int32), outputs=F,
                spread_sq=float(ref.spread_sq(sq, count)), sq_dist=sq, n_samples=int(count.sum()), n_distinct=U)


class ModesStandIn(front.StandIn):
    def modes(self, *args, **kw):
        self._log("modes", args, kw)
        if kw.get("values") is not None:
            v = kw["values"]
            out = canned(len(v), kw.get("multiplicity"), v.shape[1], kw["radius_sq_sum"], F=v)
        else:
            n = self._n_rows(args[0]) * self.O
            n_items = len(kw["w"]) if kw.get("w") is not None else self._count(kw)
            out = canned(n_items, kw.get("multiplicity") if kw.get("w") is not None else None, n, kw["radius_sq_sum"])
        if not kw["sq_dist"]:
            out["sq_dist"] = None
        return out


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(ModesStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.posterior_modes(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).posterior_modes(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def _check(pm, out, shape, sep, min_mass=0.02, n_chains=None):
    """The result against the stand-in's canned outputs, finished by the plain restatement."""
    n = int(np.prod(shape))
    M = out["n_samples"]
    lab, centres, mass = ref.labels_of(out["rho"], out["delta_sq"], out["parent"], out["count"], sep * sep * n, math.ceil(min_mass * M))
    assert pm.n_modes == len(centres) and np.array_equal(pm.sample_labels, lab) and np.array_equal(pm.centres, centres)
    assert np.array_equal(pm.mass, mass / M) and pm.n_samples == M and pm.n_distinct == out["n_distinct"]
    assert pm.mode_mean.shape == (pm.n_modes,) + shape == pm.mode_sd.shape and pm.between.shape == (pm.n_modes,) * 2
    assert np.array_equal(pm.rho, out["rho"]) and np.array_equal(pm.parent, out["parent"]) and np.array_equal(pm.delta, np.sqrt(out["delta_sq"] / n))
    assert pm.spread == math.sqrt(out["spread_sq"] / n)
    items = lab[out["item_sample"]]
    if n_chains is None:
        assert np.array_equal(pm.labels, items) and pm.occupancy is None and pm.hops is None and pm.hop_matrix is None
    else:
        occ, hops, hm = ref.chain_figures(items.reshape(n_chains, -1), pm.n_modes)
        assert np.array_equal(pm.labels, items.reshape(n_chains, -1))
        assert np.array_equal(pm.occupancy, occ) and np.array_equal(pm.hops, hops) and np.array_equal(pm.hop_matrix, hm)
    return lab


# ---- valid calls
TRACE = [("all", {}, dict(replicas=None, step0=10, nsteps=30, thin=1), 4, 120),
         ("cold_thin", dict(chains="cold", thin=3), dict(replicas=[1], step0=10, nsteps=30, thin=3), 1, 10),
         ("list_burn_in", dict(chains=[2, 0], burn_in=0.5, thin=2), dict(replicas=[2, 0], step0=20, nsteps=20, thin=2), 2, 20),
         ("burn_in_zero", dict(burn_in=0), dict(replicas=None, step0=0, nsteps=40, thin=1), 4, 160)]


@pytest.mark.parametrize("name, kw, source, C, M", TRACE, ids=[t[0] for t in TRACE])
def test_trace_sources(name, kw, source, C, M):
    pt, calls, pm = run("reg", **kw)
    (tag, fn, args, got), = calls
    n = len(pt.traindata)
    rad = 0.05 / 2
    assert (tag, fn, args) == ("self", "modes", ["train"])                                   # the default rows
    assert got == front.enc(dict(source, radius_sq_sum=rad * rad * n, sq_dist=False, outputs=True))
    _check(pm, canned(M, None, n, rad * rad * n), (n, 1), 0.05, n_chains=C)
    assert pm.n_modes == 2 and pm.labels.shape == (C, M // C) and pm.distances is None and pm.centre_rows.shape == (2, 2)
    assert (pm.centre_rows[:, 0] == 0).all()                                                 # the five samples all show in chain 0 first


@pytest.mark.parametrize("key, w", [("reg", W), ("cls", WC)], ids=["reg", "cls"])
def test_weight_sources(key, w):
    O = 1 if key == "reg" else 3
    for weights, mult in ((w, None), (w.T, None), ((w, MULT), MULT)):
        pt, calls, pm = run(key, "test", weights=weights, separation=0.2, radius=0.01, min_mass=0.0, return_distances=True)
        (_, fn, args, got), = calls
        n = len(pt.testdata) * O
        assert args == ["test"]
        assert got == front.enc(dict(w=np.asarray(w), multiplicity=mult, radius_sq_sum=0.01 * 0.01 * n, sq_dist=True, outputs=True))
        out = canned(6, None if mult is None else np.asarray(mult), n, 0.01 * 0.01 * n)
        _check(pm, out, (len(pt.testdata), O), 0.2, min_mass=0.0)
        assert np.array_equal(pm.distances, np.sqrt(out["sq_dist"] / n)) and (pm.centre_rows[:, 0] == -1).all() and (pm.centre_rows[:, 1] >= 0).all()


def test_rows_values_and_options():
    # rows with extra columns: x cut to n_in, float32
    for key, rows in (("reg", REG_ROWS), ("cls", CLS_ROWS)):
        pt, calls, pm = run(key, rows, chains="cold")
        assert calls[0][2] == front.enc([np.ascontiguousarray(rows[:, :4], dtype=np.float32)])
        assert pm.mode_mean.shape[1:] == (12, 1 if key == "reg" else 3)
    # a host matrix: no rows, no samples; a pair carries the multiplicities
    pt, calls, pm = run("reg", values=VALUES, separation=0.1)
    (_, fn, args, got), = calls
    assert fn == "modes" and args == [] and got == front.enc(dict(values=VALUES, multiplicity=None, radius_sq_sum=0.05 * 0.05 * 3, sq_dist=False, outputs=True))
    lab = _check(pm, canned(8, None, 3, 0.05 * 0.05 * 3, F=VALUES), (3,), 0.1)
    assert pm.n_modes == 2 and lab.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and (pm.centre_rows == -1).all() and pm.mass.tolist() == [0.5, 0.5]
    mult = [1, 0, 2, 1, 1, 3, 0, 1]
    pt, calls, pm = run("cls", values=(VALUES.astype(np.float64).tolist(), mult), separation=0.1, radius=0.03)
    assert calls[0][3] == front.enc(dict(values=VALUES, multiplicity=mult, radius_sq_sum=0.03 * 0.03 * 3, sq_dist=False, outputs=True))
    lab = _check(pm, canned(8, np.asarray(mult), 3, 0.03 * 0.03 * 3, F=VALUES), (3,), 0.1)
    assert lab.tolist() == [1, -1, 1, 1, 0, 0, -1, 0] and pm.mass.tolist() == [5 / 9, 4 / 9]
    assert type(pm).__name__ in dir(pt_module) and pt_module.PosteriorModes is modes.PosteriorModes
    assert pt_module.modes_stuck is modes.modes_stuck and pt_module.mode_labels is modes.mode_labels and pt_module.chain_hops is modes.chain_hops
    doc = " ".join(pt_module.ParallelTemperingBase.posterior_modes.__doc__.split())
    assert "conventions in output units" in doc and "not tuned values" in doc and "Rodriguez & Laio 2014" in doc
    assert 'chains="cold" is the posterior\'s own figure' in doc and 'chains="all" pools the tempered rungs' in doc


# ---- refusals, and the order of the checks
FAULTS = [
    ("separation_zero", (), dict(separation=0), "separation = 0 must be a finite number > 0"),
    ("separation_nan", (), dict(separation=float("nan")), "separation = nan"),
    ("radius_negative", (), dict(radius=-0.1), "radius = -0.1 must be a finite number >= 0"),
    ("radius_inf", (), dict(radius=float("inf")), "radius = inf"),
    ("min_mass_above_one", (), dict(min_mass=1.5), r"min_mass = 1.5 must lie in \[0, 1\]"),
    ("min_mass_negative", (), dict(min_mass=-0.1), "min_mass = -0.1"),
    ("x_unknown_name", ("valid",), {}, "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_1d", (fill(4, 1),), {}, "x must be 2-D"), ("x_too_few_columns", (BAD_ROWS,), {}, "at least n_in = 4 columns"),
    *[(n, (), k, "weights must be" if "weights" in k else "chains") for n, k in BAD_W + TRACE_FAULTS],
    ("no_sample_trace", (), dict(burn_in=1.0), "the selection holds no sample"),
    ("no_sample_weights", (), dict(weights=(W, [0, 0, 0, 0, 0, 0])), "the selection holds no sample"),
    ("values_with_weights", (), dict(values=VALUES, weights=W), "no weights= with it"),
    ("values_1d", (), dict(values=VALUES[:, 0]), r"values must be \[n_samples, n_a\], got shape \(8,\)"),
    ("values_no_row", (), dict(values=VALUES[:0]), "values must be"), ("values_no_column", (), dict(values=VALUES[:, :0]), "values must be"),
    ("values_no_sample", (), dict(values=(VALUES, [0] * 8)), "the selection holds no sample"),
    # pairs: the order of the checks
    ("separation_zero_and_radius_negative", (), dict(separation=0, radius=-1), "separation = 0"),
    ("radius_negative_and_min_mass", (), dict(radius=-0.1, min_mass=2), "radius = -0.1"),
    ("min_mass_and_x_unknown_name", ("valid",), dict(min_mass=2), "min_mass = 2"),
    ("min_mass_and_values_with_weights", (), dict(min_mass=2, values=VALUES, weights=W), "min_mass = 2"),
    ("x_unknown_name_and_weights_1d", ("valid",), dict(weights=fill(REG_P, 1)), "x must be"),
    ("values_with_weights_and_1d", (), dict(values=VALUES[:, 0], weights=W), "no weights= with it"),
    ("values_1d_and_no_sample", (), dict(values=(VALUES[:, 0], [0] * 8)), "values must be"),
]


@pytest.mark.parametrize("name, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, args, kw, text):
    refused("reg", text, *args, **kw)


STATE_TEXT = {"none": "posterior_modes needs the chains' device handle", "sharded": "posterior_modes runs on one GPU",
              "label": "label_swap=True", "cap": "trace_capacity = 5 < NumSamples = 40", "unfinished": "no finished run_chains"}


@pytest.mark.parametrize("state", STATES)
def test_object_states(state):
    refused(f"reg_{state}", STATE_TEXT[state])
    # the handle comes first, before the arguments; the trace's state last, after the rows
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "separation = 0", separation=0)
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "x must be", "valid")
    if state in ("none", "sharded"):
        refused(f"reg_{state}", STATE_TEXT[state], weights=W)
        refused(f"reg_{state}", STATE_TEXT[state], values=VALUES)
    else:                                                               # weights= and values= need no finished trace
        _, calls, pm = run(f"reg_{state}", weights=W)
        assert len(calls) == 1 and pm.n_samples == 6
        _, calls, pm = run(f"reg_{state}", values=VALUES)
        assert len(calls) == 1 and pm.n_samples == 8
    if state == "cap":
        refused("reg_cap_unfinished", STATE_TEXT["cap"])


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(modes)
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
        pm = modes.PosteriorModes(*[None] * len(modes.PosteriorModes._fields))
        with pytest.raises(ValueError, match="min_mass = 2 must lie in"):
            modes.modes_stuck(pm, min_mass=2)
        with pytest.raises(ValueError, match="has no chains"):
            modes.modes_stuck(pm)
    finally:
        sys.settrace(before)
    missed = {t for ln, t in sites.items() if ln not in hit}
    print(f"{len(sites)} raise sites in modes.py, {len(sites) - len(missed)} reached")
    assert missed == set()
