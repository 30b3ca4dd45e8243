"""The Python front of posterior_compress (no GPU), on the two drop-in classes of tests/test_analysis_front_cpu.py with its recording
stand-in for `_lib.Sampler`, taught the one call more (answered by tests/compress_ref.py): valid calls over every sample source, the
keywords the sampler receives, what comes back, every refusal and the order of the checks, the object states, the binding's
symbol table and the README's example.  The last test asserts that the cases here reach every `raise` of compress.py."""
import ast
import inspect
import os
import re
import sys

import numpy as np
import pytest

import compress_ref as ref
import test_analysis_front_cpu as front
from test_analysis_front_cpu import BAD_ROWS, BAD_W, ETA, MULT, REG_P, STATES, TRACE_FAULTS, W, WC, fill

from ptnn_amd import _lib, compress, parallel_tempering as pt_module  # noqa: E402

VALUES = np.concatenate([fill((6, 3), 21, 0.1, 0.12, np.float32), fill((2, 3), 22, 0.8, 0.82, np.float32)])      # clumps of six and two
DISTINCT = 5


def canned(n_items, mult, n, m, subsets, F=None):
    """What a device would return for `n_items` items that fall on DISTINCT samples in turn."""
    U = min(DISTINCT, n_items) if F is None else len(F)
    item = np.arange(n_items) % U
    count = np.bincount(item, weights=np.ones(n_items) if mult is None else np.maximum(mult, 0), minlength=U).astype(np.int32)
    if F is None:
        F = (fill((U, n), 3, 0.0, 0.004) + np.where(np.arange(U) % 2 == 0, 0.2, 0.7)[:, None]).astype(np.float32)
    sq = ref.sq_of(F)
    h = ref.herd(sq, count, m)
    sub = None if subsets is None else np.array([float(ref.subset_energy(sq, count, item[s], mu=h["mu"], d0=h["d0"])) for s in subsets])
    return dict(picks=h["picks"].astype(np.int32), energy=h["energy"], pick_score=h["pick_score"], mu=h["mu"], d0=float(h["d0"]),
                subset_energy=sub, count=count, item_sample=item.astype(np.int32), outputs=F, sq_dist=sq, n_samples=int(count.sum()), n_distinct=U)


class CompressStandIn(front.StandIn):
    def compress(self, *args, **kw):
        self._log("compress", args, kw)
        if kw.get("values") is not None:
            v = kw["values"]
            out = canned(len(v), kw.get("multiplicity"), v.shape[1], kw["m"], kw["subsets"], F=v)
        else:
            n = self._n_rows(args[0]) * self.O
            n_items = len(kw["w"]) if kw.get("w") is not None else self._count(kw)
            out = canned(n_items, kw.get("multiplicity") if kw.get("w") is not None else None, n, kw["m"], kw["subsets"])
        if not kw.get("sq_dist"):
            out["sq_dist"] = None
        return out

    def traces(self, step0=0, nsteps=None, pos_w=True):
        return dict(pos_w=(fill((self.R, 1, self.P), 40, dtype=np.float32) + np.float32(step0)))

    def trace_rows(self, row0=0, nrows=None):
        return fill((self.R, 1, 8), 41, dtype=np.float32) - np.float32(row0)


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(CompressStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def run(key, *args, **kw):
    calls = []
    pt = make(key, calls)
    return pt, calls, pt.posterior_compress(*args, **kw)


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).posterior_compress(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def _check(pc, out, n, m):
    assert np.array_equal(pc.picks, out["picks"][:m]) and pc.picks.dtype == np.int64 and np.array_equal(pc.energy, out["energy"])
    assert pc.spread == out["d0"] and pc.spread_rms == out["d0"] / np.sqrt(n) and np.array_equal(pc.energy_rms, out["energy"] / np.sqrt(n))
    assert np.array_equal(pc.equivalent_draws, np.where(out["energy"] > 0, out["d0"] / np.where(out["energy"] > 0, out["energy"], 1), np.inf))
    assert np.array_equal(pc.items, compress.first_items(out["item_sample"], out["n_distinct"])[out["picks"]])
    assert pc.n_samples == out["n_samples"] and pc.n_distinct == out["n_distinct"] and np.array_equal(pc.mu, out["mu"])
    assert (pc.mean_gap, pc.sd_ratio) == compress.moment_match(out["outputs"], out["count"], out["picks"])
    assert pc.energy_thinned == out["subset_energy"][-1]


# ---- valid calls
TRACE = [("all", {}, dict(replicas=None, step0=10, nsteps=30, thin=1), 4, 120),
         ("cold_thin", dict(chains="cold", thin=3), dict(replicas=[1], step0=10, nsteps=30, thin=3), 1, 10),
         ("list_burn_in", dict(chains=[2, 0], burn_in=0.5, thin=2), dict(replicas=[2, 0], step0=20, nsteps=20, thin=2), 2, 20)]


@pytest.mark.parametrize("name, kw, source, C, M", TRACE, ids=[t[0] for t in TRACE])
def test_trace_sources(name, kw, source, C, M):
    pt, calls, pc = run("reg", 3, **kw)
    (tag, fn, args, got), = calls
    n = len(pt.traindata)
    thinned = ((np.arange(3) * M) // 3).astype(np.int32)[None, :]
    assert (tag, fn, args) == ("self", "compress", ["train"])                                # the default rows
    assert got == front.enc(dict(source, m=3, subsets=thinned, sq_dist=False, outputs=True))
    out = canned(M, None, n, 3, thinned)
    _check(pc, out, n, 3)
    assert pc.rows.shape == (3, 2) and pc.evaluated is None and pc.distances is None
    per = M // C
    assert np.array_equal(pc.rows, np.stack([pc.items // per, pc.items % per], axis=1))
    # the vectors and eta are the trace rows of the picks: row step0 + thin * r of chain replicas[c]
    reps = list(range(4)) if source["replicas"] is None else source["replicas"]
    base, rows = fill((4, 1, REG_P), 40, dtype=np.float32), fill((4, 1, 8), 41, dtype=np.float32)
    for k, (c, r) in enumerate(pc.rows):
        step = source["step0"] + source["thin"] * int(r)
        assert np.array_equal(pc.vectors[k], base[reps[c], 0] + np.float32(step)) and pc.eta[k] == rows[reps[c], 0, 3] - np.float32(step)
    assert pc.vectors.dtype == np.float32 and pc.eta.dtype == np.float32


def test_weight_sources_and_evaluate():
    for key, w, eta in (("reg", W, ETA), ("reg", W, None), ("cls", WC, None)):
        O = 1 if key == "reg" else 3
        for weights, mult in ((w, None), (w.T, None), ((w, MULT), MULT)):
            ev = [0, 3, 3]
            pt, calls, pc = run(key, 2, "test", weights=weights, eta=eta, evaluate=ev, return_distances=True)
            n = len(pt.testdata) * O
            thinned = compress.thinned_items(2, 6, mult).astype(np.int32)[None, :]
            # evaluate= has another size than m: the thinned subset is judged by a call of its own
            (_, fn, args, got), (_, fn2, args2, got2) = calls
            assert fn == fn2 == "compress" and args == args2 == ["test"]
            assert got == front.enc(dict(w=np.asarray(w), multiplicity=mult, m=2, subsets=np.array([ev], np.int32), sq_dist=True, outputs=True))
            assert got2 == front.enc(dict(w=np.asarray(w), multiplicity=mult, m=0, subsets=thinned))
            out = canned(6, None if mult is None else np.asarray(mult), n, 2, np.array([ev]))
            assert np.array_equal(pc.evaluated, out["subset_energy"]) and pc.evaluated.shape == (1,)
            assert pc.energy_thinned == canned(6, None if mult is None else np.asarray(mult), n, 0, thinned)["subset_energy"][0]
            assert np.array_equal(pc.distances, np.sqrt(out["sq_dist"] / n)) and (pc.rows[:, 0] == -1).all() and np.array_equal(pc.rows[:, 1], pc.items)
            assert np.array_equal(pc.vectors, np.asarray(w, dtype=np.float32)[pc.items])
            assert pc.eta is None if eta is None else np.array_equal(pc.eta, np.asarray(eta, dtype=np.float32)[pc.items])
    # evaluate= of the size m rides in the same call, the thinned subset last; a [B, k] array is taken as it is
    pt, calls, pc = run("reg", 2, weights=W, evaluate=[[0, 1], [4, 4]])
    (_, _, _, got), = calls
    sub = np.array([[0, 1], [4, 4], [0, 3]], np.int32)
    assert got == front.enc(dict(w=W, multiplicity=None, m=2, subsets=sub, sq_dist=False, outputs=True))
    out = canned(6, None, len(pt.traindata), 2, sub)
    assert np.array_equal(pc.evaluated, out["subset_energy"][:2]) and pc.energy_thinned == out["subset_energy"][2]
    # m = 0: nothing is picked, the subsets are judged
    pt, calls, pc = run("reg", 0, "test", weights=W, evaluate=pc.items)
    assert len(calls) == 1 and pc.picks.shape == (0,) and pc.energy_thinned is None and pc.mean_gap is None and pc.vectors is None
    assert pc.evaluated.shape == (1,) and pc.rows.shape == (0, 2) and pc.spread > 0


def test_values_and_exports():
    pt, calls, pc = run("reg", 3, values=VALUES)
    (_, fn, args, got), = calls
    thinned = np.array([[0, 2, 5]], np.int32)
    assert fn == "compress" and args == [] and got == front.enc(dict(values=VALUES, multiplicity=None, m=3, subsets=thinned, sq_dist=False, outputs=True))
    _check(pc, canned(8, None, 3, 3, thinned, F=VALUES), 3, 3)
    assert pc.vectors is None and pc.eta is None and (pc.rows == -1).all() and int((pc.picks >= 6).sum()) == 1
    mult = [1, 0, 2, 1, 1, 3, 0, 1]
    pt, calls, pc = run("cls", np.int64(2), values=(VALUES.astype(np.float64).tolist(), mult))
    assert calls[0][3] == front.enc(dict(values=VALUES, multiplicity=mult, m=2, subsets=np.array([[0, 4]], np.int32), sq_dist=False, outputs=True))
    assert pc.n_samples == 9 and not set(pc.picks) & {1, 6}
    assert "ptnn_compress" in _lib.SYMBOLS and _lib.SYMBOLS["ptnn_compress"][1][1]._type_ is _lib.CompressSpec and _lib.ABI_VERSION == 4
    assert pt_module.PosteriorCompression is compress.PosteriorCompression and pt_module.moment_match is compress.moment_match


def test_readme_example_names_exist():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "README.md")).read()
    block = text[text.index("pt.posterior_compress(32"):]
    block = block[:block.index("```")]
    assert "weights=pc.vectors" in block and "eta=pc.eta" in block and "evaluate=pc.items" in block
    for name in re.findall(r"pc\.([a-z_]+)", block):
        assert name in compress.PosteriorCompression._fields, name
    for method in re.findall(r"pt\.([a-z_]+)\(", block):
        assert callable(getattr(pt_module.ParallelTemperingBase, method)), method
    params = inspect.signature(pt_module.ParallelTemperingBase.posterior_compress).parameters
    for word in ("chains", "evaluate", "burn_in", "thin", "weights", "values"):
        assert word in params
    assert "ptnn_dev_compress.hpp" in text and "NOT monotone" in " ".join(open(os.path.join(root, "DESIGN.md")).read().split())


# ---- refusals, and the order of the checks
FAULTS = [
    ("m_negative", (-1,), {}, "m = -1 must be an integer in"), ("m_float", (2.5,), {}, "m = 2.5 must be an integer"),
    ("m_text", ("3",), {}, "m = '3' must be an integer"), ("m_bool", (True,), {}, "m = True must be an integer"),
    ("m_above_items", (121,), {}, "m = 121 picks but the selection holds 120 items"),
    ("m_above_positive", (6,), dict(weights=(W, MULT)), "m = 6 picks but the selection holds 5 items with a positive count"),
    ("m_above_values", (9,), dict(values=VALUES), "m = 9 picks but the selection holds 8"),
    ("eta_without_weights", (2,), dict(eta=ETA), "eta= comes with weights="),
    ("eta_wrong_length", (2,), dict(weights=W, eta=ETA[:3]), "eta must have one entry per vector: 6"),
    ("x_unknown_name", (2, "valid"), {}, "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_too_few_columns", (2, BAD_ROWS), {}, "at least n_in = 4 columns"),
    *[(n, (2,), k, "weights must be" if "weights" in k else "chains") for n, k in BAD_W + TRACE_FAULTS],
    ("no_sample_trace", (0,), dict(burn_in=1.0), "the selection holds no sample"),
    ("no_sample_weights", (0,), dict(weights=(W, [0, 0, 0, 0, 0, 0])), "the selection holds no sample"),
    ("values_with_weights", (2,), dict(values=VALUES, weights=W), "no weights= with it"),
    ("values_1d", (2,), dict(values=VALUES[:, 0]), r"values must be \[n_samples, n_a\], got shape \(8,\)"),
    ("values_no_sample", (0,), dict(values=(VALUES, [0] * 8)), "the selection holds no sample"),
    ("evaluate_out_of_range", (2,), dict(weights=W, evaluate=[0, 6]), r"evaluate holds item 6 outside \[0, 6\)"),
    ("evaluate_negative", (2,), dict(evaluate=[[0, -1]]), r"evaluate holds item -1 outside \[0, 120\)"),
    ("evaluate_absent", (2,), dict(weights=(W, MULT), evaluate=[0, 2]), "evaluate holds item 2, whose multiplicity is 0"),
    ("evaluate_3d", (2,), dict(evaluate=np.zeros((1, 2, 2), int)), "evaluate must be one list"),
    ("evaluate_floats", (2,), dict(evaluate=[0.5, 1.0]), "evaluate must be one list"),
    ("evaluate_empty", (2,), dict(evaluate=[]), "evaluate must be one list"),
    # pairs: the order of the checks
    ("m_and_eta", (-1,), dict(eta=ETA), "m = -1"), ("eta_and_x", (2, "valid"), dict(eta=ETA), "eta= comes with"),
    ("x_and_weights", (2, "valid"), dict(weights=fill(REG_P, 1)), "x must be"), ("m_above_and_evaluate", (7,), dict(weights=W, evaluate=[9]), "m = 7 picks"),
    ("values_with_weights_and_1d", (2,), dict(values=VALUES[:, 0], weights=W), "no weights= with it"),
]


@pytest.mark.parametrize("name, args, kw, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_refusals(name, args, kw, text):
    refused("reg", text, *args, **kw)


STATE_TEXT = {"none": "posterior_compress needs the chains' device handle", "sharded": "posterior_compress runs on one GPU",
              "label": "label_swap=True", "cap": "trace_capacity = 5 < NumSamples = 40", "unfinished": "no finished run_chains"}


@pytest.mark.parametrize("state", STATES)
def test_object_states(state):
    refused(f"reg_{state}", STATE_TEXT[state], 2)
    # the handle comes first, before the arguments; the trace's state last, after the rows
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "m = -1", -1)
    refused(f"reg_{state}", STATE_TEXT[state] if state in ("none", "sharded") else "x must be", 2, "valid")
    if state in ("none", "sharded"):
        refused(f"reg_{state}", STATE_TEXT[state], 2, weights=W)
        refused(f"reg_{state}", STATE_TEXT[state], 2, values=VALUES)
    else:                                                               # weights= and values= need no finished trace
        _, calls, pc = run(f"reg_{state}", 2, weights=W)
        assert len(calls) == 1 and pc.n_samples == 6
        _, calls, pc = run(f"reg_{state}", 2, values=VALUES)
        assert len(calls) == 1 and pc.n_samples == 8


def test_every_raise_of_the_module_is_reached():
    path = inspect.getsourcefile(compress)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) >= 9
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
    print(f"{len(sites)} raise sites in compress.py, {len(sites) - len(missed)} reached")
    assert missed == set()
