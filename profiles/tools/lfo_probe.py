"""Leave-future-out cross-validation (ParallelTemperingBase.leave_future_out, ptnn_lfo) timed on the BASELINE shapes whose rows
are ordered in time, and on one that is not for the cost of the call alone:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 3  Mackey-Glass 4-10-1 x 64 chains, S = 10 000, Langevin (bench.py mackey64)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net; its rows have no order: call cost only)

For each case, all chains, burn-in 0.5, r_eff = 1, training rows, origins N // 2 .. N - 1, block 1 (protocol of elpd_probe.py:
host clock around a call that synchronises, one untimed call first, minimum and median of --reps calls):
  - the one device call that scores every origin from the first fit (refit=False), beside predictive_accuracy("train") on the
    same selection in the same run, and their ratio (both do one Pareto smoothing per row / origin over the same S);
  - configs 1 and 3: backward LFO at the default threshold with refits: the number of refits and the total wall time (once);
  - config 1 with --exact: exact LFO, a refit at every origin (k_threshold below every k-hat), once: the baseline it replaces.
One JSON line per case; --out writes them to a file as well.

    python profiles/tools/lfo_probe.py [--cases 1,3,5] [--reps 3] [--exact] [--out profiles/lfo_probe.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity  # noqa: E402

CASES = {
    "1": dict(name="config1_sunspot_4_5_1_x64", topo=(4, 5, 1), data="sunspot", R=64, S=10000, walk=True),
    "3": dict(name="config3_mackey_4_10_1_x64", topo=(4, 10, 1), data="mackey", R=64, S=10000, walk=True),
    "5": dict(name="config5_synthetic_32_512_1_x128", topo=(32, 512, 1), data="synthetic512", R=128, S=201, walk=False),
}


def _timed(fn, reps):
    fn()                                                                    # first call: code objects, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()                                                          # returns after the device has finished
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,3,5")
    ap.add_argument("--reps", type=int, default=3, help="timed calls; the minimum and the median are reported")
    ap.add_argument("--exact", action="store_true", help="config 1: also exact LFO, one refit per origin")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    lines = []
    for key in a.cases.split(","):
        c = CASES[key]
        if c["data"] == "synthetic512":
            train, test = parity.synthetic_regression(1280, 1024, 32, 512, seed=5)
        else:
            d = parity.datasets()
            train, test = d[c["data"] + "_train"], d[c["data"] + "_test"]
        R, S = c["R"], c["S"]
        with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pt = ParallelTempering(True, 0.1, train, test, list(c["topo"]), R, 2, R * S, 100, 0.5, tmp, seed=7, write_files=False)
            pt.initialize_chains(0.5)
            t0 = time.perf_counter()
            pt.run_chains()
            fit_s = time.perf_counter() - t0
            N = len(train)
            pa, t_pa = _timed(lambda: pt.predictive_accuracy("train"), a.reps)
            one, t_one = _timed(lambda: pt.leave_future_out(refit=False), a.reps)
            fin = one.khat[np.isfinite(one.khat)]
            line = dict(case=c["name"], n_rows=N, n_origins=int(one.origins.size), chains=R, S=S, n_samples=one.n_samples,
                        n_distinct=pa.n_distinct, first_fit_wall_s=round(fit_s, 4), k_threshold=round(one.k_threshold, 4),
                        lfo_call_wall_s_min=round(min(t_one), 6), lfo_call_wall_s_median=round(float(np.median(t_one)), 6),
                        elpd_call_wall_s_min=round(min(t_pa), 6), elpd_call_wall_s_median=round(float(np.median(t_pa)), 6),
                        lfo_over_elpd=round(min(t_one) / min(t_pa), 3), elpd_lfo_no_refit=round(one.elpd_lfo, 4),
                        elpd_loo_same_rows=round(float(np.sum(pa.elpd_loo_i[N // 2:])), 4),
                        khat_max_no_refit=round(float(fin.max()), 4) if fin.size else None,
                        n_high_k_no_refit=int(np.count_nonzero(fin > one.k_threshold)))
            if c["walk"]:
                t0 = time.perf_counter()
                lfo = pt.leave_future_out()
                line.update(walk_wall_s=round(time.perf_counter() - t0, 4), n_refits=lfo.n_refits, refit_origins=[int(i) for i in lfo.refit_origins],
                            elpd_lfo=round(lfo.elpd_lfo, 4), se_elpd_lfo=round(lfo.se_elpd_lfo, 4))
            if a.exact and key == "1":
                t0 = time.perf_counter()
                ex = pt.leave_future_out(k_threshold=-1e300)
                line.update(exact_wall_s=round(time.perf_counter() - t0, 4), exact_n_refits=ex.n_refits, exact_elpd_lfo=round(ex.elpd_lfo, 4),
                            exact_se_elpd_lfo=round(ex.se_elpd_lfo, 4))
            print(json.dumps(line), flush=True)
            lines.append(line)
            pt._sampler.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
