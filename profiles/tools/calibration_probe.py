"""Calibration (ParallelTemperingBase.predictive_calibration: PIT, quantiles, CRPS; Brier / reliability) timed on the BASELINE
shapes of predict_probe.py:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net)

For each case on the test rows, all chains, burn-in 0.5: wall time of the whole call (host clock around a call that synchronises;
one untimed call first; minimum of --reps calls), with and without the pair term of the CRPS (regressions), n_distinct /
n_samples, the pair terms per second that the difference of the two implies, and the float64 oracle (tests/calibration_ref.py)
on the host, timed on --ref-rows rows of the device's own outputs (runs of equal samples merged) and extrapolated to all rows
(labelled so).  A selection of
more than 65536 distinct samples is thinned until it fits (the thin used is recorded).  One JSON line per case, appended to --out.

    python profiles/tools/calibration_probe.py [--cases 1,4,5] [--reps 3] [--ref-rows 2] [--out profiles/calibration_probe.jsonl]

The per-kernel split comes from a run of its own:  rocprofv3 --kernel-trace --stats -- python profiles/tools/calibration_probe.py
--cases 1 --reps 1 --ref-rows 0
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity  # noqa: E402
from elpd_probe import CASES  # noqa: E402


def timed(fn, reps):
    fn()                                                                        # first call: code objects, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()                                                              # returns after the device has finished
        ts.append(time.perf_counter() - t0)
    return out, min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per variant; the minimum is reported")
    ap.add_argument("--ref-rows", type=int, default=2, help="rows the host oracle is timed on (0 = skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ptnn_amd import _lib
    for key in a.cases.split(","):
        c = CASES[key]
        if c["data"] == "synthetic512":
            train, test = parity.synthetic_regression(1280, 1024, 32, 512, seed=5)
        else:
            d = parity.datasets()
            train, test = d[c["data"] + "_train"], d[c["data"] + "_test"]
        R, S = c["R"], c["S"]
        with tempfile.TemporaryDirectory() as tmp:
            if c["task"] == 0:
                from ptnn_amd.pt_timeseries_regression import ParallelTempering
                pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, 100, 0.5, tmp, seed=7,
                                       write_files=False)
            else:
                from ptnn_amd.pt_classification import ParallelTempering
                pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, 100, tmp, seed=7,
                                       write_files=False)
            pt.initialize_chains(0.5)
            pt.run_chains()
            desc = pt._sampler.describe()
            thin = 1
            while pt.predictive_calibration("test", thin=thin, crps=False).n_distinct > _lib.CALIB_MAX_DISTINCT:
                thin += 1
            cal0, t_row = timed(lambda: pt.predictive_calibration("test", thin=thin, crps=False), a.reps)
            U, M, n_rows = cal0.n_distinct, cal0.n_samples, len(test)
            line = dict(case=c["name"], rows="test", n_rows=n_rows, chains=R, S=S, thin=thin, kernel=desc.get("kernel"),
                        compact_traces=desc.get("compact_traces"), n_samples=M, n_distinct=U, distinct_ratio=round(U / M, 5),
                        wall_s_min_without_pair_term=round(t_row, 6))
            if c["task"] == 0:
                cal, t_all = timed(lambda: pt.predictive_calibration("test", thin=thin), a.reps)
                tiles = -(-U // 256)
                pairs = n_rows * (tiles * (tiles + 1) // 2) * 256 * 256             # A evaluations the pair kernel makes
                line.update(wall_s_min_with_pair_term=round(t_all, 6), pair_evaluations=pairs,
                            pair_evaluations_per_s_from_the_difference=round(pairs / max(t_all - t_row, 1e-9), 1),
                            crps=round(cal.crps, 6), se_crps=round(cal.se_crps, 6),
                            coverage={str(k): round(v, 4) for k, v in cal.coverage.items()})
                if a.ref_rows > 0:
                    import calibration_ref as ref
                    pp = pt.posterior_predictive(test[:a.ref_rows, :c["topo"][0]], thin=thin, return_samples=True)
                    eta = pt._sampler.eta_trace()[:, int(S * 0.5)::thin].reshape(-1)
                    y = test[:a.ref_rows, c["topo"][0]].astype(np.float32).astype(np.float64)
                    # runs of consecutive samples equal in (outputs on these rows, eta): the oracle's distinct samples and counts
                    fx, e32 = np.ascontiguousarray(pp.samples[:, :, 0]), np.ascontiguousarray(eta, np.float32)
                    new = np.ones(fx.shape[0], bool)
                    new[1:] = np.any(fx[1:].view(np.uint32) != fx[:-1].view(np.uint32), axis=1) | (e32[1:].view(np.uint32) != e32[:-1].view(np.uint32))
                    starts = np.flatnonzero(new)
                    counts = np.diff(np.append(starts, fx.shape[0]))
                    t0 = time.perf_counter()
                    r = ref.rows(fx[starts], y, e32[starts], counts)
                    t_ref = time.perf_counter() - t0
                    line.update(host_oracle_rows_timed=a.ref_rows, host_oracle_s_per_row=round(t_ref / a.ref_rows, 4),
                                host_oracle_s_all_rows_extrapolated=round(t_ref / a.ref_rows * n_rows, 2),
                                crps_max_rel_err_on_those_rows=float(np.max(np.abs(cal.crps_i[:a.ref_rows] / r["crps"] - 1.0))))
            else:
                line.update(brier=round(cal0.brier, 6), log_score=round(cal0.log_score, 6), ece=round(cal0.ece, 6), mce=round(cal0.mce, 6))
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            pt._sampler.close()


if __name__ == "__main__":
    main()
