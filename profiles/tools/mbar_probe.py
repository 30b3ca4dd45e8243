"""MBAR over every rung (ParallelTemperingBase.rung_reweighting) timed after a bench-shaped run of each of the five bench.py workloads.

For each workload (bench.WORKLOADS: chains, S, proposals, maxtemp as bench.py runs them; seed 7), burn-in 0.5, thin 1, 2^20 prior
draws: wall time of the whole call (host clock around a call that synchronises; one untimed call first; minimum and median of
--reps calls), the sweeps of the fixed point to 1e-10 and its last residual, the Kish ESS of the reweighted sample against the
cold rung's split-ESS of U, the largest weight share, and log Z by MBAR beside the stepping-stone and thermodynamic-integration
estimates of log_evidence on the same draws.
One JSON line per workload; --out writes them to a file as well.

    python profiles/tools/mbar_probe.py [--workloads sunspot64,...] [--reps 3] [--max-iter 10000] [--out profiles/mbar_probe.jsonl]
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

import bench  # noqa: E402


def _timed(fn, reps):
    fn()                                                          # first call: code objects, allocations
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()                                                # returns after the device has finished
        ts.append(time.perf_counter() - t0)
    return out, min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(bench.WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prior-draws", type=int, default=1 << 20)
    ap.add_argument("--max-iter", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for key in a.workloads.split(","):
        c = bench.WORKLOADS[key]
        train, test, _ = bench.load_data(c["data"])
        R, S = c["R"], c["S"]
        with tempfile.TemporaryDirectory() as tmp:
            if c["task"] == 0:
                from ptnn_amd.pt_timeseries_regression import ParallelTempering
                pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, c["si"], 0.5, tmp,
                                       seed=7, write_files=False)
            else:
                from ptnn_amd.pt_classification import ParallelTempering
                pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, c["si"], tmp, seed=7,
                                       write_files=False)
            pt.initialize_chains(0.5)
            pt.run_chains()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                rw, t_min, t_med = _timed(lambda: pt.rung_reweighting(prior_draws=a.prior_draws, max_iter=a.max_iter), a.reps)
                ev = pt.log_evidence(prior_draws=a.prior_draws)
            line = dict(workload=key, chains=R, S=S, n_train=int(np.asarray(train).shape[0]), P=int(pt.num_param),
                        draws_per_rung=int(rw.cold_draws), items=int(rw.log_weights.size + a.prior_draws), prior_draws=a.prior_draws,
                        wall_s_min=round(t_min, 6), wall_s_median=round(t_med, 6), sweeps=int(rw.n_iter), residual=float(f"{rw.residual:.3g}"),
                        converged=bool(rw.residual <= 1e-10), kish_ess=round(rw.kish_ess, 2), cold_ess=round(float(rw.n_eff[-1]), 2),
                        ess_gain=round(rw.ess_gain, 3) if rw.ess_gain == rw.ess_gain else None, max_weight_share=float(f"{rw.max_weight_share:.3g}"),
                        log_z_mbar=round(rw.log_z_mbar, 4), se_log_z_mbar=round(rw.se_log_z_mbar, 4),
                        log_z_ss=round(ev.log_z_ss, 4), se_log_z_ss=round(ev.se_log_z_ss, 4), log_z_ti=round(ev.log_z_ti, 4),
                        se_log_z_ti=round(ev.se_log_z_ti, 4))
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
