"""Rank-normalised diagnostics (ParallelTemperingBase.rank_diagnostics) timed beside convergence_diagnostics on the cases of
convergence_probe.py (configs 1, 4 and 5: all chains, burn-in 0.5, every weight plus the likelihood).  Wall time of each call (host
clock around a call that synchronises; one untimed call first, the minimum of --reps).  One JSON line per case; --out writes them
to a file as well.  For the kernel split run it under `rocprofv3 --kernel-trace --stats` with --reps 1.

    python profiles/tools/rank_probe.py [--cases 1,4,5] [--out profiles/rank_probe.jsonl]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity  # noqa: E402
from convergence_probe import CASES  # noqa: E402


def timed(f, reps):
    f()                                                                         # first call: code objects, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()                                                               # returns after the device has finished
        ts.append(time.perf_counter() - t0)
    return out, min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
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
            cd, t_cd = timed(pt.convergence_diagnostics, a.reps)
            rd, t_rd = timed(pt.rank_diagnostics, a.reps)
            _, t_pc = timed(lambda: pt.rank_diagnostics(per_chain=True), a.reps)
            fin = np.isfinite(rd.r_hat)
            line = dict(case=c["name"], chains=rd.n_chains, draws_per_chain=rd.n_draws, quantities=len(rd.names),
                        pooled_draws=2 * rd.n_chains * (rd.n_draws // 2), convergence_s=round(t_cd, 6), rank_s=round(t_rd, 6),
                        rank_per_chain_s=round(t_pc, 6), r_hat_median=round(float(np.median(rd.r_hat[fin])), 4) if fin.any() else None,
                        classic_r_hat_median=round(float(np.nanmedian(cd.r_hat)), 4), ess_bulk_likelihood=float(rd.ess_bulk[-1]),
                        ess_tail_likelihood=float(rd.ess_tail[-1]), classic_ess_likelihood=float(cd.ess[-1]))
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
