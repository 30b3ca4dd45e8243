"""Predictive accuracy (ParallelTemperingBase.predictive_accuracy: lppd, WAIC, PSIS-LOO) timed on the BASELINE shapes of
predict_probe.py:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net)

For each case and row set ("train", "test"), all chains, burn-in 0.5, r_eff = 1: wall time of the whole call (host clock around a
call that synchronises; one untimed call first; minimum and median of --reps calls), n_distinct / n_samples, the PSIS tail length
M, and the largest k-hat and the number of rows above good_k.  One JSON line per (case, rows); --out writes them to a file as well.

    python profiles/tools/elpd_probe.py [--cases 1,4,5] [--reps 3] [--out profiles/elpd_probe.jsonl]
"""
import argparse
import json
import math
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
    "1": dict(name="config1_sunspot_4_5_1_x64", task=0, topo=(4, 5, 1), data="sunspot", R=64, lg=True, lr=0.1, maxtemp=2, S=10000),
    "4": dict(name="config4_ionosphere_34_50_2_x256", task=1, topo=(34, 50, 2), data="ions", R=256, lg=False, lr=0.01, maxtemp=10, S=2000),
    "5": dict(name="config5_synthetic_32_512_1_x128", task=0, topo=(32, 512, 1), data="synthetic512", R=128, lg=True, lr=0.1, maxtemp=2, S=201),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per (case, rows); the minimum and the median are reported")
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
            desc = pt._sampler.describe()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for rows in ("train", "test"):
                    pt.predictive_accuracy(rows)                                # first call: code objects, allocations
                    ts = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        pa = pt.predictive_accuracy(rows)                       # returns after the device has finished
                        ts.append(time.perf_counter() - t0)
                    U, M = pa.n_distinct, pa.n_samples
                    fin = pa.khat[np.isfinite(pa.khat)]
                    line = dict(case=c["name"], rows=rows, n_rows=int(pa.lppd_i.size), chains=R, S=S, kernel=desc.get("kernel"),
                                compact_traces=desc.get("compact_traces"), n_samples=M, n_distinct=U, distinct_ratio=round(U / M, 5),
                                psis_tail_M=int(math.ceil(min(0.2 * M, 3 * math.sqrt(M)))),
                                elpd_wall_s_min=round(min(ts), 6), elpd_wall_s_median=round(float(np.median(ts)), 6),
                                elpd_loo=round(pa.elpd_loo, 4), elpd_waic=round(pa.elpd_waic, 4), lppd=round(pa.lppd, 4),
                                khat_max=round(float(fin.max()), 4) if fin.size else None, n_high_k=pa.n_high_k,
                                good_k=round(pa.good_k, 4))
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
