"""Recursive multi-step forecasts (ParallelTemperingBase.forecast) timed on the BASELINE shapes:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 3  Mackey-Glass 4-10-1 x 64 chains, S = 10 000, Langevin (bench.py mackey64)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net; not a series: the recursion is timed only)

For each case, all chains, burn-in 0.5: origin "end" with h = 100, noise off and on, and origin "test" with h = 10, noise off.
Wall time of the whole call (host clock around a call that synchronises; one untimed call first; minimum and median of --reps
calls), trajectories, columns, the kernel layout, and the numpy baseline: the recursion a user would write on the downloaded
vectors (per sample, per step one forward pass of the window), timed on --cpu-trajectories trajectories and extrapolated
linearly to the call's trajectory count.  One JSON line per (case, request); --out writes them to a file as well.

    python profiles/tools/forecast_probe.py [--cases 1,3,5] [--reps 3] [--cpu-trajectories 50] [--out profiles/forecast_probe.jsonl]
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
from parity import orc  # noqa: E402

CASES = {
    "1": dict(name="config1_sunspot_4_5_1_x64", topo=(4, 5, 1), data="sunspot", R=64, lg=True, lr=0.1, maxtemp=2, S=10000),
    "3": dict(name="config3_mackey_4_10_1_x64", topo=(4, 10, 1), data="mackey", R=64, lg=True, lr=0.1, maxtemp=2, S=10000),
    "5": dict(name="config5_synthetic_32_512_1_x128", topo=(32, 512, 1), data="synthetic512", R=128, lg=True, lr=0.1, maxtemp=2, S=201),
}
REQUESTS = [("end", 100, False), ("end", 100, True), ("test", 10, False)]
FC_LANE_MAX_P = 96          # csrc/ptnn_dev_forecast.hpp: the lane layout up to 96 parameters


def numpy_seconds(w, origins, h, topo, n):
    """Seconds of the numpy recursion over n trajectories (w[:n]) from every origin."""
    w = np.asarray(w[:n], np.float64)
    win0 = np.asarray(origins, np.float64)
    t0 = time.perf_counter()
    for v in range(w.shape[0]):
        for r in range(win0.shape[0]):
            win = win0[r].copy()
            for _ in range(h):
                y = orc.forward(win[None], w[v], topo)[1][0, 0]
                win = np.append(win[1:], y)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,3,5")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per request; the minimum and the median are reported")
    ap.add_argument("--cpu-trajectories", type=int, default=50, help="trajectories the numpy baseline is timed on (0: none)")
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
        R, S, topo = c["R"], c["S"], c["topo"]
        P = topo[0] * topo[1] + topo[1] * topo[2] + topo[1] + topo[2]
        with tempfile.TemporaryDirectory() as tmp:
            from ptnn_amd.pt_timeseries_regression import ParallelTempering
            pt = ParallelTempering(c["lg"], c["lr"], train, test, list(topo), R, c["maxtemp"], R * S, 100, 0.5, tmp, seed=7,
                                   write_files=False)
            pt.initialize_chains(0.5)
            pt.run_chains()
            desc = pt._sampler.describe()
            w_all = None
            for origin, h, noise in REQUESTS:
                line = dict(case=c["name"], origin=origin, horizon=h, noise=noise, chains=R, S=S, kernel=desc.get("kernel"),
                            compact_traces=desc.get("compact_traces"), layout="lane" if P <= FC_LANE_MAX_P else "split")
                try:
                    pt.forecast(h, origin, noise=noise)                         # first call: code objects, allocations
                except Exception as e:                                          # noqa: BLE001  (e.g. rows without eta)
                    line["error"] = str(e)[:300]
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    continue
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fc = pt.forecast(h, origin, noise=noise)                    # returns after the device has finished
                    ts.append(time.perf_counter() - t0)
                n_org = fc.mean.shape[0]
                line.update(n_origins=n_org, n_samples=fc.n_samples, n_trajectories=fc.n_trajectories,
                            columns=n_org * h, forward_passes=fc.n_trajectories * n_org * h,
                            forecast_wall_s_min=round(min(ts), 6), forecast_wall_s_median=round(float(np.median(ts)), 6),
                            mean_last=round(float(fc.mean[-1, -1]), 6),
                            band_5_95_last=[round(float(fc.percentiles[5][-1, -1]), 6), round(float(fc.percentiles[95][-1, -1]), 6)])
                if a.cpu_trajectories > 0:
                    if w_all is None:
                        w_all = pt._sampler.traces(S // 2, S - S // 2)["pos_w"].reshape(-1, P)
                    origins = (np.asarray(test)[-1:, 1:topo[0] + 1] if origin == "end" else np.asarray(test)[:, :topo[0]])
                    n = min(a.cpu_trajectories, w_all.shape[0])
                    # the test-row request: a tenth of the origins timed (the recursion is the same per origin)
                    sub = origins if origin == "end" else origins[:max(1, origins.shape[0] // 10)]
                    t = numpy_seconds(w_all, sub, h, topo, n)
                    scale = fc.n_trajectories / n * origins.shape[0] / sub.shape[0]
                    line.update(numpy_timed_trajectories=n, numpy_timed_origins=int(sub.shape[0]),
                                numpy_s_extrapolated=round(t * scale, 3),
                                numpy_s_extrapolated_all_samples=round(t * fc.n_samples / n * origins.shape[0] / sub.shape[0], 3))
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
