"""Forecast verification (ParallelTemperingBase.forecast_accuracy / ptnn_forecast_score) timed on two shapes:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64), every 50th row: 6 400 trajectories (the pair
            terms take at most 65 536, and cost M^2 / 2 per column)
  32-96-1   the synthetic 32-96-1 net of the golden data x 16 chains, S = 2 000, every 4th row: 4 000 trajectories (not a
            series: host origins with random truth; the split layout of the forward kernel)

For each case, all chains, burn-in 0.5, noise on, the test rows as rolling origins, h = 10: the call with the pair term of the
CRPS and the energy score, with each alone, and with neither.  Wall time of the whole call (host clock around a call that
synchronises; one untimed call first; the minimum of --reps calls), trajectories, origins, columns, and the host reference:
tests/fscore_ref.py on the device's own means and samples of --ref-origins origins and the first --ref-trajectories
trajectories m of the call's M, timed once with and once without the pair terms; the O(M) part is scaled by M / m, the O(M^2)
part (the difference of the two timings) by (M / m)^2, and the sum linearly to all origins.  That is a double extrapolation
from single timings: an order of magnitude, not a ratio to quote to two digits.  One JSON line per (case, request); --out writes
them to a file as well.

    python profiles/tools/fscore_probe.py [--cases 1,96] [--reps 3] [--ref-origins 1] [--ref-trajectories 1000]
                                          [--out profiles/fscore_probe.jsonl]
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

CASES = {
    "1": dict(name="config1_sunspot_4_5_1_x64", topo=(4, 5, 1), data="sunspot", R=64, S=10000, thin=50, series=True),
    "96": dict(name="synth32_32_96_1_x16", topo=(32, 96, 1), data="synth32", R=16, S=2000, thin=4, series=False),
}
REQUESTS = [(True, True), (True, False), (False, True), (False, False)]        # (crps pair term, energy score)
H = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,96")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per request; the minimum is reported")
    ap.add_argument("--ref-origins", type=int, default=1, help="origins the host reference is timed on (0: none)")
    ap.add_argument("--ref-trajectories", type=int, default=1000, help="trajectories the host reference is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fscore_ref
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    from ptnn_amd.verification import series_from_windows, windows_and_truth
    lines = []
    for key in a.cases.split(","):
        c = CASES[key]
        d = parity.datasets()
        train, test = d[c["data"] + "_train"], d[c["data"] + "_test"]
        R, S, topo = c["R"], c["S"], c["topo"]
        I = topo[0]
        with tempfile.TemporaryDirectory() as tmp:
            pt = ParallelTempering(True, 0.1, train, test, list(topo), R, 2, R * S, 100, 0.5, tmp, seed=7, write_files=False)
            pt.initialize_chains(0.5)
            pt.run_chains()
            s = pt._sampler
            if c["series"]:
                series, stride = series_from_windows(np.asarray(test, np.float32), I)
                origins, truth = windows_and_truth(series, I, H, stride, n_origins=test.shape[0])
            else:
                origins = np.ascontiguousarray(test[:, :I], np.float32)
                truth = np.random.default_rng(1).uniform(0.1, 0.9, (test.shape[0], H)).astype(np.float32)
            sel = dict(step0=S // 2, nsteps=S - S // 2, thin=c["thin"])
            for crps, energy in REQUESTS:
                line = dict(case=c["name"], horizon=H, noise=True, chains=R, S=S, thin=c["thin"], crps=crps, energy=energy,
                            layout="lane" if pt.num_param <= 96 else "split")
                kw = dict(sel, noise=True, seed=7, quantiles=(0.05, 0.95), crps=crps, energy=energy)
                try:
                    out = s.forecast_score(H, origins, truth, **kw)                  # first call: code objects, allocations
                except Exception as e:                                               # noqa: BLE001
                    line["error"] = str(e)[:300]
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    continue
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out = s.forecast_score(H, origins, truth, **kw)                  # returns after the device has finished
                    ts.append(time.perf_counter() - t0)
                line.update(n_origins=int(origins.shape[0]), n_samples=out["n_samples"], n_trajectories=out["n_trajectories"],
                            columns=int(np.isfinite(truth).sum()), wall_s_min=round(min(ts), 6),
                            crps_h1=None if not crps else round(float(np.nanmean(out["crps"][:, 0])), 6),
                            crps_h10=None if not crps else round(float(np.nanmean(out["crps"][:, -1])), 6),
                            log_score_h1=round(float(np.nanmean(out["log_score"][:, 0])), 6),
                            energy_mean=None if not energy else round(float(np.nanmean(out["energy_score"])), 6))
                if a.ref_origins > 0:
                    n = min(a.ref_origins, origins.shape[0])
                    m = min(a.ref_trajectories, out["n_trajectories"])
                    sub = s.forecast_score(H, origins[:n], truth[:n], samples=True, means=True, **kw)
                    eta = s.eta_trace()[:, sel["step0"]::sel["thin"]].reshape(-1)[:m]
                    mu, ys = sub["means"][:m], sub["samples"][:m]
                    t0 = time.perf_counter()
                    fscore_ref.scores(mu, ys, eta, truth[:n], None, levels=(0.05, 0.95), crps=False, energy=False)
                    t_lin = time.perf_counter() - t0                                 # the O(M) part: grows with M
                    t_pair = 0.0
                    if crps or energy:                                               # the O(M^2) part: grows with M^2
                        t0 = time.perf_counter()
                        fscore_ref.scores(mu, ys, eta, truth[:n], None, levels=(0.05, 0.95), crps=crps, energy=energy)
                        t_pair = max(0.0, time.perf_counter() - t0 - t_lin)
                    g = out["n_trajectories"] / m
                    line.update(ref_timed_origins=n, ref_timed_trajectories=m,
                                ref_s_extrapolated=round((t_lin * g + t_pair * g * g) * origins.shape[0] / n, 1))
                print(json.dumps(line), flush=True)
                lines.append(line)
            s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
