"""Convergence diagnostics (ParallelTemperingBase.convergence_diagnostics) timed on the shapes of predict_probe.py:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net)

For each case: all chains, burn-in 0.5, every weight plus the likelihood.  Wall time of the call (host clock around a call that
synchronises; one untimed call first, the minimum of --reps), the truncation lags, the FP64 FMAs the lag kernel issued -- for each
quantity 2C split chains x the draws each 64-lag tile reads x the lags its blocks covered (64, 128, 256, 512, 512, ... until its
last sequence closed) -- against the h^2 / 2 per split chain a full-lag evaluation needs, and the float64 numpy oracle (tests/convergence_ref.py, FFT
autocovariance) on the same draws, timed over the first --oracle-quantities quantities and scaled to all of them (its order of
magnitude, not a speed-up claim).  One JSON line per case; --out writes them to a file as well.

    python profiles/tools/convergence_probe.py [--cases 1,4,5] [--out profiles/convergence_probe.jsonl]
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

import convergence_ref  # noqa: E402
import parity  # noqa: E402

CASES = {
    "1": dict(name="config1_sunspot_4_5_1_x64", task=0, topo=(4, 5, 1), data="sunspot", R=64, lg=True, lr=0.1, maxtemp=2, S=10000),
    "4": dict(name="config4_ionosphere_34_50_2_x256", task=1, topo=(34, 50, 2), data="ions", R=256, lg=False, lr=0.01, maxtemp=10, S=2000),
    "5": dict(name="config5_synthetic_32_512_1_x128", task=0, topo=(32, 512, 1), data="synthetic512", R=128, lg=True, lr=0.1, maxtemp=2, S=201),
}


def lags_covered(max_t, h):
    """Lags the host loop's blocks (64, 128, 256, then 512 each, capped at h) computed for a quantity whose sequences closed at
    max_t: the pair loop reads rho up to max_t + 2."""
    need, t0, nl = max_t + 2, 0, 64
    while True:
        nl = min(nl, -(-(h - t0) // 64) * 64)
        t0 += nl
        if t0 > need or t0 >= h:
            return min(t0, h)
        nl = min(2 * nl, 512)


def fma_issued(max_t, h, C):
    """FP64 FMAs conv_lags_kernel issues for one quantity: every 64-lag tile below lags_covered runs its 2C split chains over the
    draws i < h - (first lag of the tile), in tiles of 32 draws, 64 FMAs per draw."""
    return sum(2 * C * 64 * min(h, -(-(h - tl0) // 32) * 32) for tl0 in range(0, lags_covered(max_t, h), 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-quantities", type=int, default=20, help="quantities the numpy oracle is timed over (then scaled)")
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
            pt.convergence_diagnostics()                                        # first call: code objects, allocations
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                cd = pt.convergence_diagnostics()                               # returns after the device has finished
                ts.append(time.perf_counter() - t0)
            Q, C, n = len(cd.names), cd.n_chains, cd.n_draws
            h = n // 2
            fma = sum(fma_issued(int(m), h, C) for m in cd.trunc_lag)
            fma_full = Q * 2 * C * h * h // 2
            # the oracle on the same draws: the first k quantities
            k = min(a.oracle_quantities, Q)
            b = S // 2
            tr = pt._sampler.traces(b, S - b)
            x = np.concatenate([tr["pos_w"][:, :, :k - 1], tr["likeh"][:, :, None]], axis=2).astype(np.float32)
            t0 = time.perf_counter()
            convergence_ref.diagnose_all(x)
            t_orc = (time.perf_counter() - t0) * Q / k
            fin = np.isfinite(cd.r_hat)
            line = dict(case=c["name"], chains=C, S=S, draws_per_chain=n, quantities=Q, kernel=desc.get("kernel"),
                        schedule=desc.get("schedule"), wall_s_min=round(min(ts), 6), wall_s_median=round(float(np.median(ts)), 6),
                        trunc_lag_median=int(np.median(cd.trunc_lag)), trunc_lag_max=int(cd.trunc_lag.max()),
                        r_hat_median=round(float(np.median(cd.r_hat[fin])), 4) if fin.any() else None,
                        r_hat_likelihood=float(cd.r_hat[-1]), ess_likelihood=float(cd.ess[-1]),
                        fp64_fma_issued=fma, fp64_fma_full_lags=fma_full, fma_ratio=round(fma / fma_full, 5),
                        oracle_quantities_timed=k, oracle_s_extrapolated=round(t_orc, 3))
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
