"""Posterior predictive checks (ParallelTemperingBase.predictive_check: replicated data, test quantities, p-values) timed on
the BASELINE shapes of predict_probe.py:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net)

For each case on the test rows, all chains, burn-in 0.5: wall time of the whole call (host clock around a call that synchronises;
one untimed call first; minimum of --reps calls), n_distinct / n_samples, replicated values per second, the p-values, and the
float64 oracle (tests/ppc_ref.py) on the host, timed on the first --ref-occ occurrences of the device's own outputs and
extrapolated to all occurrences (labelled so).  One JSON line per case, appended to --out.

    python profiles/tools/ppc_probe.py [--cases 1,4,5] [--reps 3] [--ref-occ 64] [--out profiles/ppc_probe.jsonl]
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
from calibration_probe import timed  # noqa: E402
from elpd_probe import CASES  # noqa: E402

LAGS = (1, 2, 3, 4, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--reps", type=int, default=3, help="timed calls; the minimum is reported")
    ap.add_argument("--ref-occ", type=int, default=64, help="occurrences the host oracle is timed on (0 = skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ppc_ref as ref
    for key in a.cases.split(","):
        c = CASES[key]
        if c["data"] == "synthetic512":
            train, test = parity.synthetic_regression(1280, 1024, 32, 512, seed=5)
        else:
            d = parity.datasets()
            train, test = d[c["data"] + "_train"], d[c["data"] + "_test"]
        R, S, I = c["R"], c["S"], c["topo"][0]
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
            kw = dict(lags=LAGS) if c["task"] == 0 else {}
            chk, t_call = timed(lambda: pt.predictive_check("test", **kw), a.reps)
            U, M, n_rows = chk.n_distinct, chk.n_samples, len(test)
            line = dict(case=c["name"], rows="test", n_rows=n_rows, chains=R, S=S, kernel=desc.get("kernel"),
                        compact_traces=desc.get("compact_traces"), n_samples=M, n_distinct=U, distinct_ratio=round(U / M, 5),
                        n_stats=len(chk.names), wall_s_min=round(t_call, 6), replicated_values_per_s=round(M * n_rows / t_call, 1),
                        p_value={k: round(v, 4) for k, v in chk.p_value.items()})
            if a.ref_occ > 0:
                k = min(a.ref_occ, M // R)                                      # the first occurrences of the first chain
                pp = pt.posterior_predictive("test", chains=[0], return_samples=True)
                y = test[:, I].astype(np.float32).astype(np.float64)
                t0 = time.perf_counter()
                if c["task"] == 0:
                    eta = pt._sampler.eta_trace()[0, int(S * 0.5):][:k]
                    z = np.stack([ref.normals(pt.seed, i, n_rows) for i in range(k)])
                    ref.reduce(*ref.regression(pp.samples[:k, :, 0], eta, y, z, LAGS))
                else:
                    u = np.stack([ref.uniforms(pt.seed, i, n_rows) for i in range(k)])
                    ref.reduce(*ref.classification(pp.samples[:k], y.astype(np.int64), u)[:2])
                t_ref = time.perf_counter() - t0
                line.update(host_oracle_occurrences_timed=k, host_oracle_s_per_occurrence=round(t_ref / k, 6),
                            host_oracle_s_all_occurrences_extrapolated=round(t_ref / k * M, 2))
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            pt._sampler.close()


if __name__ == "__main__":
    main()
