"""Power-scaling sensitivity (ParallelTemperingBase.powerscale_sensitivity) timed on the BASELINE shapes of predict_probe.py:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net)

For each case on the test rows, all chains, burn-in 0.5, the default quantities, and the smallest thin in 1, 2, ... that keeps
the distinct samples under the cap and the PSIS tail under its bound (recorded; a refused thin costs one refused call, an accepted
one the untimed call plus --reps timed calls): wall time of the whole call (host clock around a call that synchronises; one
untimed call first; minimum of --reps calls), n_distinct / n_samples, Q, quantity-values ordered per second, k-hat, the largest
sensitivities, and the float64 oracle (tests/powerscale_ref.py) on the host, timed on --ref-q random quantities with the
device's components, the same U and random multiplicities summing to M, and extrapolated to all Q (labelled so).  One JSON
line per case, appended to --out.

    python profiles/tools/powerscale_probe.py [--cases 1,4,5] [--reps 3] [--ref-q 8] [--out profiles/powerscale_probe.jsonl]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import parity  # noqa: E402
from calibration_probe import timed  # noqa: E402
from elpd_probe import CASES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--reps", type=int, default=3, help="timed calls; the minimum is reported")
    ap.add_argument("--ref-q", type=int, default=8, help="quantities the host oracle is timed on (0 = skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import powerscale_ref as ref
    from ptnn_amd import _lib
    warnings.simplefilter("ignore")
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
            groups = ["weights", "eta", "predictions"] if c["task"] == 0 else ["weights", "predictions"]
            sel, _ = pt._trace_selection(None, "all", 1)
            for thin in range(1, 9):
                sel["thin"] = thin
                try:
                    out, t_call = timed(lambda: pt._sampler.powerscale("test", groups=groups, **sel), a.reps)
                    break
                except _lib.PtnnError as e:
                    if "thin=" not in str(e) and "PSIS tail" not in str(e):
                        raise
            else:
                raise SystemExit(f"{c['name']}: every thin in 1 .. 8 was refused (distinct-sample cap or PSIS tail bound)")
            U, M, Q = out["n_distinct"], out["n_samples"], out["n_quantities"]
            top = np.argsort(-out["sens"][1])[:3]
            line = dict(case=c["name"], rows="test", n_rows=len(test), chains=R, S=S, thin=thin, kernel=desc.get("kernel"),
                        n_samples=M, n_distinct=U, n_quantities=Q, wall_s_min=round(t_call, 6),
                        values_ordered_per_s=round(Q * U / t_call, 1), khat=np.round(out["khat"], 3).tolist(),
                        tail_len=out["tail_len"].tolist(), prior_sens_max=float(np.max(out["sens"][1])),
                        prior_sens_median=float(np.median(out["sens"][1])), lik_sens_median=float(np.median(out["sens"][0])),
                        prior_sens_top=[int(t) for t in top])
            if a.ref_q > 0:
                rng = np.random.default_rng(0)
                counts = 1 + rng.multinomial(M - U, np.full(U, 1.0 / U))
                vals = rng.normal(0, 1, (a.ref_q, U)).astype(np.float32)
                t0 = time.perf_counter()
                ref.powerscale(vals, out["logp"], counts)
                t_ref = time.perf_counter() - t0
                line.update(host_oracle_quantities_timed=a.ref_q, host_oracle_s_per_quantity=round(t_ref / a.ref_q, 6),
                            host_oracle_s_all_quantities_extrapolated=round(t_ref / a.ref_q * Q, 2))
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            pt._sampler.close()


if __name__ == "__main__":
    main()
