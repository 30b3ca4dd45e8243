"""Prior predictive check (ParallelTemperingBase.prior_predictive) timed on the three BASELINE shapes:

  config 1  Sunspot 4-5-1 (bench.py sunspot64's net), train rows
  config 4  Ionosphere 34-50-2 (bench.py ionosphere256's net), train rows
  config 5  synthetic 32-512-1 (bench.py synthetic512's net; a vector is 70 KB), train rows

at 4 096 draws x 4 prior scales (0.25, 1, 4, 25), percentiles (5, 50, 95), on the handle initialize_chains() makes (4 chains: the
call does not look at them).  Wall time of the whole call: a host clock around a call that synchronises, one untimed call first,
the minimum of `--reps` (3).  Beside it the host numpy forward pass over the same drawn vectors, timed on `--cpu-draws` (256) draws
of one scale and scaled to all draws and scales: an order of magnitude only -- it leaves out every reduction.  One JSON line per
case; --out writes them to a file as well.

    python profiles/tools/prior_probe.py [--cases 1,4,5] [--out profiles/prior_probe.jsonl]
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
from predict_probe import numpy_forward  # noqa: E402

CASES = {
    "1": dict(name="config1_sunspot_4_5_1", task=0, topo=(4, 5, 1), data="sunspot"),
    "4": dict(name="config4_ionosphere_34_50_2", task=1, topo=(34, 50, 2), data="ions"),
    "5": dict(name="config5_synthetic_32_512_1", task=0, topo=(32, 512, 1), data="synthetic512"),
}
SCALES = (0.25, 1.0, 4.0, 25.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--cpu-draws", type=int, default=256, help="draws the numpy forward pass is timed over (then scaled)")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per case; the minimum is reported")
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
        I, H, O = c["topo"]
        with tempfile.TemporaryDirectory() as tmp:
            if c["task"] == 0:
                from ptnn_amd.pt_timeseries_regression import ParallelTempering
                pt = ParallelTempering(True, 0.1, train, test, list(c["topo"]), 4, 2, 4 * 50, 10, 0.5, tmp, seed=7, write_files=False)
            else:
                from ptnn_amd.pt_classification import ParallelTempering
                pt = ParallelTempering(False, 0.01, train, test, list(c["topo"]), 4, 10, 4 * 50, 10, tmp, seed=7, write_files=False)
            pt.initialize_chains(0.5)
            call = lambda **kw: pt.prior_predictive("train", n_draws=a.draws, sigma_squared=SCALES, percentiles=(5, 50, 95), **kw)  # noqa: E731
            call()                                                              # first call: code objects, allocations
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = call()                                                    # returns after the device has finished
                ts.append(time.perf_counter() - t0)
            k = min(a.cpu_draws, a.draws)
            W = pt.prior_predictive("train", n_draws=k, sigma_squared=SCALES[-1], return_weights=True).weights[0].astype(np.float64)
            X = np.asarray(train, dtype=np.float64)[:, :I]
            t0 = time.perf_counter()
            numpy_forward(c["task"], X, W, c["topo"])
            t_cpu = time.perf_counter() - t0
            line = dict(case=c["name"], rows="train", n_rows=X.shape[0], n_draws=a.draws, scales=list(SCALES), n_param=pt.num_param,
                        prior_wall_s_min=round(min(ts), 6), prior_wall_s_all=[round(t, 6) for t in ts],
                        forward_flop=2 * a.draws * len(SCALES) * X.shape[0] * (I * H + H * O),
                        saturated_share={str(s): round(float(res.saturated[j].mean()), 4) for j, s in enumerate(SCALES)},
                        numpy_draws_timed=k, numpy_forward_s_order_of_magnitude=round(t_cpu * a.draws * len(SCALES) / k, 3))
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
