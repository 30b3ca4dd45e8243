"""Posterior predictive (ParallelTemperingBase.posterior_predictive) timed on the three BASELINE shapes it is meant for:

  config 1  Sunspot 4-5-1 x 64 chains, S = 10 000, Langevin (bench.py sunspot64)
  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net; run_chains() hands the whole
            trace to the host twice -- float32 traces and the float64 posterior matrix, 3.8 GB each at this S)
  config 5  synthetic 32-512-1 x 128 chains, S = 201 (bench.py synthetic512's net; a row is 70 KB: 1.8 GB per host copy)

For each case and row set ("train", "test"), all chains, burn-in 0.5, percentiles (5, 95): wall time of the call (host clock around
a call that synchronises; one untimed call first), n_distinct / n_samples, the forward FLOPs 2 U N (I H + H O) over the distinct
vectors U and rows N, the bytes the order-statistic passes read (4 radix passes + the mean over U fp32 + U int32 per column), and
the host numpy forward pass of the same request -- every selected vector, no deduplication, what a user of the reference's drafts
runs (fx = forward over each posterior column) -- timed over the first `--cpu-vectors` vectors and scaled to all of them (marked
"extrapolated").  One JSON line per (case, rows); --out writes them to a file as well.

    python profiles/tools/predict_probe.py [--cases 1,4,5] [--out profiles/predict_probe.jsonl]
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
    "1": dict(name="config1_sunspot_4_5_1_x64", task=0, topo=(4, 5, 1), data="sunspot", R=64, lg=True, lr=0.1, maxtemp=2, S=10000),
    "4": dict(name="config4_ionosphere_34_50_2_x256", task=1, topo=(34, 50, 2), data="ions", R=256, lg=False, lr=0.01, maxtemp=10, S=2000),
    "5": dict(name="config5_synthetic_32_512_1_x128", task=0, topo=(32, 512, 1), data="synthetic512", R=128, lg=True, lr=0.1, maxtemp=2, S=201),
}


def numpy_forward(task, X, W, topo):
    """The reference's ForwardPass per sample (REG:51-55 / CLS:49-55; CLS softmax), float64: [n, rows, O]."""
    I, H, O = topo
    out = np.empty((W.shape[0], X.shape[0], O))
    for k, w in enumerate(W):
        W1 = w[:I * H].reshape(I, H)
        W2 = w[I * H:I * H + H * O].reshape(H, O)
        B1 = w[I * H + H * O:I * H + H * O + H]
        B2 = w[I * H + H * O + H:]
        hid = 1.0 / (1.0 + np.exp(-(X @ W1 - B1)))
        o = 1.0 / (1.0 + np.exp(-(hid @ W2 - B2)))
        if task == 1:
            e = np.exp(o)
            o = e / e.sum(axis=1, keepdims=True)
        out[k] = o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,5")
    ap.add_argument("--cpu-vectors", type=int, default=2000, help="vectors the numpy baseline is timed over (then scaled)")
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
        I, H, O = c["topo"]
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
            t0 = time.perf_counter()
            res = pt.run_chains()
            t_run = time.perf_counter() - t0
            desc = pt._sampler.describe()
            for rows in ("train", "test"):
                X = np.asarray(train if rows == "train" else test, dtype=np.float64)[:, :I]
                N = X.shape[0]
                pt.posterior_predictive(rows)                                   # first call: code objects, allocations
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    pred = pt.posterior_predictive(rows)                        # returns after the device has finished
                    ts.append(time.perf_counter() - t0)
                U, M = pred.n_distinct, pred.n_samples
                k = min(a.cpu_vectors, M)
                W = res[0][:, :k].T
                t0 = time.perf_counter()
                fx = numpy_forward(c["task"], X, W, c["topo"])
                t_cpu_k = time.perf_counter() - t0
                t_cpu_pct = 0.0
                if k == M:                                                      # the full request: the percentile step too
                    t0 = time.perf_counter()
                    fx.mean(axis=0)
                    np.percentile(fx, [5, 95], axis=0)
                    t_cpu_pct = time.perf_counter() - t0
                line = dict(case=c["name"], rows=rows, n_rows=N, chains=R, S=S, run_chains_s=round(t_run, 4), kernel=desc.get("kernel"),
                            compact_traces=desc.get("compact_traces"), n_samples=M, n_distinct=U, distinct_ratio=round(U / M, 5),
                            predict_wall_s_min=round(min(ts), 6), predict_wall_s_median=round(float(np.median(ts)), 6),
                            forward_flop=2 * U * N * (I * H + H * O), forward_flop_no_dedup=2 * M * N * (I * H + H * O),
                            select_bytes=(4 + 1) * U * N * O * 8,
                            numpy_vectors_timed=k, numpy_forward_s=round(t_cpu_k * M / k + t_cpu_pct, 4),
                            numpy_extrapolated=k < M)
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
