"""Classification report (ParallelTemperingBase.classification_report: confusion counts, per-class scores and one-vs-rest ROC-AUC
of every sampled net) timed on the BASELINE classifier of predict_probe.py:

  config 4  Ionosphere 34-50-2 x 256 chains, S = 2 000, random walk (bench.py ionosphere256's net)

On the train rows, all chains, burn-in 0.5 -- a pooled selection of more than 10^4 distinct samples: wall time of the whole call
(host clock around a call that synchronises; one untimed call first; minimum of --reps calls) with auc=True and auc=False, beside
posterior_predictive on the same selection (the forward pass and the reduction of the pooled classifier, which the report contains),
n_distinct / n_samples, and the float64 numpy reference (tests/report_ref.py) on the host, timed on the device's own outputs of
--ref-samples of the samples and extrapolated to all distinct ones (labelled so).  One JSON line, appended to --out.

    python profiles/tools/report_probe.py [--reps 3] [--ref-samples 64] [--rows train] [--out profiles/report_probe.jsonl]

The per-kernel split comes from a run of its own:  rocprofv3 --kernel-trace --stats -- python profiles/tools/report_probe.py
--reps 1 --ref-samples 0
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed calls per variant; the minimum is reported")
    ap.add_argument("--ref-samples", type=int, default=64, help="samples the host reference is timed on (0 = skip)")
    ap.add_argument("--rows", default="train", choices=("train", "test"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ptnn_amd.pt_classification import ParallelTempering
    c = CASES["4"]
    d = parity.datasets()
    train, test = d[c["data"] + "_train"], d[c["data"] + "_test"]
    rows = train if a.rows == "train" else test
    R, S, K = c["R"], c["S"], c["topo"][2]
    with tempfile.TemporaryDirectory() as tmp:
        pt = ParallelTempering(c["lg"], c["lr"], train, test, list(c["topo"]), R, c["maxtemp"], R * S, 100, tmp, seed=7, write_files=False)
        pt.initialize_chains(0.5)
        pt.run_chains()
        desc = pt._sampler.describe()
        rep, t_auc = timed(lambda: pt.classification_report(a.rows), a.reps)
        _, t_plain = timed(lambda: pt.classification_report(a.rows, auc=False), a.reps)
        _, t_pred = timed(lambda: pt.posterior_predictive(a.rows), a.reps)
        U, M, n_rows = rep.n_distinct, rep.n_samples, len(rows)
        line = dict(case=c["name"], rows=a.rows, n_rows=n_rows, chains=R, S=S, kernel=desc.get("kernel"), n_samples=M, n_distinct=U,
                    distinct_ratio=round(U / M, 5), wall_s_min_report_with_auc=round(t_auc, 6), wall_s_min_report_without_auc=round(t_plain, 6),
                    wall_s_min_posterior_predictive=round(t_pred, 6),
                    sample_class_rankings_per_s_from_the_difference=round(U * K / max(t_auc - t_plain, 1e-9), 1),
                    accuracy=round(rep.metrics["accuracy"], 6), balanced_accuracy_mean=round(rep.metric_mean["balanced_accuracy"], 6),
                    macro_auc=round(rep.metrics["macro_auc"], 6), macro_auc_mean=round(rep.metric_mean["macro_auc"], 6),
                    macro_auc_5_95=[round(float(rep.metric_percentiles[q]["macro_auc"]), 6) for q in (5, 95)])
        if a.ref_samples > 0:
            import report_ref as ref
            n = min(a.ref_samples, M)
            w = pt._sampler.traces(int(S * 0.5), n)["pos_w"][0]                  # the first chain's first rows of the selection
            pp = pt.posterior_predictive(a.rows, weights=w, return_samples=True)
            y = rows[:, c["topo"][0]].astype(np.int64)
            t0 = time.perf_counter()
            r = ref.report(pp.samples, np.ones(n, np.int64), y, K)
            t_ref = time.perf_counter() - t0
            got = pt.classification_report(a.rows, weights=w)
            line.update(host_reference_samples_timed=n, host_reference_s_per_sample=round(t_ref / n, 6),
                        host_reference_s_all_distinct_extrapolated=round(t_ref / n * U, 2),
                        sample_metrics_equal_on_those=bool(np.array_equal(got.sample_metrics, r["sample_metrics"], equal_nan=True)))
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        pt._sampler.close()


if __name__ == "__main__":
    main()
