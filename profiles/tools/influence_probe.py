"""Timing record of case_influence: one setting per fresh process under its own time limit; in it a warm-up
call, then timed calls, beside the float64 numpy reference (tests/influence_ref.py) on the same arrays -- the device's own
expanded outputs and pointwise log-likelihoods of the selection -- on this machine's CPU share.  Recorded, not gated.  The
library must have been built.

    python profiles/tools/influence_probe.py [--out FILE]                # both settings -> profiles/influence_timing.json
    rocprofv3 --kernel-trace --stats -d DIR -o run -f csv -- python profiles/tools/influence_probe.py --child sunspot --no-cpu
                                                                          # the kernels' own times, a run of its own

Settings: Sunspot 4-5-1, case_influence("test", "train") (198 target rows, 298 cases) on the full posterior matrix of the
README's run (64 replicas, 640 000 samples, burn-in 0.5); and the Ionosphere shape 34-50-2 (synthetic rows of that shape: 234
train, 117 test) with 1000 distinct weight vectors.  flops = 2 n_a n_b U: the covariance kernel's multiply-adds alone."""
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "profiles", "influence_timing.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIMIT = 420                                                              # seconds per child
REPS = 5
IONO_U = 1000


def _timed(fn, reps=REPS):
    fn()                                                                 # warm-up: code objects loaded, buffers touched
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return times, out


def _record(setting, pt, cpu, **src):
    import numpy as np
    import influence_ref as ref
    times, ci = _timed(lambda: pt.case_influence("test", "train", **src))
    n_a, n_b = int(np.prod(ci.cov.shape[:-1])), int(ci.cov.shape[-1])
    rec = dict(setting=setting, n_a=n_a, n_b=n_b, n_samples=int(ci.n_samples), n_distinct=int(ci.n_distinct), gpu_seconds=times,
               flops=2.0 * n_a * n_b * ci.n_distinct, top_case_of_row_0=int(ci.top_cases.reshape(-1, ci.top_cases.shape[-1])[0, 0]))
    if cpu:
        pred = pt.posterior_predictive("test", return_samples=True, **{k: v for k, v in src.items() if k != "eta"})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            acc = pt.predictive_accuracy("train", return_pointwise=True, **src)
        A = pred.samples.reshape(pred.samples.shape[0], -1)
        cpu_times, r = _timed(lambda: ref.influence(A, acc.log_lik), reps=2)
        s_a, s_b = np.sqrt(r["target_var"]), np.sqrt(r["case_var"])
        share = np.abs(ci.cov.reshape(n_a, n_b) - r["cov"]) / ref.tol(ci.n_samples, s_a, s_b)     # both within the bound: U <= S
        rec.update(cpu_seconds=cpu_times, cpu_threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or None,
                   cpu_arrays=f"float32 [{A.shape[0]}, {n_a}] and float64 [{A.shape[0]}, {n_b}], expanded",
                   largest_gap_to_numpy_as_share_of_bound=float(share.max()))
    return rec


def sunspot_child(cpu):
    import parity
    import ptnn_amd  # noqa: F401
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    d = parity.datasets()
    pt = ParallelTempering(True, 0.1, d["sunspot_train"], d["sunspot_test"], [4, 5, 1], 64, 2, 640000, 100, 0.5, tempfile.mkdtemp(), seed=1,
                           write_files=False)
    pt.initialize_chains(0.5)
    pt.run_chains()
    return _record("sunspot 4-5-1, the full posterior matrix", pt, cpu)


def ionosphere_child(cpu):
    from parity import orc
    from test_gpu_analysis_shapes import _data, _vectors
    from test_gpu_predict import _pt
    topo = (34, 50, 2)
    train, test = _data(orc.TASK_CLS, topo, 1, n_tr=234, n_te=117)
    pt = _pt(orc.TASK_CLS, topo, train, test, 4, 20, tempfile.mkdtemp(), lr=0.01, maxtemp=10)
    return _record("ionosphere 34-50-2, 1000 vectors", pt, cpu, weights=_vectors(topo, IONO_U, 2))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps({"sunspot": sunspot_child, "ionosphere": ionosphere_child}[sys.argv[2]]("--no-cpu" not in sys.argv)), flush=True)
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    record = json.load(open(out)) if os.path.exists(out) else {}
    for name in ("sunspot", "ionosphere"):                              # a fresh process each; the first failure ends the probe
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True, timeout=LIMIT)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            return p.returncode
        record[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, record[name]["gpu_seconds"], record[name].get("cpu_seconds"), flush=True)
    with open(out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
