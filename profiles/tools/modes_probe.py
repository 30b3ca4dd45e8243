"""Timing record of posterior_modes: one setting per fresh process under its own time limit; in it a warm-up
call, then timed calls, beside the float64 numpy restatement (tests/modes_ref.py: sq_float64 and density_peaks_rows) on the device's
own outputs on this machine's CPU share.  Recorded, not gated.  The library must have been built.

    python profiles/tools/modes_probe.py [--out FILE]                    # both settings -> profiles/modes_timing.json
    rocprofv3 --kernel-trace --stats -d DIR -o run -f csv -- python profiles/tools/modes_probe.py --child sunspot --no-cpu
                                                                          # the kernels' own times, a run of its own

Settings: Sunspot 4-5-1, posterior_modes("test") (198 rows) on the full posterior matrix of the README's run (64 replicas, 640 000
samples, burn-in 0.5: about 4000 distinct samples); and the Ionosphere shape 34-50-2 (synthetic rows of that shape: 234 train, 117
test) with 1000 distinct weight vectors.  flops = 3 n U (U + 1) / 2: a subtraction and a fused multiply-add per column and pair
of the upper triangle."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "profiles", "modes_timing.json")
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
    import modes_ref as ref
    times, pm = _timed(lambda: pt.posterior_modes("test", **src))
    U, n = int(pm.n_distinct), int(np.prod(pm.mode_mean.shape[1:]))
    rec = dict(setting=setting, n=n, n_samples=int(pm.n_samples), n_distinct=U, n_modes=int(pm.n_modes), mass=[float(v) for v in pm.mass],
               spread=float(pm.spread), gpu_seconds=times, flops=3.0 * U * (U + 1) / 2 * n)
    # the device call alone, without the host finishing
    if src:
        w = dict(w=src["weights"])
    else:
        kw, _ = pt._sample_source(None, None, "all", 1, count=True)
        w = kw
    r2 = (0.025 ** 2) * n
    rec["device_call_seconds"] = _timed(lambda: pt._sampler.modes("test", radius_sq_sum=r2, outputs=True, **w))[0]
    if cpu:
        low = pt._sampler.modes("test", radius_sq_sum=r2, outputs=True, sq_dist=True, **w)
        t0 = time.perf_counter()
        sq = ref.sq_float64(low["outputs"])
        t1 = time.perf_counter()
        rho, delta, parent = ref.density_peaks_rows(sq, low["count"], r2)
        t2 = time.perf_counter()
        rec.update(cpu_seconds=dict(sq=t1 - t0, density_and_parents=t2 - t1), cpu_threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or None,
                   same_rho=bool(np.array_equal(rho, low["rho"])), same_parent=bool(np.array_equal(parent, low["parent"])),
                   largest_relative_gap_of_sq_to_numpy=float(np.max(np.abs(sq - low["sq_dist"]) / np.maximum(sq, 1e-300))))
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
