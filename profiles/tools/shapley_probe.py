"""Timing record of shapley_values: one call on the GPU per setting, each in a fresh process under its own
time limit, beside the float64 numpy restatement (tests/shapley_ref.py) timed on a small slice on this CPU and scaled up to the
same work -- a projection, labelled as one.  Recorded, not gated.  The library must have been built.

    python profiles/tools/shapley_probe.py --gpu      # the two GPU settings -> profiles/shapley_timing.json (merged)
    python profiles/tools/shapley_probe.py --cpu      # the CPU slices and their projections -> the same file

Settings: Sunspot 4-5-1, exact (16 coalitions), the 198 test rows, 64 background rows, the samples of the README's run (64
replicas, 640 000 samples, burn-in 0.5); and the Ionosphere shape 34-50-2 (synthetic rows of that shape: 234 train, 117 test), 32
permutations, 64 background rows, 1000 distinct weight vectors."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "profiles", "shapley_timing.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIMIT = 240                                                              # seconds per GPU child
IONO_U, IONO_PERMS, IONO_SEED = 1000, 32, 7


def sunspot_child():
    import numpy as np
    import parity
    import ptnn_amd  # noqa: F401
    from ptnn_amd.pt_timeseries_regression import ParallelTempering
    d = parity.datasets()
    pt = ParallelTempering(True, 0.1, d["sunspot_train"], d["sunspot_test"], [4, 5, 1], 64, 2, 640000, 100, 0.5, tempfile.mkdtemp(), seed=1,
                           write_files=False)
    pt.initialize_chains(0.5)
    pt.run_chains()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        sv = pt.shapley_values("test", "train", max_background=64)
        times.append(time.perf_counter() - t0)
    n_rows = int(np.asarray(d["sunspot_test"]).shape[0])
    return dict(setting="sunspot 4-5-1 exact", n_rows=n_rows, n_background=int(sv.background.shape[0]), n_coalitions=sv.n_coalitions,
                n_samples=int(sv.n_samples), n_distinct=int(sv.n_distinct), gpu_seconds=times, importance=sv.importance.tolist(),
                efficiency_gap=sv.efficiency_gap)


def ionosphere_case():
    from parity import orc
    from test_gpu_analysis_shapes import _data, _vectors
    topo = (34, 50, 2)
    train, test = _data(orc.TASK_CLS, topo, 1, n_tr=234, n_te=117)
    return topo, train, test, _vectors(topo, IONO_U, 2)


def ionosphere_child():
    from parity import orc
    from test_gpu_predict import _pt
    topo, train, test, W = ionosphere_case()
    pt = _pt(orc.TASK_CLS, topo, train, test, 4, 20, tempfile.mkdtemp(), lr=0.01, maxtemp=10)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        sv = pt.shapley_values("test", "train", max_background=64, n_permutations=IONO_PERMS, seed=IONO_SEED, weights=W)
        times.append(time.perf_counter() - t0)
    return dict(setting="ionosphere 34-50-2, 32 permutations", n_rows=int(test.shape[0]), n_background=int(sv.background.shape[0]),
                n_coalitions=sv.n_coalitions, n_samples=int(sv.n_samples), n_distinct=int(sv.n_distinct), gpu_seconds=times,
                efficiency_gap=sv.efficiency_gap)


def cpu_slices(record):
    """shapley_ref on a slice that finishes within a minute, scaled to the setting's (distinct vectors x rows)."""
    import numpy as np
    import parity
    import shapley_ref as ref
    from parity import orc
    from ptnn_amd.shapley import shapley_table
    from test_gpu_analysis_shapes import _vectors
    d = parity.datasets()
    tr, te = np.asarray(d["sunspot_train"]), np.asarray(d["sunspot_test"])
    bg = tr[np.rint(np.linspace(0, tr.shape[0] - 1, 64)).astype(np.int64), :4]
    masks, coef = shapley_table(4)
    W = _vectors((4, 5, 1), 20, 3)
    t0 = time.perf_counter()
    for w in W:
        ref.functionals(ref.coalition_values(te[:, :4], bg, w, (4, 5, 1), orc.TASK_REG, masks), coef)
    per_vector = (time.perf_counter() - t0) / W.shape[0]
    gpu = record.get("sunspot", {})
    U = gpu.get("n_distinct", 320000)
    record["sunspot_cpu"] = dict(slice="20 vectors x 198 rows x 16 coalitions x 64 background rows", seconds_per_vector=per_vector,
                                 projected_for_vectors=U, projected_seconds=per_vector * U,
                                 note="a projection: the slice's time scaled by the number of distinct vectors")
    topo, train, test, Wi = ionosphere_case()
    bgi = train[np.rint(np.linspace(0, train.shape[0] - 1, 64)).astype(np.int64), :34]
    masks, coef = shapley_table(34, n_permutations=IONO_PERMS, seed=IONO_SEED)
    t0 = time.perf_counter()
    ref.functionals(ref.coalition_values(test[:8, :34], bgi, Wi[0], topo, orc.TASK_CLS, masks), coef)
    per_row = (time.perf_counter() - t0) / 8
    record["ionosphere_cpu"] = dict(slice=f"1 vector x 8 rows x {masks.size} coalitions x 64 background rows", seconds_per_vector_row=per_row,
                                    projected_for=f"{IONO_U} vectors x {test.shape[0]} rows", projected_seconds=per_row * IONO_U * test.shape[0],
                                    note="a projection: the slice's time scaled by vectors x rows")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps({"sunspot": sunspot_child, "ionosphere": ionosphere_child}[sys.argv[2]]()), flush=True)
        return 0
    record = json.load(open(OUT)) if os.path.exists(OUT) else {}
    if "--gpu" in sys.argv:
        for name in ("sunspot", "ionosphere"):                          # a fresh process each; the first failure ends the probe
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True, timeout=LIMIT)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                return p.returncode
            record[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(name, record[name]["gpu_seconds"], flush=True)
    if "--cpu" in sys.argv:
        cpu_slices(record)
        print({k: v["projected_seconds"] for k, v in record.items() if k.endswith("_cpu")})
    with open(OUT, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
