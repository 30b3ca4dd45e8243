"""One ptnn_compress call for the kernel-time table of DESIGN.md section 34: U random output vectors of 8 columns through values=,
m picks and one evaluated subset of m items.  Meant to run under the profiler, a run of its own, nothing else traced:

    rocprofv3 --kernel-trace --stats -d DIR -o run -f csv -- python profiles/tools/compress_probe.py 4096 256

The library must have been built.  Prints the energy curve's ends and the wall time of the call."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    U, m = int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 256
    import uncertainty_cases as cases
    from parity import orc
    from test_gpu_predict import _pt
    train, test, _, _, _ = cases.regression_case((4, 5, 1))
    pt = _pt(orc.TASK_REG, (4, 5, 1), np.array(train), np.array(test), 4, 20, tempfile.mkdtemp())
    rng = np.random.default_rng(U)
    values = rng.normal(0.5, 0.1, (U, 8)).astype(np.float32)
    subset = rng.integers(0, U, (1, m)).astype(np.int32)
    t0 = time.perf_counter()
    out = pt._sampler.compress(values=values, m=m, subsets=subset)
    dt = time.perf_counter() - t0
    print(f"U = {U}, m = {m}: energy[0] = {out['energy'][0]:.6g}, energy[-1] = {out['energy'][-1]:.6g}, equivalent draws = "
          f"{out['d0'] / out['energy'][-1]:.1f}, random subset = {out['subset_energy'][0]:.6g}, call {dt * 1e3:.1f} ms", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
