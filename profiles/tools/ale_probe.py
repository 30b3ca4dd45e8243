"""Cost probe: ale_forward_kernel beside pd_forward_kernel, Ionosphere shape 34-50-2, same (U, rows): all 34 inputs, 16 bins
against 16 grid values.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times; the library must have been built."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from parity import orc  # noqa: E402
from test_gpu_analysis_shapes import _data, _vectors  # noqa: E402
from test_gpu_predict import _pt  # noqa: E402

topo = (34, 50, 2)
U = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 16
train, test = _data(orc.TASK_CLS, topo, 1, n_tr=234, n_te=117)
pt = _pt(orc.TASK_CLS, topo, train, test, 4, 20, tempfile.mkdtemp(), lr=0.01, maxtemp=10)
W = _vectors(topo, U, 2)
for rep in range(2):
    t0 = time.perf_counter()
    pd = pt.partial_dependence("test", grid=G, weights=W)
    t1 = time.perf_counter()
    ale = pt.accumulated_effects("test", bins=G, weights=W)
    t2 = time.perf_counter()
    both = pt.accumulated_effects("test", inputs=[0, 1, 2, 3], bins=G, pairs="all", weights=W)
    t3 = time.perf_counter()
    print(f"rep {rep}: U = {pd.n_distinct}, rows = {test.shape[0]}, inputs = {pd.inputs.size}, grid = bins = {G}: partial dependence "
          f"{1e3 * (t1 - t0):.2f} ms, accumulated effects {1e3 * (t2 - t1):.2f} ms, 4 inputs with their 6 pairs {1e3 * (t3 - t2):.2f} ms")
print("pd effect_range", np.round(pd.effect_range[:6, 0], 5), "ale effect_range", np.round(ale.effect_range[:6, 0], 5))
print("interaction", np.round(both.interaction[:, 0], 6))
