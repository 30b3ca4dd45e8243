"""Cost probe: sensitivity_forward_kernel beside predict_forward_kernel, Ionosphere shape 34-50-2, same (U, rows).  The library must
have been built (PTNN_LIBRARY selects another one, as in every probe)."""
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
train, test = _data(orc.TASK_CLS, topo, 1, n_tr=234, n_te=117)
pt = _pt(orc.TASK_CLS, topo, train, test, 4, 20, tempfile.mkdtemp(), lr=0.01, maxtemp=10)
W = _vectors(topo, U, 2)
for rep in range(2):
    t0 = time.perf_counter()
    pp = pt.posterior_predictive("test", weights=W)
    t1 = time.perf_counter()
    se = pt.input_sensitivity("test", weights=W)
    t2 = time.perf_counter()
    print(f"rep {rep}: U = {se.n_distinct}, rows = {test.shape[0]}, predictive {1e3 * (t1 - t0):.2f} ms, sensitivity {1e3 * (t2 - t1):.2f} ms")
print("importance", np.round(se.importance[0, :6], 5))
