"""Record tests/golden/sgd_rows_parent.npz: the inputs and the outputs (uint32 bit patterns) that tests/test_gpu_sgd_rows.py holds
the SGD row loop to, bit for bit.  Run ONCE, on the commit BEFORE a change to sweep_rows_reg41, on the GPU:

    python3 profiles/tools/record_sgd_rows.py [out.npz]

The cases live in the test module, so the recording and the test cannot drift apart."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_sgd_rows as t  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.GOLDEN_FILE)
rec = t.record()
np.savez_compressed(out, **rec)
print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")
