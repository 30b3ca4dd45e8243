"""Record tests/golden/analysis_bits_parent.npz: every output of the nine posterior-analysis calls that
tests/test_gpu_analysis_bits.py holds bit for bit (and the digest of each case's inputs).  Run ONCE, on the commit BEFORE a change
to the reductions and scans of the analysis kernels (csrc/ptnn_dev_wg.hpp and its callers), on the GPU:

    python3 profiles/tools/record_analysis_bits.py [out.npz]

The cases live in the test module, so the recording and the test cannot drift apart."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_analysis_bits as t  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.GOLDEN_FILE)
rec = t.record()
np.savez_compressed(out, **rec)
print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")
