"""Record a golden file of tests/test_gpu_analysis_bits.py: every output of a list of posterior-analysis calls that the test holds
bit for bit (and the digest of each case's inputs).  Run ONCE per list, on the commit BEFORE the change the list guards, on the GPU:

    python3 profiles/tools/record_analysis_bits.py first [out.npz]      tests/golden/analysis_bits_parent.npz: the nine calls recorded
                                                                        before the reductions and scans of the analysis kernels
                                                                        (csrc/ptnn_dev_wg.hpp and its callers) were gathered
    python3 profiles/tools/record_analysis_bits.py second [out.npz]     tests/golden/analysis_bits_parent2.npz: the second list, recorded
                                                                        before the host code of these calls was folded onto shared paths
    python3 profiles/tools/record_analysis_bits.py third [out.npz]      tests/golden/analysis_bits_parent3.npz: the third list, recorded
                                                                        before the scored calls, the predictive-mixture columns and
                                                                        the rung layout were folded onto shared frames
    python3 profiles/tools/record_analysis_bits.py forward [out.json]   tests/golden/forward_bits_parent.json: the digests of
                                                                        tests/test_gpu_forward_bits.py, recorded before the per-shape
                                                                        forward kernels took their common pieces from csrc/ptnn_dev_net.hpp

PTNN_LIBRARY=<the parent commit's libptnn.so> selects the library where the Python tree is the new commit's.
The cases live in the test modules, so the recording and the test cannot drift apart."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LISTS = ("first", "second", "third", "forward")
if len(sys.argv) < 2 or sys.argv[1] not in LISTS:
    sys.exit("usage: record_analysis_bits.py first|second|third|forward [out]")
if sys.argv[1] == "forward":
    import test_gpu_forward_bits as f  # noqa: E402
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", f.GOLDEN_FILE)
    rec = f.record()
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{out}: {sum(len(c) for c in rec.values())} digests of {len(rec)} cases, {os.path.getsize(out)} bytes")
    sys.exit(0)

import test_gpu_analysis_bits as t  # noqa: E402

file, record = {"first": (t.GOLDEN_FILE, t.record), "second": (t.GOLDEN_FILE2, t.record2), "third": (t.GOLDEN_FILE3, t.record3)}[sys.argv[1]]
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", file)
rec = record()
np.savez_compressed(out, **rec)
print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")
