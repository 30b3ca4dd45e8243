"""The case grid of the classification report's tests: at seven classification shapes the data of tests/test_gpu_analysis_shapes.py
(`_data`, seed 11: 150 train rows, 53 test rows) and 65 weight vectors (`_vectors`, seed 12), the float64 oracle's softmax
probabilities of the vectors on the test rows, and the two quantities that bound what an fp32 forward pass within 1e-5 of the
oracle can change: the (sample, row) pairs whose two largest probabilities lie within MARGIN of each other (their argmax may
differ), and the (positive, negative) score pairs within NEAR = 2 MARGIN (their order may differ).  No device."""
import functools

import numpy as np

from parity import orc

SHAPES = [(4, 6, 3), (34, 7, 2), (9, 5, 2), (11, 9, 10), (20, 8, 2), (16, 12, 10), (6, 10, 18)]
IDS = ["-".join(map(str, t)) for t in SHAPES]
DATA_SEED, VECTOR_SEED, N_VECTORS = 11, 12, 65
MARGIN = 1e-5           # the forward tolerance tests/test_gpu_analysis_shapes.py enforces
NEAR = 2e-5             # two scores each within MARGIN of the oracle's can swap only if the oracle's lie within this
EXCLUDED_CAP = 0.01     # share of (sample, row) pairs the confusion comparison may leave out
NEAR_CAP = 0.01         # share of (positive, negative) pairs that may lie within NEAR


@functools.lru_cache(maxsize=None)
def case(topo):
    """(train, test, W [65, P] float32, oracle probabilities [65, 53, K] float64) of a shape; shared, not to be written to."""
    from test_gpu_analysis_shapes import _data, _vectors
    from test_gpu_predict import _outputs
    train, test = _data(orc.TASK_CLS, topo, DATA_SEED)
    W = _vectors(topo, N_VECTORS, VECTOR_SEED)
    p = _outputs(orc.TASK_CLS, test[:, :topo[0]], W.T.astype(np.float64), topo)
    for a in (train, test, W, p):
        a.setflags(write=False)
    return train, test, W, p


def top_two_margin(p):
    """[U, N]: the largest probability minus the second largest."""
    s = np.sort(p, axis=2)
    return s[:, :, -1] - s[:, :, -2]


def near_pairs(p, y, K, tol=NEAR):
    """(near [U, K], pairs [K]): per (sample, class) the (positive, negative) pairs with |p_n - p_m| <= tol, and n_k (N - n_k)."""
    U = p.shape[0]
    near = np.zeros((U, K), np.int64)
    pairs = np.zeros(K, np.int64)
    for k in range(K):
        pos = y == k
        pairs[k] = int(pos.sum()) * int((~pos).sum())
        if pairs[k]:
            d = np.abs(p[:, pos, k][:, :, None] - p[:, ~pos, k][:, None, :])
            near[:, k] = (d <= tol).sum(axis=(1, 2))
    return near, pairs
