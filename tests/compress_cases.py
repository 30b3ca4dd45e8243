"""The inputs of the posterior-compression tests (tests/test_compress_cpu.py, tests/test_gpu_compress.py)."""
import numpy as np

# the known answer: eight points on a line, sample 5 absent, M = 10.  The curve rises at n = 5 and n = 7: it is not monotone.
KNOWN_VALUES = np.array([[0], [1], [2], [3], [10], [11], [12], [20]], np.float32)
KNOWN_COUNTS = np.array([1, 2, 1, 1, 1, 0, 3, 1], np.int32)
KNOWN_M = 7
KNOWN_PICKS = [3, 6, 1, 4, 7, 0, 2]
KNOWN_ENERGY = [4.82, 0.72, 269 / 450, 0.32, 0.42, 49 / 450, 0.15877551020408163]

# the strides of the kernels: 256 threads of the mean kernel, 1024 of the herding walk
LINE_U = (1, 2, 255, 256, 257, 1023, 1024, 1025)


def line(U, seed=0):
    """U integer points on a line (repeats among them: distance 0 between distinct samples, ties go to the lower index): every
    distance is an integer, every sum of them exact in double.  -> values [U, 1] float32."""
    rng = np.random.default_rng(7000 + 10 * U + seed)
    return rng.integers(-500, 501, (U, 1)).astype(np.float32)


def planted(seed=0):
    """Two tight groups of 96 and 32 samples on 12 columns, counts 1 -> (values [128, 12] float32, group [128])."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.3, 0.01, (96, 12))
    b = rng.normal(0.6, 0.01, (32, 12))
    return np.concatenate([a, b]).astype(np.float32), np.concatenate([np.zeros(96, np.int64), np.ones(32, np.int64)])
