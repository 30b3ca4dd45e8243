"""The reference of the case-influence tests: the weighted two-pass cross-covariance of two sample matrices in float64 numpy, with
an np.longdouble variant for the bound checks, the error bound of DESIGN.md section 30, and the host arithmetic of the result
restated.  No device import."""
import numpy as np


def influence(A, B, mult=None, dtype=np.float64):
    """A [S, n_a] target columns and B [S, n_b] case log-likelihoods, a sample per row, with integer multiplicities mult [S]
    (None: 1 each).  Two passes in `dtype`: the weighted means, then the weighted centred products; ddof 1 over the expanded
    multiset of M = sum(mult) samples.  -> dict(cov [n_a, n_b], target_mean, target_var [n_a], case_mean, case_var [n_b], all of
    `dtype`; n_samples = M)."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    m = np.ones(A.shape[0], dtype=dtype) if mult is None else np.asarray(mult, dtype=dtype)
    M = m.sum()
    ma, mb = (m[:, None] * A).sum(axis=0) / M, (m[:, None] * B).sum(axis=0) / M
    da, db = A - ma, B - mb
    wa = m[:, None] * da
    return dict(cov=(wa.T @ db) / (M - 1), target_mean=ma, target_var=(wa * da).sum(axis=0) / (M - 1), case_mean=mb,
                case_var=(m[:, None] * db * db).sum(axis=0) / (M - 1), n_samples=int(M))


def influence_longdouble(A, B, mult=None):
    """influence() in np.longdouble (the products of the matrix product included: an explicit sum, not BLAS)."""
    A, B = np.asarray(A, dtype=np.longdouble), np.asarray(B, dtype=np.longdouble)
    m = np.ones(A.shape[0], dtype=np.longdouble) if mult is None else np.asarray(mult, dtype=np.longdouble)
    M = m.sum()
    ma, mb = (m[:, None] * A).sum(axis=0) / M, (m[:, None] * B).sum(axis=0) / M
    da, db = A - ma, B - mb
    wa = m[:, None] * da
    cov = np.stack([(wa[:, a, None] * db).sum(axis=0) for a in range(A.shape[1])]) / (M - 1)
    return dict(cov=cov, target_mean=ma, target_var=(wa * da).sum(axis=0) / (M - 1), case_mean=mb,
                case_var=(m[:, None] * db * db).sum(axis=0) / (M - 1), n_samples=int(M))


def tol(U, s_a, s_b):
    """The bound on |cov - exact| of a two-pass centred float64 sum of U weighted products in any order:
    16 (U + 64) 2^-53 s_a s_b, s the expanded ddof-1 standard deviations; s_a [n_a], s_b [n_b] -> [n_a, n_b]."""
    return 16.0 * (U + 64) * 2.0 ** -53 * np.multiply.outer(np.asarray(s_a, dtype=np.float64), np.asarray(s_b, dtype=np.float64))


def top_cases(cov, top):
    """The `top` case indices of each target column by |cov| descending, lowest index first on a tie, in plain loops."""
    cov = np.asarray(cov)
    flat = cov.reshape(-1, cov.shape[-1])
    k = min(top, flat.shape[1])
    idx = np.array([sorted(range(flat.shape[1]), key=lambda i: (-abs(row[i]), i))[:k] for row in flat], dtype=np.int64)
    return idx.reshape(cov.shape[:-1] + (k,))
