"""Posterior predictive, host side (no GPU): the percentile arithmetic that turns the device's exact order statistics into
np.percentile's values, the exported entry point, and its argument checks, which run before anything touches a device."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def _via_order_stats(values, pcts):
    """What posterior_predictive does with the device's output, with np.partition standing in for the radix select."""
    from ptnn_amd.parallel_tempering import lerp_percentile, percentile_ranks
    n = values.shape[0]
    spots = percentile_ranks(n, pcts)
    ranks = sorted({r for lo, hi, _ in spots for r in (lo, hi)})
    part = np.partition(values, ranks, axis=0)
    os_ = {r: part[r].astype(np.float32) for r in ranks}       # the device returns fp32 values
    return [lerp_percentile(os_[lo], os_[hi], g) for lo, hi, g in spots]


PCTS = [0, 5, 37.5, 50, 95, 100, 2.5, 97.5, 99.9, 33.333]


@pytest.mark.parametrize("M", [1, 2, 3, 1000])
def test_percentiles_from_order_statistics_equal_numpy(pt, M):
    rng = np.random.default_rng(M)
    vals = rng.random((M, 7)).astype(np.float32)
    got = _via_order_stats(vals, PCTS)
    want = np.percentile(vals.astype(np.float64), PCTS, axis=0)
    for k, p in enumerate(PCTS):
        assert np.array_equal(got[k], want[k]), p


def test_percentiles_with_multiplicities(pt):
    """Distinct values with counts, expanded: what a chain of mostly rejected steps looks like."""
    rng = np.random.default_rng(7)
    distinct = rng.standard_normal((40, 3)).astype(np.float32)
    counts = rng.integers(1, 30, size=40)
    vals = np.repeat(distinct, counts, axis=0)
    got = _via_order_stats(vals, PCTS)
    want = np.percentile(vals.astype(np.float64), PCTS, axis=0)
    for k, p in enumerate(PCTS):
        assert np.array_equal(got[k], want[k]), p


def test_library_exports_predict(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_predict is not None and "ptnn_predict" in _lib.SYMBOLS
    assert C.sizeof(_lib.PredictSpec) > 0


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.PredictSpec()
    s.struct_bytes = C.sizeof(_lib.PredictSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source = 1, 10, 4, _lib.PREDICT_X_TRAIN
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_predict(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_predict_rejects_bad_arguments_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=8))
    assert rc < 0 and "struct_bytes" in msg
    rc, msg = _err(lib, _spec(thin=0))
    assert rc < 0 and "thin" in msg
    rc, msg = _err(lib, _spec(x_source=7))
    assert rc < 0 and "x_source" in msg
    rc, msg = _err(lib, _spec(x_source=_lib.PREDICT_X_HOST))
    assert rc < 0 and "needs x" in msg
    rc, msg = _err(lib, _spec(n_rows=0))
    assert rc < 0 and "n_rows" in msg
    rc, msg = _err(lib, _spec(n_ranks=17))
    assert rc < 0 and "n_ranks" in msg
    rc, msg = _err(lib, _spec(n_ranks=2))
    assert rc < 0 and "ranks is NULL" in msg
    w = np.zeros(4, np.float32)
    rc, msg = _err(lib, _spec(w=w.ctypes.data_as(C.POINTER(C.c_float)), n_w=0))
    assert rc < 0 and "n_w" in msg
    out = np.zeros(4, np.float32)
    rc, msg = _err(lib, _spec(order_stats=out.ctypes.data_as(C.POINTER(C.c_float))))
    assert rc < 0 and "without ranks" in msg
    # a consistent request reaches the handle check
    rc, msg = _err(lib, _spec())
    assert rc < 0 and "null handle" in msg
