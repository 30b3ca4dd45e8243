"""Input sensitivity, host side (no GPU): the float64 reference against central differences of the oracle's forward pass and at
its closed form, the host helper of top_prob, the exported entry point, and its argument checks, which run before anything
touches a device."""
import ctypes as C

import numpy as np
import pytest

import sensitivity_ref as ref
from parity import orc


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def _outputs(X, w, topo, task):
    out = orc.forward(X, w, topo)[1]
    if task == orc.TASK_CLS:
        e = np.exp(out)
        out = e / e.sum(axis=1, keepdims=True)
    return out


def _setup(topo, seed, n=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, topo[0])), rng.standard_normal(orc.num_param(topo))


@pytest.mark.parametrize("task,topo", [(orc.TASK_REG, (4, 5, 1)), (orc.TASK_CLS, (4, 12, 3))], ids=["reg-4-5-1", "cls-4-12-3"])
def test_jacobian_against_central_differences(task, topo):
    I, _, O = topo
    X, w = _setup(topo, 11 + O)
    g = ref.jacobian(X, w, topo, task)
    assert g.shape == (X.shape[0], O, I)
    # central differences at step 1e-4: truncation step^2 |f'''| / 6 ~ 1e-9 |f'''|, rounding 2^-53 / step ~ 1e-12
    step = 1e-4
    fd = np.empty_like(g)
    for i in range(I):
        dx = np.zeros(I)
        dx[i] = step
        fd[:, :, i] = (_outputs(X + dx, w, topo, task) - _outputs(X - dx, w, topo, task)) / (2 * step)
    assert np.max(np.abs(fd - g)) <= 1e-7 * max(1.0, np.max(np.abs(g)))
    assert np.max(np.abs(g)) > 1e-3                                    # the comparison is not of zeros


def test_jacobian_closed_form_one_hidden_unit():
    topo = (3, 1, 1)
    X, w = _setup(topo, 5)
    W1, W2, B1, B2 = orc.decode(w, topo)
    hid, out = orc.forward(X, w, topo)
    want = (out * (1 - out) * W2[0, 0] * hid * (1 - hid)) * W1[:, 0][None, :]       # [n, I]
    np.testing.assert_allclose(ref.jacobian(X, w, topo, orc.TASK_REG)[:, 0, :], want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("topo", [(4, 12, 3), (6, 9, 18)])
def test_class_gradients_sum_to_zero(topo):
    X, w = _setup(topo, 23)
    g = ref.jacobian(X, w, topo, orc.TASK_CLS)
    assert np.max(np.abs(g.sum(axis=1))) <= 1e-15
    assert np.all(ref.error_bound(X, w, topo, orc.TASK_CLS) >= np.abs(g))          # the bound's |J| terms dominate g itself


def test_saturated_units_keep_their_slope():
    """e / (1 + e)^2 where 1 - sigmoid(z) would cancel to 0."""
    s, d = ref._sigmoid_slope(np.array([40.0, -40.0, 0.0]))
    assert d[0] == d[1] and 0 < d[0] < 1e-17 and d[2] == 0.25
    assert s[0] == 1.0 and 0 < s[1] < 1e-17


def test_top_share_with_multiplicities(pt):
    from ptnn_amd.parallel_tempering import top_share
    rng = np.random.default_rng(3)
    a = rng.random((30, 2, 5)).astype(np.float32)
    a[4, 0, :] = [0.25, 0.75, 0.75, 0.1, 0.75]                        # an exact tie: the first index wins
    a[9, 1, :] = 0.5                                                   # all equal: input 0
    counts = rng.integers(0, 6, 30)
    counts[4] = 3
    counts[9] = 2
    got = top_share(a, counts)
    expd = np.repeat(a, counts, axis=0)
    want = np.zeros((2, 5))
    for row in expd:
        for o in range(2):
            want[o, np.argmax(row[o])] += 1
    want /= expd.shape[0]
    assert np.array_equal(got, want)
    assert np.array_equal(top_share(expd), want)
    assert np.allclose(got.sum(axis=1), 1.0)
    only = top_share(a[4:5], [3])
    assert only[0, 1] == 1.0 and only[0, 2] == 0.0 and only[0, 4] == 0.0


def test_library_exports_sensitivity(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_sensitivity is not None and "ptnn_sensitivity" in _lib.SYMBOLS
    assert C.sizeof(_lib.SensitivitySpec) > 0
    assert lib.ptnn_abi_version() == 4 and _lib.ABI_VERSION == 4


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.SensitivitySpec()
    s.struct_bytes = C.sizeof(_lib.SensitivitySpec)
    s.thin, s.nsteps, s.n_rows, s.x_source = 1, 10, 4, _lib.PREDICT_X_TRAIN
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_sensitivity(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_sensitivity_rejects_bad_arguments_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    fp, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
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
    w = np.zeros(4, np.float32)
    rc, msg = _err(lib, _spec(w=w.ctypes.data_as(fp), n_w=0))
    assert rc < 0 and "n_w" in msg
    out = np.zeros(4, np.float32)
    ranks = np.zeros(17, np.int64)
    for n_f, ranks_f, out_f in (("n_ranks", "ranks", "order_stats"), ("n_ranks2", "ranks2", "abs_order_stats")):
        rc, msg = _err(lib, _spec(**{n_f: 17, ranks_f: ranks.ctypes.data_as(i64p)}))
        assert rc < 0 and "n_ranks = 17" in msg, n_f
        rc, msg = _err(lib, _spec(**{n_f: 2}))
        assert rc < 0 and "ranks is NULL" in msg, n_f
        rc, msg = _err(lib, _spec(**{out_f: out.ctypes.data_as(fp)}))
        assert rc < 0 and "without ranks" in msg, n_f
    # a consistent request reaches the handle check
    rc, msg = _err(lib, _spec())
    assert rc < 0 and "null handle" in msg
    rc, msg = _err(lib, _spec(n_ranks=1, ranks=ranks.ctypes.data_as(i64p), n_ranks2=1, ranks2=ranks.ctypes.data_as(i64p)))
    assert rc < 0 and "null handle" in msg
