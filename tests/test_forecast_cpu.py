"""Recursive forecasts, host side (no GPU): the float64 oracle of tests/forecast_ref.py against known answers, the noise
counter layout, the "end" window of the shipped series, and the exported entry point's argument checks, which run before
anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import forecast_ref as ref
import parity
from parity import orc
from ptnn_amd import philox


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


def _vector(topo, seed=1):
    I, H, O = topo
    return np.random.default_rng(seed).standard_normal(I * H + H * O + H + O)


def test_zero_hidden_weights_give_a_constant_path():
    # W2 = 0: the output is sigmoid(-B2) whatever the window, so every step repeats it
    topo = (4, 5, 1)
    w = _vector(topo)
    W1, W2, B1, B2 = orc.decode(w, topo)
    W2[:] = 0.0
    B2[:] = 0.75
    origins = np.random.default_rng(2).random((3, 4))
    path = ref.trajectories(w[None], origins, 12, topo)
    want = 1.0 / (1.0 + np.exp(0.75))
    assert path.shape == (1, 3, 12)
    np.testing.assert_allclose(path, want, rtol=0, atol=1e-15)


def test_one_step_is_the_forward_pass():
    topo = (5, 10, 1)
    ws = np.stack([_vector(topo, s) for s in range(4)])
    origins = np.random.default_rng(3).random((7, 5))
    path = ref.trajectories(ws, origins, 1, topo)
    for v in range(4):
        assert np.array_equal(path[v, :, 0], orc.forward(origins, ws[v], topo)[1][:, 0])


def test_recursion_feeds_outputs_back():
    topo = (4, 5, 1)
    w = _vector(topo, 5)
    origin = np.array([0.1, 0.2, 0.3, 0.4])
    path = ref.trajectories(w[None], origin[None], 9, topo)[0, 0]
    win = origin.copy()
    for k in range(9):
        assert np.array_equal(ref.teacher_windows(origin, path, k, 4), win)
        y = orc.forward(win[None], w, topo)[1][0, 0]
        assert path[k] == y
        win = np.append(win[1:], y)


def test_noise_counter_layout():
    seed, i, r, h = 0x1234_5678_9ABC, 17, 3, 11
    z = ref.noise_draws(h, i, r, seed)
    for k in range(h):
        x = philox.philox4x32(k >> 2, i, r, 4, seed)
        u = [philox.uniform23(v)[()] for v in x]
        rad0, rad1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
        comp = [rad0 * np.cos(2 * np.pi * u[1]), rad0 * np.sin(2 * np.pi * u[1]),
                rad1 * np.cos(2 * np.pi * u[3]), rad1 * np.sin(2 * np.pi * u[3])]
        assert z[k] == pytest.approx(comp[k & 3], rel=1e-15, abs=1e-15)
    assert philox.STREAM_FORECAST == 4
    # a longer horizon extends the draws, it does not change them
    assert np.array_equal(ref.noise_draws(40, i, r, seed)[:h], z)
    # noise on: each step adds exp(eta / 2) z_k, and the noisy value is what the next step reads
    topo = (4, 5, 1)
    w = _vector(topo, 6)
    origin = np.array([[0.3, 0.1, 0.4, 0.1]])
    eta = np.array([-3.0])
    noisy = ref.trajectories(w[None], origin, 6, topo, eta=eta, seed=seed, traj_index=[i])[0, 0]
    zz = ref.noise_draws(6, i, 0, seed)
    win = origin[0].copy()
    for k in range(6):
        y = orc.forward(win[None], w, topo)[1][0, 0] + np.exp(-1.5) * zz[k]
        assert noisy[k] == pytest.approx(y, rel=1e-14)
        win = np.append(win[1:], noisy[k])


def test_end_window_of_sunspot():
    d = parity.datasets()
    te, series = d["sunspot_test"], d["sunspot_scaled"]
    # every row is 5 consecutive values of one series (delay 1); the rows step by 2 and overlap
    assert np.array_equal(te[1:, :3], te[:-1, 2:5])
    n = series.shape[0]
    assert np.allclose(te[-1], series[n - 6:n - 1], rtol=0, atol=1e-6)
    win = ref.end_window(te, 4)
    assert np.array_equal(win, te[-1, 1:5].astype(np.float64))
    assert win[-1] == te[-1, 4] and np.array_equal(win[:3], te[-1, 1:4])
    # the window right after the last row: the series' values n - 5 .. n - 2, whose successor is its last value
    assert np.allclose(win, series[n - 5:n - 1], rtol=0, atol=1e-6)
    # the 5-input series the same way
    t5 = d["sunspot5_test"]
    assert np.array_equal(ref.end_window(t5, 5), t5[-1, 1:6].astype(np.float64))
    assert np.array_equal(t5[1:, :4], t5[:-1, 2:6])


def test_forecast_entry_point_is_exported(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    assert lib.ptnn_forecast is not None and "ptnn_forecast" in _lib.SYMBOLS
    s = _spec(struct_bytes=4)
    rc = lib.ptnn_forecast(None, C.byref(s))
    assert rc < 0 and f"expected {C.sizeof(_lib.ForecastSpec)}" in lib.ptnn_last_error().decode()


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.ForecastSpec()
    s.struct_bytes = C.sizeof(_lib.ForecastSpec)
    s.thin, s.nsteps, s.n_origins, s.origin_source, s.horizon = 1, 10, 4, _lib.FORECAST_ORIGIN_TRAIN, 5
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_forecast(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_forecast_rejects_bad_arguments_without_a_device(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=8))
    assert rc < 0 and "struct_bytes" in msg
    for hz in (0, -3):
        rc, msg = _err(lib, _spec(horizon=hz))
        assert rc < 0 and "horizon" in msg
    rc, msg = _err(lib, _spec(n_origins=1 << 20, horizon=1 << 12))
    assert rc < 0 and "columns" in msg
    rc, msg = _err(lib, _spec(n_ranks=17, ranks=(C.c_int64 * 17)()))
    assert rc < 0 and "n_ranks" in msg
    rc, msg = _err(lib, _spec(origin_source=7))
    assert rc < 0 and "origin_source" in msg
    rc, msg = _err(lib, _spec(origin_source=_lib.FORECAST_ORIGIN_HOST))
    assert rc < 0 and "origins" in msg
    w = (C.c_float * 8)()
    rc, msg = _err(lib, _spec(w=C.cast(w, C.POINTER(C.c_float)), n_w=1, noise=1))
    assert rc < 0 and "eta" in msg
    rc, msg = _err(lib, _spec(thin=0))
    assert rc < 0 and "thin" in msg
    # past the argument checks: a null handle
    rc, msg = _err(lib, _spec())
    assert rc < 0 and "handle" in msg
