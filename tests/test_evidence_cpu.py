"""Log evidence, host side (no GPU): the regression constant log c against quadrature over eta, evidence_from_rungs on a
conjugate toy with a known answer, philox.prior_weights' layout, evidence_compare's arithmetic, and the argument checks of
ptnn_evidence and log_evidence, which run before anything touches a device."""
import ctypes as C
import math

import numpy as np
import pytest

import evidence_ref as ref
from ptnn_oracle import TASK_CLS, TASK_REG


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__
    __graft_entry__.build()
    import ptnn_amd
    return ptnn_amd


@pytest.mark.parametrize("n_rows,sse", [(1, 0.3), (12, 0.7), (12, 40.0), (50, 3.5), (298, 12.0)])
def test_log_c_against_quadrature_over_eta(n_rows, sse):
    from ptnn_amd.parallel_tempering import evidence_log_c
    want = ref.log_c_quadrature(n_rows, sse)
    assert evidence_log_c(TASK_REG, n_rows) == pytest.approx(want, abs=1e-8)
    assert ref.log_c(TASK_REG, n_rows) == evidence_log_c(TASK_REG, n_rows)
    assert evidence_log_c(TASK_CLS, n_rows) == 0.0


def _toy(a, betas, n, n_prior, seed):
    """theta ~ N(0, 1), U = -a theta^2 / 2: q_beta = N(0, 1 / (1 + a beta)), log Z = -log(1 + a) / 2; exact iid draws."""
    from ptnn_amd.parallel_tempering import evidence_from_rungs
    rng = np.random.default_rng(seed)
    betas = np.asarray(betas, np.float64)
    d = np.append(np.diff(betas), 0.0)
    st = [ref.rung_stats(-0.5 * a * (rng.standard_normal(n) / math.sqrt(1 + a * b)) ** 2, dk) for b, dk in zip(betas, d)]
    u0 = -0.5 * a * rng.standard_normal(n_prior) ** 2
    p0 = ref.prior_stats(u0, np.zeros(n_prior), 0.0)
    p1 = ref.prior_stats(u0, np.zeros(n_prior), betas[0])
    return evidence_from_rungs(betas, [s["mean"] for s in st], [s["var"] for s in st], np.full(betas.size, float(n)),
                               [s["log_stone"] for s in st], [s["relvar"] for s in st],
                               prior_log_mean_exp_b=p0["log_mean_exp"], prior_u_mean=p0["u_mean"], prior_u_var=p0["u_var"],
                               prior_kish_ess_b=p0["kish"], prior_log_mean_exp_first=p1["log_mean_exp"],
                               prior_kish_ess_first=p1["kish"], n_prior=n_prior)


@pytest.mark.parametrize("a", [0.5, 4.0, 30.0])
def test_evidence_from_rungs_on_a_conjugate_toy(a):
    truth = -0.5 * math.log(1 + a)
    dense = np.geomspace(1e-3, 1.0, 48)
    r = _toy(a, dense, 20000, 1 << 16, seed=int(a * 10))
    assert abs(r["log_z_ss"] - truth) < 4 * r["se_log_z_ss"]
    assert abs(r["log_z_ti"] - truth) < 4 * r["se_log_z_ti"] + r["ti_discretisation"]
    assert r["betas"][0] == 0.0 and r["betas"].size == dense.size + 1
    assert r["u_mean"].size == r["u_mcse"].size == r["ess"].size == dense.size + 1
    # a coarse ladder: the discretisation term grows
    coarse = _toy(a, np.geomspace(1e-3, 1.0, 6), 20000, 1 << 16, seed=int(a * 10) + 1)
    assert coarse["ti_discretisation"] > 2 * r["ti_discretisation"]


def test_evidence_from_rungs_arithmetic():
    from ptnn_amd.parallel_tempering import evidence_from_rungs
    betas = [0.25, 0.5, 1.0]
    r = evidence_from_rungs(betas, [-4.0, -3.0, -2.0], [1.0, 1.0, 4.0], [100.0, 100.0, 100.0], [-0.5, -0.7, 0.0], [0.1, 0.2, 9.0],
                            prior_log_mean_exp_b=0.0, prior_u_mean=-6.0, prior_u_var=9.0, prior_kish_ess_b=1000.0,
                            prior_log_mean_exp_first=-1.0, prior_kish_ess_first=500.0, n_prior=1000, log_c=2.0)
    # trapezoid over (0, -6), (.25, -4), (.5, -3), (1, -2)
    integral = 0.125 * (-6 - 4) + 0.125 * (-4 - 3) + 0.25 * (-3 - 2)
    assert r["log_z_ti"] == pytest.approx(2.0 + integral, rel=1e-14)
    half = 0.25 * (-6 - 3) + 0.25 * (-3 - 2)            # points 0, 0.5, 1
    assert r["ti_discretisation"] == pytest.approx(abs(integral - half), rel=1e-14)
    assert r["log_z_ss"] == pytest.approx(2.0 - 1.0 - 0.5 - 0.7, rel=1e-14)
    w = np.array([0.125, 0.25, 0.375, 0.25])
    var = np.array([9.0 / 1000, 0.01, 0.01, 0.04])
    assert r["se_log_z_ti"] == pytest.approx(math.sqrt(float(np.dot(w * w, var))), rel=1e-12)
    assert r["se_log_z_ss"] == pytest.approx(math.sqrt(1 / 500 - 1 / 1000 + 0.1 / 100 + 0.2 / 100), rel=1e-12)
    for bad in ([0.5, 0.9], [0.0, 1.0], [0.5, 0.5, 1.0], [1.0, 0.5]):
        with pytest.raises(ValueError, match="betas"):
            evidence_from_rungs(bad, [0] * len(bad), [1] * len(bad), [10] * len(bad), [0] * len(bad), [0] * len(bad),
                                prior_log_mean_exp_b=0, prior_u_mean=0, prior_u_var=1, prior_kish_ess_b=10,
                                prior_log_mean_exp_first=0, prior_kish_ess_first=10, n_prior=10)


def test_prior_weights_layout():
    from ptnn_amd import philox
    assert philox.STREAM_PRIOR == 5
    w = philox.prior_weights(77, 3, 10, 5.0)
    np.testing.assert_array_equal(w, philox.normals(10, 3, 0, 5, 77) * 5.0)
    x = philox.philox4x32(np.arange(3), 3, 0, 5, 77)
    z0 = math.sqrt(-2 * math.log(philox.uniform23(x[0][0]))) * math.cos(2 * math.pi * philox.uniform23(x[1][0]))
    assert w[0] == pytest.approx(5.0 * z0, rel=1e-14)
    z5 = math.sqrt(-2 * math.log(philox.uniform23(x[0][1]))) * math.sin(2 * math.pi * philox.uniform23(x[1][1]))
    assert w[5] == pytest.approx(5.0 * z5, rel=1e-14)                 # k = 5: counter k / 4 = 1, component 1
    assert not np.array_equal(philox.prior_weights(77, 4, 10, 5.0), w)
    assert not np.array_equal(philox.prior_weights(78, 3, 10, 5.0), w)


def test_evidence_compare_arithmetic():
    from ptnn_amd.parallel_tempering import Evidence, evidence_compare
    a = Evidence(*([None] * len(Evidence._fields)))._replace(log_z_ss=-10.0, se_log_z_ss=0.3, log_z_ti=-10.5, se_log_z_ti=0.4)
    b = a._replace(log_z_ss=-12.0, se_log_z_ss=0.4, log_z_ti=-11.0, se_log_z_ti=0.3)
    c = evidence_compare(a, b)
    assert c["log_bf_ss"] == 2.0 and c["se_log_bf_ss"] == pytest.approx(0.5)
    assert c["log_bf_ti"] == 0.5 and c["se_log_bf_ti"] == pytest.approx(0.5)


def test_ptnn_evidence_struct_guard(pt):
    from ptnn_amd import _lib
    lib = pt.load_library()
    s = _lib.EvidenceSpec()
    s.struct_bytes = C.sizeof(_lib.EvidenceSpec) - 8
    rc = lib.ptnn_evidence(None, C.byref(s))
    assert rc < 0 and f"expected {C.sizeof(_lib.EvidenceSpec)}" in lib.ptnn_last_error().decode()


def _spec(**kw):
    from ptnn_amd import _lib
    s = _lib.EvidenceSpec()
    s.struct_bytes = C.sizeof(_lib.EvidenceSpec)
    s.thin, s.nsteps = 1, 10
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_evidence(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_ptnn_evidence_rejects_bad_arguments_without_a_device(pt):
    lib = pt.load_library()
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc, msg = _err(lib, None)
    assert rc < 0 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=8))
    assert rc < 0 and "struct_bytes" in msg
    rc, msg = _err(lib, _spec(nsteps=0))
    assert rc < 0 and "no source" in msg
    rc, msg = _err(lib, _spec(thin=0))
    assert rc < 0 and "thin" in msg
    w = np.zeros(64, np.float32)
    u = np.zeros(16)
    rc, msg = _err(lib, _spec(w=w.ctypes.data_as(fp), u=u.ctypes.data_as(dp), n_rungs=2, n_per_rung=8))
    assert rc < 0 and "not both" in msg
    rc, msg = _err(lib, _spec(u=u.ctypes.data_as(dp), n_rungs=0, n_per_rung=8))
    assert rc < 0 and "n_rungs" in msg
    rc, msg = _err(lib, _spec(u=u.ctypes.data_as(dp), n_rungs=2, n_per_rung=0))
    assert rc < 0 and "n_per_rung" in msg
    bad = u.copy()
    bad[3] = np.nan
    rc, msg = _err(lib, _spec(u=bad.ctypes.data_as(dp), n_rungs=2, n_per_rung=8))
    assert rc < 0 and "not finite" in msg
    mu = np.ones(16, np.int32)
    mu[9] = -2
    rc, msg = _err(lib, _spec(u=u.ctypes.data_as(dp), n_rungs=2, n_per_rung=8, multiplicity=mu.ctypes.data_as(ip)))
    assert rc < 0 and "negative" in msg
    a = np.zeros(5)
    rc, msg = _err(lib, _spec(n_prior=100, a=a.ctypes.data_as(dp), n_a=5))
    assert rc < 0 and "exponents" in msg
    rc, msg = _err(lib, _spec(n_prior=100, n_a=1))
    assert rc < 0 and "exponents" in msg
    rc, msg = _err(lib, _spec(n_prior=-1))
    assert rc < 0 and "n_prior" in msg
    a[0] = np.inf
    rc, msg = _err(lib, _spec(n_prior=100, a=a.ctypes.data_as(dp), n_a=1))
    assert rc < 0 and "not finite" in msg
    out = np.zeros(16)
    rc, msg = _err(lib, _spec(u=u.ctypes.data_as(dp), n_rungs=2, n_per_rung=8, u_out=out.ctypes.data_as(dp)))
    assert rc < 0 and "u_out" in msg
    rc, msg = _err(lib, _spec(u_prior_out=out.ctypes.data_as(dp)))
    assert rc < 0 and "u_prior_out" in msg
    # a consistent request reaches the handle check
    rc, msg = _err(lib, _spec())
    assert rc < 0 and "null handle" in msg
    rc, msg = _err(lib, _spec(u=u.ctypes.data_as(dp), n_rungs=2, n_per_rung=8))
    assert rc < 0 and "null handle" in msg


def _cls_pt(tmp_path, **kw):
    from ptnn_amd.pt_classification import ParallelTempering
    rng = np.random.default_rng(0)
    x = rng.random((12, 4))
    y = rng.integers(0, 3, 12)
    data = np.column_stack([x, y])
    return ParallelTempering(False, 0.1, data, data, [4, 5, 3], 4, 1000, 4 * 100, 10, str(tmp_path), seed=1, write_files=False, **kw)


def test_log_evidence_refusals_before_a_device(tmp_path, pt):
    pt_ = _cls_pt(tmp_path)
    with pytest.raises(ValueError, match="initialize_chains"):
        pt_.log_evidence()
