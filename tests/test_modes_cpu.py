"""Posterior modes without a GPU: tests/modes_ref.py on hand-made matrices with known answers (ties in rho and in sq resolved by
index, a zero-count sample, U = 1), the host functions of ptnn_amd/modes.py against the reference's independent restatement,
modes_stuck, and the planted cases of tests/modes_cases.py proven with the oracle's float64 forward: the margins are wide enough
that the fp32 device cannot flip a comparison, and the reference alone returns exactly the planted labelling; and the C entry's
argument checks and structure layout, which need neither a handle nor a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import modes_cases as cases
import modes_ref as ref
import report_cases

from ptnn_amd import _lib, modes, parallel_tempering as pt_module  # noqa: E402


def _line(points):
    p = np.asarray(points, dtype=np.float64)
    return (p[:, None] - p[None, :]) ** 2


def test_two_clumps_on_a_line():
    #            0    1    2    3     4     5     6
    sq = _line([0.0, 0.1, 0.2, 5.0, 5.1, 5.2, 5.3])
    count = [1, 1, 1, 1, 1, 1, 1]
    rho, delta, parent = ref.density_peaks(sq, count, 0.15 ** 2)
    assert rho.tolist() == [2, 3, 2, 2, 3, 3, 2]
    # the densest, lowest index: 1 (nothing precedes it); 4 follows 1 (rho 3, index above), 5 follows 4
    assert parent.tolist() == [1, -1, 1, 4, 1, 4, 5]
    assert delta[1] == sq[1].max() and delta[4] == sq[4, 1] and delta[5] == sq[5, 4] and delta[0] == sq[0, 1]
    lab, centres, mass = ref.labels_of(rho, delta, parent, count, 1.0, 1)
    assert centres.tolist() == [4, 1] and mass.tolist() == [4, 3] and lab.tolist() == [1, 1, 1, 0, 0, 0, 0]
    # a centre needs the mass: with min_count 4 sample 4 (rho 3) is no centre and everything joins the one mode
    lab, centres, mass = ref.labels_of(rho, delta, parent, count, 1.0, 4)
    assert centres.tolist() == [1] and mass.tolist() == [7] and (lab == 0).all()


def test_ties_in_rho_and_sq_go_to_the_lower_index():
    sq = _line([0.0, 1.0, 2.0, 3.0])                                        # nobody is near anybody: every rho is 1
    rho, delta, parent = ref.density_peaks(sq, [1, 1, 1, 1], 0.0)
    assert rho.tolist() == [1, 1, 1, 1] and parent.tolist() == [-1, 0, 1, 2] and delta.tolist() == [9.0, 1.0, 1.0, 1.0]
    sq = _line([1.0, 0.0, 2.0])                                             # sample 0 lies between the other two: both follow it
    rho, delta, parent = ref.density_peaks(sq, [1, 1, 1], 0.0)
    assert parent.tolist() == [-1, 0, 0]
    sq = np.array([[0.0, 4.0, 1.0, 1.0], [4.0, 0.0, 1.0, 1.0], [1.0, 1.0, 0.0, 4.0], [1.0, 1.0, 4.0, 0.0]])
    rho, delta, parent = ref.density_peaks(sq, [1, 1, 1, 1], 0.0)
    assert parent.tolist() == [-1, 0, 0, 0]                                 # 2 and 3: equal sq to 0 and 1, the lower index wins
    # duplicates: d = 0 between different samples, equal rho
    sq = _line([0.0, 7.0, 0.0, 7.0])
    rho, delta, parent = ref.density_peaks(sq, [2, 1, 1, 2], 0.0)
    assert rho.tolist() == [3, 3, 3, 3] and parent.tolist() == [-1, 0, 0, 1] and delta.tolist() == [49.0, 49.0, 0.0, 0.0]
    lab, centres, mass = ref.labels_of(rho, delta, parent, [2, 1, 1, 2], 1.0, 1)
    assert centres.tolist() == [0, 1] and mass.tolist() == [3, 3] and lab.tolist() == [0, 1, 0, 1]   # equal mass: the lower centre first


def test_a_zero_count_sample_is_absent():
    sq = _line([0.0, 0.05, 0.1, 9.0])
    count = [1, 0, 2, 1]
    rho, delta, parent = ref.density_peaks(sq, count, 0.2 ** 2)
    assert rho.tolist() == [3, 0, 3, 1] and parent.tolist() == [-1, -1, 0, 2] and delta[1] == 0.0
    lab, centres, mass = ref.labels_of(rho, delta, parent, count, 1.0, 1)
    assert lab.tolist() == [0, -1, 0, 1] and centres.tolist() == [0, 3] and mass.tolist() == [3, 1]
    got = modes.mode_labels(rho, delta, parent, count, 1.0, 1)
    assert got[0].tolist() == lab.tolist() and got[1].tolist() == [0, 3] and got[2].tolist() == [3, 1]
    assert float(ref.spread_sq(sq, count)) == pytest.approx((2 * 2 * 0.01 + 2 * 81.0 + 2 * 2 * 8.9 ** 2) / 16, rel=1e-12)


def test_one_sample():
    rho, delta, parent = ref.density_peaks(np.zeros((1, 1)), [3], 0.0)
    assert rho.tolist() == [3] and parent.tolist() == [-1] and delta.tolist() == [0.0]
    lab, centres, mass = modes.mode_labels(rho, delta, parent, [3], 1.0, 3)
    assert lab.tolist() == [0] and centres.tolist() == [0] and mass.tolist() == [3]
    out = dict(rho=rho, delta_sq=delta, parent=parent, count=[3], item_sample=[0, 0, 0, 0, 0, 0], outputs=np.full((1, 4), 0.25, np.float32),
               spread_sq=0.0, n_samples=6, n_distinct=1, sq_dist=np.zeros((1, 1)))
    pm = modes.finish_modes(dict(out, count=[6]), (2, 2), 4, 0.01, 0.02, n_chains=2)
    assert pm.n_modes == 1 and pm.mass.tolist() == [1.0] and pm.hops.tolist() == [0, 0] and pm.occupancy.tolist() == [[1.0], [1.0]]
    assert pm.labels.shape == (2, 3) and pm.centre_rows.tolist() == [[0, 0]] and pm.hop_matrix.tolist() == [[0]]
    assert pm.mode_mean.shape == (1, 2, 2) and (pm.mode_mean == 0.25).all() and (pm.mode_sd == 0).all() and pm.within.tolist() == [0.0]
    assert pm.spread == 0.0 and pm.distances.tolist() == [[0.0]] and pm.between.tolist() == [[0.0]]


@pytest.mark.parametrize("seed", range(6))
def test_host_functions_against_the_restatement(seed):
    rng = np.random.default_rng(seed)
    U, n, C, m = 40, 6, 3, 30
    centres = rng.uniform(0.2, 0.8, (3, n))
    F = (centres[rng.integers(0, 3, U)] + 0.01 * rng.standard_normal((U, n))).astype(np.float32)
    F[7] = F[3]                                                             # duplicates that are not neighbours
    item = rng.integers(0, U, C * m)
    count = np.bincount(item, minlength=U)
    sep, rad, min_mass = 0.1, 0.05, 0.02
    r = ref.modes(F, count, sep, rad, min_mass)
    M = int(count.sum())
    fast = ref.density_peaks_rows(r["sq"], count, rad * rad * n)           # the row-wise numpy form is the loops'
    assert all(np.array_equal(a, r[k]) for a, k in zip(fast, ("rho", "delta_sq", "parent")))
    assert np.allclose(ref.sq_float64(F), r["sq"], rtol=1e-13, atol=0)
    out = dict(rho=r["rho"], delta_sq=r["delta_sq"], parent=r["parent"].astype(np.int32), count=count.astype(np.int32), item_sample=item.astype(np.int32),
               outputs=F, spread_sq=float(ref.spread_sq(r["sq"], count)), n_samples=M, n_distinct=U, sq_dist=r["sq"])
    pm = modes.finish_modes(out, (n,), n, sep * sep * n, min_mass, n_chains=C)
    assert pm.n_modes == r["n_modes"] == 3 and np.array_equal(pm.sample_labels, r["sample_labels"]) and np.array_equal(pm.centres, r["centres"])
    assert np.array_equal(pm.mass, r["mass"]) and pm.mass.sum() == 1.0 and (np.diff(pm.mass) <= 0).all()
    lab = r["sample_labels"][item].reshape(C, m)
    occ, hops, hm = ref.chain_figures(lab, 3)
    assert np.array_equal(pm.labels, lab) and np.array_equal(pm.occupancy, occ) and np.array_equal(pm.hops, hops) and np.array_equal(pm.hop_matrix, hm)
    assert hm.sum() == hops.sum() and (np.diag(hm) == 0).all()
    F64 = F.astype(np.float64)
    for k in range(3):
        mem = r["sample_labels"] == k
        big = np.repeat(F64[mem], count[mem], axis=0)
        assert np.allclose(pm.mode_mean[k], big.mean(axis=0), rtol=1e-13, atol=0) and np.allclose(pm.mode_sd[k], big.std(axis=0), rtol=1e-9, atol=1e-15)
        d2 = ((big - F64[r["centres"][k]]) ** 2).sum(axis=1) / n
        assert pm.within[k] == pytest.approx(math.sqrt(d2.mean()), rel=1e-13)
        first = int(np.flatnonzero(item == r["centres"][k])[0])
        assert pm.centre_rows[k].tolist() == [first // m, first % m]
    assert np.allclose(pm.between, np.sqrt(r["sq"][np.ix_(r["centres"], r["centres"])] / n), rtol=1e-13, atol=0)
    assert np.array_equal(pm.delta, np.sqrt(r["delta_sq"] / n)) and np.array_equal(pm.distances, np.sqrt(r["sq"] / n))
    # without chains
    flat = modes.finish_modes(out, (n,), n, sep * sep * n, min_mass, None)
    assert flat.occupancy is None and flat.hops is None and flat.hop_matrix is None and flat.labels.shape == (C * m,)
    assert (flat.centre_rows[:, 0] == -1).all() and np.array_equal(flat.centre_rows[:, 1], pm.centre_rows[:, 0] * m + pm.centre_rows[:, 1])
    none = modes.finish_modes(out, (n,), n, sep * sep * n, min_mass, None, with_rows=False)
    assert (none.centre_rows == -1).all()
    assert pt_module.PosteriorModes is modes.PosteriorModes and pt_module.modes_stuck is modes.modes_stuck


def test_modes_stuck():
    pm = modes.PosteriorModes(*[None] * len(modes.PosteriorModes._fields))
    pm = pm._replace(mass=np.array([0.6, 0.3, 0.1, 0.0]), occupancy=np.array([[1.0, 0, 0, 0], [0.5, 0.5, 0, 0], [0.2, 0.2, 0.6, 0]]))
    assert modes.modes_stuck(pm).tolist() == [[0, 1], [0, 2], [1, 2]]
    assert modes.modes_stuck(pm, min_mass=0.2).tolist() == [[0, 1]]
    assert modes.modes_stuck(pm, min_mass=0).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert modes.modes_stuck(pm, min_mass=0.7).shape == (0, 2) and modes.modes_stuck(pm).dtype == np.int64
    with pytest.raises(ValueError, match="min_mass = 2 must lie in"):
        modes.modes_stuck(pm, min_mass=2)
    with pytest.raises(ValueError, match="has no chains"):
        modes.modes_stuck(pm._replace(occupancy=None))


@pytest.mark.parametrize("topo", [cases.REG_TOPO, cases.CLS_TOPO], ids=lambda t: "-".join(map(str, t)))
def test_planted_cases_have_the_margins(topo):
    task, train, test, W, mult, group, base, sep, radius = cases.planted(topo)
    assert len(W) == sum(cases.SIZES) + cases.N_PERMUTED and mult.min() >= 1
    F = cases.outputs(task, topo, test, W)
    d = cases.rms(F)
    same = group[:, None] == group[None, :]
    between, within = d[~same].min(), d[same].max()
    print(f"{topo}: between-group d >= {between:.4g} (4 separations = {4 * sep:.4g}); within-group d <= {within:.4g} (radius / 4 = {radius / 4:.4g})")
    assert between >= 4 * sep and within <= radius / 4
    for u in np.flatnonzero(base >= 0):
        assert d[u, base[u]] <= 1e-12 and not np.array_equal(W[u], W[base[u]])
    assert (base >= 0).sum() == cases.N_PERMUTED
    # an fp32 forward pass within MARGIN of the oracle moves a d by at most 2 MARGIN: neither comparison can flip
    assert min(between - sep, radius - within) >= 10 * report_cases.MARGIN and min(sep - within, between - radius) >= 10 * report_cases.MARGIN
    want, mass = cases.planted_labels(group, mult)
    r = ref.modes(F, mult, sep, radius, 0.02)
    assert r["n_modes"] == 3 and np.array_equal(r["sample_labels"], want) and (r["sample_labels"] >= 0).all()
    assert np.array_equal(r["mass"], mass) and all(group[c] == group[np.flatnonzero(want == k)[0]] for k, c in enumerate(r["centres"]))


# ---- the C entry: bound, and its argument checks need neither a handle nor a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load_library()


def _spec(**kw):
    s = _lib.ModesSpec()
    s.struct_bytes = C.sizeof(_lib.ModesSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source, s.near_sq, s.room = 1, 10, 4, _lib.PREDICT_X_TRAIN, 0.5, 1 << 20
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_modes(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device(lib):
    assert "ptnn_modes" in _lib.SYMBOLS and lib.ptnn_modes is not None and lib.ptnn_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert _lib.MODES_MAX_ELEMENTS == 1 << 27 and _lib.MODES_MAX_DISTINCT == 11585 and 11586 ** 2 > 1 << 27 >= 11585 ** 2
    # the struct of include/ptnn.h on LP64: the trace source (32 bytes), the host vectors (24), the rows (16), the host matrix (16),
    # near_sq and room (16), eight outputs and two counters (80)
    assert C.sizeof(_lib.ModesSpec) == 184 and _lib.ModesSpec.near_sq.offset == 88 and _lib.ModesSpec.rho.offset == 104
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptnn.h")).read()
    body = header[header.index("typedef struct ptnn_modes_spec {"):header.index("} ptnn_modes_spec;")]
    names = re.findall(r"[\s\*]([a-z_0-9]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.ModesSpec._fields_]
    rc, msg = _err(lib, None)
    assert rc == -1 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc == -1 and "expected 184" in msg
    one = np.zeros(4, np.float32)
    onep = one.ctypes.data_as(C.POINTER(C.c_float))
    for kw, word in ((dict(values=onep, w=onep, n_w=1, n_a=1), "not both"), (dict(near_sq=-1.0), "near_sq = -1 must be a finite number >= 0"),
                     (dict(near_sq=float("nan")), "near_sq = nan"), (dict(near_sq=float("inf")), "near_sq = inf"),
                     (dict(thin=0), "thin"), (dict(x_source=7), "x_source"), (dict(x_source=_lib.PREDICT_X_HOST), "needs x"),
                     (dict(n_rows=0), "n_rows"), (dict(w=onep, n_w=0), "n_w = 0"), (dict(values=onep, n_w=0, n_a=1), "n_w = 0"),
                     (dict(values=onep, n_w=4, n_a=0), "n_a = 0"),
                     (dict(values=onep, n_w=11586, n_a=1), "11586 distinct samples")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    assert "thin=, chains=" in _err(lib, _spec(values=onep, n_w=11586, n_a=1))[1]
    # the order of adjacent checks: both sources, near_sq, the source, the rows
    for kw, word in ((dict(values=onep, w=onep, n_w=1, n_a=1, near_sq=-1.0), "not both"), (dict(near_sq=-1.0, thin=0), "near_sq"),
                     (dict(thin=0, x_source=7), "thin"), (dict(x_source=7, n_rows=0), "x_source"), (dict(values=onep, n_w=0, n_a=0), "n_w = 0")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # a consistent request reaches the handle check
    for kw in ({}, dict(near_sq=0.0), dict(w=onep, n_w=1, nsteps=0), dict(values=onep, n_w=4, n_a=1, n_rows=0, x_source=9), dict(values=onep, n_w=11585, n_a=1)):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and "null handle" in msg, (kw, msg)
