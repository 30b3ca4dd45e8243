"""Posterior compression without a GPU: tests/compress_ref.py (the device's orders in numpy float64) on the known answer, the
planted proportions, one multiset one result, and the identity E[energy of n random draws] = D0 / n; the host functions of
ptnn_amd/compress.py; and the C entry's argument checks and structure layout, which need neither a handle nor a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import compress_cases as cases
import compress_ref as ref

from ptnn_amd import _lib, compress, parallel_tempering as pt_module  # noqa: E402


def test_known_answer_exact():
    sq = ref.sq_of(cases.KNOWN_VALUES)
    assert int(cases.KNOWN_COUNTS.sum()) == 10
    h = ref.herd(sq, cases.KNOWN_COUNTS, cases.KNOWN_M)
    assert h["picks"].tolist() == cases.KNOWN_PICKS and 5 not in h["picks"]
    for got, want in zip(h["energy"], cases.KNOWN_ENERGY):
        assert abs(got - want) <= 1e-12 * want
    assert abs(h["d0"] - 6.98) <= 1e-12 * 6.98 and h["mu"][5] == 0.0
    e = h["energy"]
    assert e[4] > e[3] and e[6] > e[5]                                      # the curve rises at n = 5 and n = 7: not monotone
    # every prefix is the energy of that subset by the definition, and by the subset evaluation
    for n in range(1, cases.KNOWN_M + 1):
        assert e[n - 1] == pytest.approx(ref.energy_plain(cases.KNOWN_VALUES, cases.KNOWN_COUNTS, h["picks"][:n]), rel=1e-12, abs=1e-13)
        assert e[n - 1] == pytest.approx(float(ref.subset_energy(sq, cases.KNOWN_COUNTS, h["picks"][:n])), rel=1e-12, abs=1e-13)
    # the long-double walk takes the same picks and agrees to double precision
    hl = ref.herd(sq, cases.KNOWN_COUNTS, cases.KNOWN_M, dtype=np.longdouble)
    assert hl["picks"].tolist() == cases.KNOWN_PICKS and np.abs(hl["energy"].astype(np.float64) - e).max() <= 1e-13


@pytest.mark.parametrize("seed", range(3))
def test_planted_proportions(seed):
    values, group = cases.planted(seed)
    sq, count = ref.sq_of(values), np.ones(len(values), np.int64)
    h = ref.herd(sq, count, 16)
    for n in (4, 8, 12, 16):
        assert int(group[h["picks"][:n]].sum()) == n // 4                   # the small group holds a quarter of the mass
    rng = np.random.default_rng(seed)
    rand = [float(ref.subset_energy(sq, count, rng.choice(len(values), 16, replace=False), mu=h["mu"], d0=h["d0"])) for _ in range(200)]
    draws = h["d0"] / h["energy"][15]
    print(f"seed {seed}: herded energy {h['energy'][15]:.4g}, 200 random 16-subsets: best {min(rand):.4g}, median {np.median(rand):.4g}; "
          f"equivalent draws {draws:.0f}")
    assert h["energy"][15] < min(rand) and draws > 100


def test_one_multiset_one_result():
    rng = np.random.default_rng(5)
    P = rng.normal(0.5, 0.1, (20, 3)).astype(np.float32)
    count = rng.integers(0, 4, 20)
    count[0] = 2
    a = ref.herd(ref.sq_of(P), count, 6)
    expand = np.repeat(np.arange(20), count)                                # the expanded list: every occurrence its own sample
    b = ref.herd(ref.sq_of(P[expand]), np.ones(len(expand), np.int64), 6)
    # (a pick's unmerged duplicate stays a candidate, but the pick's own column adds 0 to its r while every other r grows: over these
    # six picks none is taken twice)
    assert a["d0"] == pytest.approx(b["d0"], rel=1e-12)
    assert expand[b["picks"]].tolist() == a["picks"].tolist() and np.allclose(b["energy"], a["energy"], rtol=1e-12, atol=0)
    # (distinct, counts) in another order of the samples: the picks name the same samples
    perm = rng.permutation(20)
    c = ref.herd(ref.sq_of(P[perm]), count[perm], 6)
    assert perm[c["picks"]].tolist() == a["picks"].tolist() and np.allclose(c["energy"], a["energy"], rtol=1e-12, atol=0)
    mu_a, mu_b = a["mu"], b["mu"]
    assert np.allclose(mu_b, mu_a[expand], rtol=1e-12, atol=0)


def test_identity_mean_energy_of_random_draws():
    sq = ref.sq_of(cases.KNOWN_VALUES)
    _, d0 = ref.mean_distances(sq, cases.KNOWN_COUNTS)
    got = ref.mean_energy_of_draws(cases.KNOWN_VALUES, cases.KNOWN_COUNTS, 3)  # 8^3 ordered triples weighted by the counts
    assert got == pytest.approx(d0 / 3, rel=1e-12)


def test_orders_of_the_reference():
    # the tree adds i and i + N / 2 first; the strided partials add t, t + 256, ...: an order a plain sum does not take
    x = np.array([1.0, 2.0 ** -53, 0.0, 2.0 ** -53])
    assert ref.wg_sum(x) == 1.0 + 2.0 ** -52 and ((x[0] + x[1]) + x[2]) + x[3] == 1.0
    t = np.zeros(513)
    t[0], t[256], t[512] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ref.strided_sum(t) == 1.0 and ref.strided_sum(t[::-1].copy()) == 1.0 + 2.0 ** -52
    k = ref.key_of(np.array([-2.0, -0.5, 0.0, 0.25, 3.0]))
    assert (np.diff(k.astype(object)) > 0).all()


def test_host_functions():
    assert compress.thinned_items(4, 10).tolist() == [0, 2, 5, 7] and compress.thinned_items(3, 3).tolist() == [0, 1, 2]
    assert compress.thinned_items(4, 5, [2, 0, 1, 0, 1]).tolist() == [0, 0, 2, 4]  # positions 0, 1, 2, 3 of the expanded 0 0 2 4
    assert compress.thinned_items(2, 3, [0, 0, 5]).tolist() == [2, 2] and compress.thinned_items(0, 5).tolist() == []
    assert compress.first_items([2, 0, 2, 1, 0], 4).tolist() == [1, 3, 0, -1]
    F = np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 1.0], [9.0, 1.0]])
    gap, ratio = compress.moment_match(F, [1, 2, 1, 0], [0, 2])
    assert gap == 0.0 and ratio == pytest.approx(1.0 / np.sqrt(0.5))        # column 1 has no spread: left out of the median
    sq = ref.sq_of(cases.KNOWN_VALUES)
    h = ref.herd(sq, cases.KNOWN_COUNTS, 4)
    item = np.array([3, 0, 1, 1, 2, 3, 4, 6, 6, 6, 7, 5])
    out = dict(picks=h["picks"].astype(np.int32), energy=h["energy"], pick_score=h["pick_score"], mu=h["mu"], d0=float(h["d0"]), count=cases.KNOWN_COUNTS,
               item_sample=item.astype(np.int32), outputs=cases.KNOWN_VALUES, sq_dist=sq, n_samples=10, n_distinct=8)
    pc = compress.finish_compress(out, 1, n_chains=3)
    assert pc.picks.tolist() == [3, 6, 1, 4] and pc.items.tolist() == [0, 7, 2, 6] and pc.rows.tolist() == [[0, 0], [1, 3], [0, 2], [1, 2]]
    assert np.array_equal(pc.equivalent_draws, h["d0"] / h["energy"]) and pc.spread == h["d0"] and pc.spread_rms == h["d0"]
    assert np.array_equal(pc.distances, np.sqrt(sq)) and pc.vectors is None and pc.eta is None and pc.evaluated is None
    want_gap, want_ratio = compress.moment_match(cases.KNOWN_VALUES, cases.KNOWN_COUNTS, [3, 6, 1, 4])
    assert pc.mean_gap == want_gap and pc.sd_ratio == want_ratio and pc.n_samples == 10 and pc.n_distinct == 8
    flat = compress.finish_compress(dict(out, sq_dist=None), 4)
    assert flat.rows.tolist() == [[-1, 0], [-1, 7], [-1, 2], [-1, 6]] and flat.distances is None and np.array_equal(flat.energy_rms, h["energy"] / 2)
    none = compress.finish_compress(dict(out, picks=out["picks"][:0], energy=h["energy"][:0], pick_score=h["pick_score"][:0]), 1, with_rows=False)
    assert none.picks.shape == (0,) and none.rows.shape == (0, 2) and none.mean_gap is None and none.sd_ratio is None
    zero = compress.finish_compress(dict(out, energy=np.array([0.5, 0.0, -1e-17, 0.25])), 1)
    assert zero.equivalent_draws.tolist() == [h["d0"] / 0.5, np.inf, np.inf, h["d0"] / 0.25]
    assert pt_module.PosteriorCompression is compress.PosteriorCompression and pt_module.thinned_items is compress.thinned_items
    assert issubclass(pt_module.ParallelTemperingBase, compress.CompressAnalysis)
    doc = " ".join(pt_module.ParallelTemperingBase.posterior_compress.__doc__.split())
    assert "NOT monotone" in doc and "carried with each pick, not matched" in doc and "spread / k" in doc


# ---- the C entry: bound, and its argument checks need neither a handle nor a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load_library()


def _spec(**kw):
    s = _lib.CompressSpec()
    s.struct_bytes = C.sizeof(_lib.CompressSpec)
    s.thin, s.nsteps, s.n_rows, s.x_source, s.m, s.room = 1, 10, 4, _lib.PREDICT_X_TRAIN, 3, 1 << 20
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _err(lib, spec):
    rc = lib.ptnn_compress(None, None if spec is None else C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


def test_entry_point_is_bound_and_checks_its_arguments_without_a_device(lib):
    assert "ptnn_compress" in _lib.SYMBOLS and lib.ptnn_compress is not None and lib.ptnn_abi_version() == 4 == _lib.ABI_VERSION
    # the struct of include/ptnn.h on LP64: the trace source (32 bytes), the host vectors (24), the rows (16), the host matrix and m
    # (16), the subsets (16), room (8), ten outputs and two counters (96)
    assert C.sizeof(_lib.CompressSpec) == 208 and _lib.CompressSpec.m.offset == 84 and _lib.CompressSpec.room.offset == 104
    assert _lib.CompressSpec.picks.offset == 112
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptnn.h")).read()
    body = header[header.index("typedef struct ptnn_compress_spec {"):header.index("} ptnn_compress_spec;")]
    names = re.findall(r"[\s\*]([a-z_0-9]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.CompressSpec._fields_]
    # the fields the two specs share lie where ptnn_modes_spec has them
    for name in ("replicas", "thin", "w", "multiplicity", "n_w", "x_source", "n_rows", "x", "values", "n_a"):
        assert getattr(_lib.CompressSpec, name).offset == getattr(_lib.ModesSpec, name).offset, name
    rc, msg = _err(lib, None)
    assert rc == -1 and "null" in msg
    rc, msg = _err(lib, _spec(struct_bytes=4))
    assert rc == -1 and "expected 208" in msg
    one = np.zeros(4, np.float32)
    onep = one.ctypes.data_as(C.POINTER(C.c_float))
    idx = np.zeros(4, np.int32)
    idxp = idx.ctypes.data_as(C.POINTER(C.c_int32))
    for kw, word in ((dict(values=onep, w=onep, n_w=1, n_a=1), "not both"), (dict(m=-1), "m = -1 picks: must be >= 0"),
                     (dict(n_subsets=-2), "n_subsets = -2"), (dict(n_subsets=1), "subset_items is NULL"),
                     (dict(n_subsets=1, subset_items=idxp, subset_size=0), r"subset_size = 0 outside [1, 65536]"),
                     (dict(n_subsets=1, subset_items=idxp, subset_size=65537), "subset_size = 65537"),
                     (dict(thin=0), "thin"), (dict(x_source=7), "x_source"), (dict(x_source=_lib.PREDICT_X_HOST), "needs x"),
                     (dict(n_rows=0), "n_rows"), (dict(w=onep, n_w=0), "n_w = 0"), (dict(values=onep, n_w=0, n_a=1), "n_w = 0"),
                     (dict(values=onep, n_w=4, n_a=0), "n_a = 0"),
                     (dict(values=onep, n_w=11586, n_a=1), "11586 distinct samples")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # the cap's text is ptnn_modes' own
    cap = _err(lib, _spec(values=onep, n_w=11586, n_a=1))[1]
    s = _lib.ModesSpec()
    s.struct_bytes, s.values, s.n_w, s.n_a, s.room = C.sizeof(_lib.ModesSpec), onep, 11586, 1, 1 << 20
    assert lib.ptnn_modes(None, C.byref(s)) == -1 and lib.ptnn_last_error().decode() == cap and "thin=, chains=" in cap
    # the order of adjacent checks: both sources, m, the subsets, the source, the rows
    for kw, word in ((dict(values=onep, w=onep, n_w=1, n_a=1, m=-1), "not both"), (dict(m=-1, n_subsets=-1), "m = -1"),
                     (dict(n_subsets=-1, thin=0), "n_subsets"), (dict(thin=0, x_source=7), "thin"), (dict(x_source=7, n_rows=0), "x_source")):
        rc, msg = _err(lib, _spec(**kw))
        assert rc == -1 and word in msg, (kw, msg)
    # a consistent request reaches the handle check
    for kw in ({}, dict(m=0), dict(w=onep, n_w=1, nsteps=0), dict(values=onep, n_w=4, n_a=1, n_rows=0, x_source=9),
               dict(values=onep, n_w=11585, n_a=1), dict(n_subsets=1, subset_items=idxp, subset_size=4)):
        rc, msg = _err(lib, _spec(**kw))
        assert rc < 0 and "null handle" in msg, (kw, msg)
