"""Shapley attributions without a GPU: the float64 reference (tests/shapley_ref.py) against brute force over every order and
against known answers, shapley_table against the reference's tables with every property the device relies on, the symbol table
and the layout of ShapSpec against the header's struct, and the argument checks of ptnn_coalition_values through the loaded
library with a NULL handle (every call checks its spec before it looks at the handle)."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import shapley_ref as ref
from parity import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG, CLS = orc.TASK_REG, orc.TASK_CLS


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__
    __graft_entry__.build()
    sys.path.insert(0, ROOT)
    import ptnn_amd  # noqa: F401
    from ptnn_amd import _lib
    return _lib


def _case(task, topo, seed, n=3, B=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, topo[0])), rng.standard_normal((B, topo[0])), rng.standard_normal(orc.num_param(topo))


# ---- the reference ----
@pytest.mark.parametrize("task,topo", [(REG, (4, 5, 1)), (CLS, (5, 3, 3))], ids=["I4", "I5"])
def test_reference_is_brute_force_over_all_orders(task, topo):
    X, bg, w = _case(task, topo, 11 + topo[0])
    exact = ref.shapley_exact(X, bg, w, topo, task)
    brute = ref.shapley_brute_force(X, bg, w, topo, task)
    assert exact.shape == (3, topo[2], topo[0])
    np.testing.assert_allclose(exact, brute, rtol=0, atol=1e-14)
    # efficiency: the values of a row sum to v(all) - v(empty)
    I = topo[0]
    v = ref.coalition_values(X, bg, w, topo, task, [0, (1 << I) - 1])
    assert np.max(np.abs(exact.sum(axis=2) - (v[:, 1] - v[:, 0]))) <= 1e-14
    # v(all) is the net's output on the row, v(empty) the mean output over the background
    f = lambda rows: ref._f(rows, w, topo, task)                          # noqa: E731
    assert np.max(np.abs(v[:, 1] - f(X))) <= 1e-15 and np.max(np.abs(v[:, 0] - f(bg).mean(axis=0))) <= 1e-15
    # and the tables give the same numbers through the device's formula
    masks, coef = ref.table_exact(I)
    out = ref.functionals(ref.coalition_values(X, bg, w, topo, task, masks), coef)
    np.testing.assert_allclose(out[:, :, :I], exact, rtol=0, atol=1e-14)
    assert np.array_equal(out[:, :, I], v[:, 0]) and np.array_equal(out[:, :, I + 1], v[:, 1])


def test_reference_known_answers():
    topo = (4, 5, 1)
    X, bg, w = _case(REG, topo, 3, n=2, B=1)
    # one background row that differs from the explained row in one input: that input gets f(x) - f(b), the others 0
    x = bg[:1].copy()
    x[0, 2] += 0.75
    phi = ref.shapley_exact(x, bg, w, topo, REG)
    fx, fb = ref._f(x, w, topo, REG)[0, 0], ref._f(bg, w, topo, REG)[0, 0]
    assert abs(phi[0, 0, 2] - (fx - fb)) <= 1e-15 and np.all(phi[0, 0, [0, 1, 3]] == 0)
    # an input the net does not read (a zero row of W1) gets 0
    w0 = w.copy()
    w0[1 * 5:2 * 5] = 0.0
    X, bg, _ = _case(REG, topo, 4, n=3, B=6)
    phi = ref.shapley_exact(X, bg, w0, topo, REG)
    assert np.max(np.abs(phi[:, :, 1])) <= 1e-16 and np.min(np.abs(phi[:, :, 0])) > 0
    # every background row equal to the explained row: nothing to split
    assert np.all(ref.shapley_exact(X[:1], np.repeat(X[:1], 4, axis=0), w, topo, REG) == 0)
    # the hybrid row takes exactly the masked inputs
    h = ref.hybrid(X[:1], bg[:2], 0b0101)
    assert np.array_equal(h[0, :, [0, 2]].T, np.repeat(X[:1, [0, 2]], 2, axis=0)) and np.array_equal(h[0][:, [1, 3]], bg[:2][:, [1, 3]])
    bound, out = ref.error_bound(X, bg, w, topo, REG, *ref.table_exact(4))
    assert bound.shape == out.shape == (3, 1, 6) and np.all(bound > 0) and np.all(np.isfinite(bound))


# ---- shapley_table ----
def test_table_exact(binding):
    from ptnn_amd import parallel_tempering as pt
    from ptnn_amd.shapley import shapley_table
    assert pt.shapley_table is shapley_table and pt.ShapleyValues._fields[:3] == ("method", "n_coalitions", "background")
    for I in (1, 2, 4, 6):
        masks, coef = shapley_table(I)                                  # auto: exact up to 6 inputs
        want_m, want_c = ref.table_exact(I)
        assert masks.dtype == np.uint64 and coef.dtype == np.float64 and coef.flags.c_contiguous
        assert np.array_equal(masks, want_m) and coef.shape == (1 << I, I + 2)
        np.testing.assert_allclose(coef, want_c, rtol=0, atol=1e-16)
        phi = coef[:, :I]
        assert np.max(np.abs(phi.sum(axis=0))) <= 1e-15                 # per term the coefficients sum to 0 ...
        np.testing.assert_allclose(np.where(phi > 0, phi, 0).sum(axis=0), 1.0, rtol=0, atol=1e-15)     # ... and the positive ones to 1
        assert coef[:, I].tolist() == [1.0] + [0.0] * ((1 << I) - 1) and coef[:, I + 1].tolist() == [0.0] * ((1 << I) - 1) + [1.0]
    assert shapley_table(12, "exact")[0].size == 4096 and shapley_table(7)[0].size < 128      # auto past 6 inputs: permutations


def test_table_permutation(binding):
    from ptnn_amd.shapley import shapley_table
    I = 9
    masks, coef = shapley_table(I, n_permutations=6, seed=5)
    again = shapley_table(I, "permutation", n_permutations=6, seed=5)
    assert np.array_equal(masks, again[0]) and np.array_equal(coef, again[1])                 # the same seed: the same table
    assert not np.array_equal(masks, shapley_table(I, n_permutations=6, seed=6)[0])
    assert np.unique(masks).size == masks.size and masks[0] == 0 and int(masks.max()) == (1 << I) - 1   # merged; empty first; full there
    assert masks.size <= 6 * (I - 1) + 2 and coef.shape == (masks.size, I + 2)
    assert np.max(np.abs(coef[:, :I].sum(axis=0))) <= 1e-15
    np.testing.assert_allclose(np.where(coef[:, :I] > 0, coef[:, :I], 0).sum(axis=0), 1.0, rtol=0, atol=1e-15)
    assert coef[0, I] == 1 and coef[:, I].sum() == 1 and coef[masks == (1 << I) - 1, I + 1] == 1 and coef[:, I + 1].sum() == 1
    # the drawn orders come in antithetic pairs: an order and its reverse, from np.random.default_rng(seed)
    rng = np.random.default_rng(5)
    orders = []
    for _ in range(3):
        orders += [rng.permutation(I)]
        orders += [orders[-1][::-1]]
    want_m, want_c = ref.table_permutation(I, orders)
    assert np.array_equal(masks, want_m) and np.array_equal(coef, want_c)
    # explicit orders, any number of them
    got = shapley_table(I, permutations=np.array(orders[:3]))
    want = ref.table_permutation(I, orders[:3])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # all 24 orders at I = 4 collapse to the exact table
    m24, c24 = shapley_table(4, permutations=np.array(list(itertools.permutations(range(4)))))
    assert sorted(m24.tolist()) == list(range(16))
    np.testing.assert_allclose(c24[np.argsort(m24)], ref.table_exact(4)[1], rtol=0, atol=1e-15)


TABLE_FAULTS = [
    (dict(n_in=0), "n_in = 0 must be an integer"), (dict(n_in=63), "n_in = 63"), (dict(n_in=2.5), "n_in = 2.5"),
    (dict(method="kernel"), "method = 'kernel'"), (dict(n_in=13, method="exact"), "at most n_in = 12"),
    (dict(method="exact", permutations=[[0, 1, 2, 3]]), "takes no permutations"),
    (dict(n_in=8, n_permutations=3), "even integer >= 2"), (dict(n_in=8, n_permutations=0), "even integer >= 2"),
    (dict(n_in=8, n_permutations=2.5), "even integer >= 2"),
    (dict(permutations=[0, 1, 2, 3]), r"permutations must be \[n, 4\]"), (dict(permutations=np.zeros((0, 4), int)), r"permutations must be"),
    (dict(permutations=[[0, 1, 2]]), r"permutations must be \[n, 4\]"), (dict(permutations=[[0.0, 1.0, 2.0, 3.0]]), "integer orders"),
    (dict(permutations=[[0, 1, 2, 2]]), "each of 0 .. 3 once"), (dict(permutations=[[1, 2, 3, 4]]), "each of 0 .. 3 once"),
    (dict(n_in=60, n_permutations=80), "distinct coalitions: at most 4096"),
]


@pytest.mark.parametrize("kw, text", TABLE_FAULTS, ids=[str(k) for k in range(len(TABLE_FAULTS))])
def test_table_refusals(binding, kw, text):
    from ptnn_amd.shapley import shapley_table
    args = dict(n_in=4, method="auto", n_permutations=32, seed=0, permutations=None)
    args.update(kw)
    with pytest.raises(ValueError, match=text):
        shapley_table(**args)


# ---- the symbol, the ABI and the struct ----
def test_symbol_and_abi(binding):
    assert "ptnn_coalition_values" in binding.SYMBOLS
    lib = binding.load_library()
    assert lib.ptnn_abi_version() == 4 == binding.ABI_VERSION
    assert lib.ptnn_coalition_values is not None
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    assert "int ptnn_coalition_values(ptnn_handle *h, const ptnn_shapley_spec *spec);" in header
    for name, value in (("COALITIONS", 4096), ("BACKGROUND", 256), ("TERMS", 64), ("ACC", 256)):
        assert getattr(binding, "SHAP_MAX_" + name) == value and f"#define PTNN_SHAP_MAX_{name} {value}" in header


def _header_fields():
    """The fields of ptnn_shapley_spec in the header's order."""
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    body = re.search(r"typedef struct ptnn_shapley_spec \{(.*?)\} ptnn_shapley_spec;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
    return names


def test_spec_layout_is_the_headers(binding, tmp_path):
    cls = binding.ShapSpec
    names = [n for n, _ in cls._fields_]
    assert names == _header_fields()
    # the selection and row fields of ptnn_pd_spec, field for field, open the struct
    shared = ["struct_bytes", "replicas", "n_replicas", "step0", "nsteps", "thin", "w", "multiplicity", "n_w", "x_source", "n_rows", "x"]
    assert names[:12] == shared == [n for n, _ in binding.PdSpec._fields_][:12]
    for n in shared:
        assert getattr(cls, n).offset == getattr(binding.PdSpec, n).offset, n
    # sizeof and offsetof as the C compiler lays the header's struct out
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptnn.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ptnn_shapley_spec));\n'
                   + "".join(f'    printf("{n} %zu\\n", offsetof(ptnn_shapley_spec, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert int(lines[0]) == C.sizeof(cls)
    assert {ln.split()[0]: int(ln.split()[1]) for ln in lines[1:] if ln} == {n: getattr(cls, n).offset for n in names}
    # and the library's own sizeof, through the struct_bytes refusal
    lib = binding.load_library()
    assert lib.ptnn_coalition_values(None, None) == -1 and "null argument" in lib.ptnn_last_error().decode()
    for size in (0, C.sizeof(cls) + 1, C.sizeof(binding.PdSpec)):
        spec = cls()
        spec.struct_bytes = size
        assert lib.ptnn_coalition_values(None, C.byref(spec)) == -1
        assert f"ptnn_shapley_spec.struct_bytes = {size}, expected {C.sizeof(cls)}" in lib.ptnn_last_error().decode()


# ---- the library's argument checks, before the handle ----
BG = np.zeros((3, 4), np.float32)
MASKS = np.array([0, 5, 15], np.uint64)
COEF = np.array([[1.0, 0.0], [-0.5, 0.25], [0.0, 1.0]])
VALID = dict(nsteps=10, thin=1, x_source=1, n_rows=5, background=BG, n_background=3, masks=MASKS, coef=COEF, n_coalitions=3, n_terms=2)
W = np.zeros((2, 31), np.float32)
NAN_COEF, INF_COEF = COEF.copy(), COEF.copy()
NAN_COEF[2, 1] = np.nan
INF_COEF[1, 0] = -np.inf
FAULTS = [
    # ptnn_sensitivity's checks, in its order
    ("thin_zero", dict(thin=0), "thin = 0 must be >= 1"),
    ("replicas_empty", dict(replicas=np.zeros(1, np.int32), n_replicas=0), "n_replicas = 0 with a replica list"),
    ("n_w_zero", dict(w=W, n_w=0), "n_w = 0 host vectors: need at least one"),
    ("x_source_unknown", dict(x_source=7), "x_source = 7"),
    ("x_host_null", dict(x_source=0), "needs x"),
    ("n_rows_zero", dict(n_rows=0), "n_rows = 0 must be >= 1"),
    ("seventeen_ranks", dict(n_ranks=17, ranks=np.arange(17, dtype=np.int64)), "n_ranks = 17 outside [0, 16]"),
    ("ranks_null", dict(n_ranks=2), "n_ranks = 2 but ranks is NULL"),
    ("order_stats_without_ranks", dict(order_stats=np.zeros(10, np.float32)), "order_stats requested without ranks"),
    ("seventeen_ranks2", dict(n_ranks2=17, ranks2=np.arange(17, dtype=np.int64)), "n_ranks = 17 outside [0, 16]"),
    ("ranks2_null", dict(n_ranks2=1), "n_ranks = 1 but ranks is NULL"),
    ("abs_order_stats_without_ranks", dict(abs_order_stats=np.zeros(2, np.float32)), "order_stats requested without ranks"),
    # its own
    ("n_background_zero", dict(n_background=0), "n_background = 0 outside [1, 256]"),
    ("n_background_257", dict(n_background=257), "n_background = 257 outside [1, 256]"),
    ("n_coalitions_zero", dict(n_coalitions=0), "n_coalitions = 0 outside [1, 4096]"),
    ("n_coalitions_4097", dict(n_coalitions=4097), "n_coalitions = 4097 outside [1, 4096]"),
    ("n_terms_zero", dict(n_terms=0), "n_terms = 0 outside [1, 64]"),
    ("n_terms_65", dict(n_terms=65), "n_terms = 65 outside [1, 64]"),
    ("background_null", dict(background=None), "background is NULL"),
    ("masks_null", dict(masks=None), "masks is NULL"),
    ("coef_null", dict(coef=None), "coef is NULL"),
    ("coef_nan", dict(coef=NAN_COEF), "coef[2, 1] = nan (coalition 2, term 1) is not finite"),
    ("coef_inf", dict(coef=INF_COEF), "coef[1, 0] = -inf (coalition 1, term 0) is not finite"),
    # two faults at once: the order of the checks
    ("thin_zero_and_x_source_unknown", dict(thin=0, x_source=7), "thin = 0"),
    ("n_rows_zero_and_seventeen_ranks", dict(n_rows=0, n_ranks=17, ranks=np.arange(17, dtype=np.int64)), "n_rows = 0"),
    ("ranks2_null_and_n_background_zero", dict(n_ranks2=1, n_background=0), "n_ranks = 1 but"),
    ("n_background_zero_and_n_coalitions_zero", dict(n_background=0, n_coalitions=0), "n_background = 0"),
    ("n_coalitions_zero_and_n_terms_zero", dict(n_coalitions=0, n_terms=0), "n_coalitions = 0"),
    ("n_terms_65_and_background_null", dict(n_terms=65, background=None), "n_terms = 65"),
    ("background_null_and_masks_null", dict(background=None, masks=None), "background is NULL"),
    ("masks_null_and_coef_null", dict(masks=None, coef=None), "masks is NULL"),
    ("coef_inf_and_coef_nan", dict(coef=np.where(np.isnan(NAN_COEF), np.nan, INF_COEF)), "coef[1, 0] = -inf"),
]


def _call(binding, fields):
    cls = binding.ShapSpec
    spec, keep, types = cls(), [], dict(cls._fields_)
    spec.struct_bytes = C.sizeof(cls)
    for name, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(np.ascontiguousarray(v))
            v = keep[-1].ctypes.data_as(types[name])
        setattr(spec, name, v)
    lib = binding.load_library()
    rc = lib.ptnn_coalition_values(None, C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


@pytest.mark.parametrize("fields", [VALID, dict(VALID, masks=np.array([0, 1 << 40, 15], np.uint64)),
                                    dict(VALID, background=np.full((3, 4), np.nan, np.float32)),
                                    dict(VALID, w=W, n_w=2, nsteps=0, thin=0), dict(VALID, x_source=0, x=np.zeros((5, 4), np.float32)),
                                    dict(VALID, n_ranks=16, ranks=np.arange(16, dtype=np.int64), n_ranks2=1, ranks2=np.zeros(1, np.int64),
                                         order_stats=np.zeros(16 * 10, np.float32), abs_order_stats=np.zeros(2, np.float32))],
                         ids=["trace", "mask_bits_checked_with_the_handle", "background_checked_with_the_handle", "host_vectors", "host_rows",
                              "ranks"])
def test_valid_specs_reach_the_handle(binding, fields):
    rc, text = _call(binding, fields)
    assert rc < 0 and "handle" in text.lower(), text


@pytest.mark.parametrize("name, over, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_spec_refusals(binding, name, over, text):
    rc, got = _call(binding, dict(VALID, **over))
    assert rc == -1 and text in got, got
