"""Partial dependence and ICE curves without a GPU: the float64 reference (tests/pd_ref.py) against the oracle's forward pass on
explicitly rebuilt rows and against a closed form, pd_grid against np.percentile with every refusal, the symbol table and the
layout of PdSpec against the header's struct, and the argument checks of ptnn_partial_dependence through the loaded library with a
NULL handle (every call checks its spec before it looks at the handle)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pd_ref as ref
from parity import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__
    __graft_entry__.build()
    sys.path.insert(0, ROOT)
    import ptnn_amd  # noqa: F401
    from ptnn_amd import _lib
    return _lib


# ---- the reference ----
@pytest.mark.parametrize("task,topo", [(orc.TASK_REG, (4, 5, 1)), (orc.TASK_CLS, (6, 7, 3))], ids=["reg", "cls"])
def test_reference_is_the_oracle_on_rebuilt_rows(task, topo):
    I, H, O = topo
    rng = np.random.default_rng(5 + I)
    X = rng.standard_normal((9, I))
    w = rng.standard_normal(orc.num_param(topo))
    inputs, grid = [I - 1, 0, 2], rng.standard_normal((3, 4)) * 2
    got = ref.ice_all(X, w, topo, task, inputs, grid)
    assert got.shape == (9, 3, 4, O)
    for a, j in enumerate(inputs):
        for k in range(4):
            rows = np.array([[grid[a, k] if i == j else X[n, i] for i in range(I)] for n in range(9)])    # rebuilt element by element
            want = orc.forward(rows, w, topo)[1]
            if task == orc.TASK_CLS:
                want = np.exp(want) / np.exp(want).sum(axis=1, keepdims=True)
            assert np.array_equal(got[:, a, k], want) and np.array_equal(ref.ice(X, w, topo, task, j, grid[a, k]), want)
    # a grid value equal to the row's own input gives the row's own output
    own = ref.ice(X[:1], w, topo, task, 2, X[0, 2])
    f = orc.forward(X[:1], w, topo)[1]
    assert np.array_equal(own, np.exp(f) / np.exp(f).sum(axis=1, keepdims=True) if task == orc.TASK_CLS else f)
    T = ref.error_bound_all(X, w, topo, task, inputs, grid)
    assert T.shape == got.shape and np.all(T > 0) and np.all(np.isfinite(T))


def test_reference_closed_form_one_hidden_unit():
    topo = (3, 1, 1)
    sig = lambda t: 1.0 / (1.0 + math.exp(-t))          # noqa: E731
    X = np.array([[0.5, -1.0, 2.0], [0.0, 0.25, -0.75]])
    w = np.array([0.7, -0.3, 0.2, 1.5, 0.1, -0.4])       # W1 [3, 1], W2 [1, 1], B1, B2
    for n in range(2):
        for j in range(3):
            for v in (-2.0, 0.0, 3.5):
                x = X[n].copy()
                x[j] = v
                want = sig(1.5 * sig(0.7 * x[0] - 0.3 * x[1] + 0.2 * x[2] - 0.1) + 0.4)
                assert abs(ref.ice(X, w, topo, orc.TASK_REG, j, v)[n, 0] - want) <= 1e-15


def test_reference_reductions():
    f = np.array([[[0.25], [0.5], [1.0]], [[0.125], [0.125], [0.5]]], np.float32).reshape(2, 3, 1, 1, 1)   # M = 2, 3 rows
    pd = ref.row_means(f)
    assert pd.shape == (2, 1, 1, 1) and pd[0, 0, 0, 0] == 1.75 / 3 and pd[1, 0, 0, 0] == 0.75 / 3
    p32 = np.array([[[[0.25], [1.0], [0.5]]], [[[0.5], [0.5], [0.5]]]], np.float32)                          # [2, 1, 3, 1]
    assert ref.ranges(p32).tolist() == [[[0.75]], [[0.0]]]


# ---- pd_grid ----
def test_pd_grid(binding):
    from ptnn_amd import parallel_tempering as pt
    from ptnn_amd.effects import pd_grid
    assert pt.pd_grid is pd_grid and pt.PartialDependence._fields[:3] == ("inputs", "grid", "pd_mean")
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((37, 5))
    idx, g = pd_grid(rows, None, 16, (5, 95))
    assert idx.dtype == np.int32 and idx.tolist() == [0, 1, 2, 3, 4] and g.dtype == np.float32 and g.shape == (5, 16)
    for j in range(5):
        assert np.array_equal(g[j], np.percentile(rows[:, j], np.linspace(5, 95, 16)).astype(np.float32))
    idx, g = pd_grid(rows, [3, 0], 1, (50, 50))
    assert idx.tolist() == [3, 0] and np.array_equal(g[:, 0], np.median(rows[:, [3, 0]], axis=0).astype(np.float32))
    idx, g = pd_grid(rows, [4], 64, (0, 100))
    assert g.shape == (1, 64) and g[0, 0] == np.float32(rows[:, 4].min()) and g[0, -1] == np.float32(rows[:, 4].max())
    idx, g = pd_grid(rows, [1, 2], [0.5, -1.0, 0.5])                     # one list for every input; repeats and any order
    assert np.array_equal(g, np.array([[0.5, -1.0, 0.5]] * 2, np.float32)) and g.flags.c_contiguous
    idx, g = pd_grid(rows, np.array([2, 1]), np.array([[1.0, 2.0], [3.0, 4.0]]))
    assert idx.tolist() == [2, 1] and g.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    for kw, text in ((dict(inputs=[5]), r"inputs \[5\]: one or more integer indices in \[0, 5\)"), (dict(inputs=[-1]), "integer indices"),
                     (dict(inputs=[]), "integer indices"), (dict(inputs=[0.5]), "integer indices"), (dict(inputs=[[0, 1]]), "integer indices"),
                     (dict(inputs=[1, 3, 1]), "given twice"), (dict(grid=0), "grid = 0 values: between 1 and 64"),
                     (dict(grid=65), "grid = 65 values"), (dict(grid=np.zeros(65)), "grid = 65 values"), (dict(grid=np.zeros((5, 0))), "grid = 0 values"),
                     (dict(grid=np.zeros((4, 3))), r"\[5, G\]"), (dict(grid=np.zeros((5, 3, 1))), "got shape"),
                     (dict(inputs=[0, 1], grid=np.zeros((5, 3))), r"\[2, G\]"),
                     (dict(grid=[0.0, float("nan")]), r"grid\[0, 1\] = nan \(input 0\) is not a finite"),
                     (dict(inputs=[4, 2], grid=[[0.0, 1.0], [float("inf"), 1.0]]), r"grid\[1, 0\] = inf \(input 2\)"),
                     (dict(grid=[1e39]), "not a finite float32"),
                     (dict(grid_range=(5,)), "pair"), (dict(grid_range="ab"), "pair"), (dict(grid_range=(-1, 95)), "0 <= lo <= hi <= 100"),
                     (dict(grid_range=(60, 40)), "0 <= lo <= hi <= 100"), (dict(grid_range=(5, 101)), "0 <= lo <= hi <= 100"),
                     (dict(grid_range=(float("nan"), 50)), "0 <= lo <= hi <= 100")):
        args = dict(inputs=None, grid=8, grid_range=(5, 95))
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            pd_grid(rows, **args)
    # the order of the checks: inputs, then the grid's size, then grid_range, then the values
    with pytest.raises(ValueError, match="given twice"):
        pd_grid(rows, [1, 1], 0, (9, 1))
    with pytest.raises(ValueError, match="grid = 0 values"):
        pd_grid(rows, None, 0, (9, 1))


# ---- the symbol, the ABI and the struct ----
def test_symbol_and_abi(binding):
    assert "ptnn_partial_dependence" in binding.SYMBOLS
    lib = binding.load_library()
    assert lib.ptnn_abi_version() == 4 == binding.ABI_VERSION
    assert lib.ptnn_partial_dependence is not None
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    assert "int ptnn_partial_dependence(ptnn_handle *h, const ptnn_pd_spec *spec);" in header
    assert binding.PD_MAX_GRID == 64 and "#define PTNN_PD_MAX_GRID 64" in header


def _header_fields():
    """The fields of ptnn_pd_spec in the header's order."""
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    body = re.search(r"typedef struct ptnn_pd_spec \{(.*?)\} ptnn_pd_spec;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
    return names


def test_spec_layout_is_the_headers(binding, tmp_path):
    cls = binding.PdSpec
    names = [n for n, _ in cls._fields_]
    assert names == _header_fields()
    # the selection and row fields of ptnn_sensitivity_spec, field for field, open the struct
    shared = ["struct_bytes", "replicas", "n_replicas", "step0", "nsteps", "thin", "w", "multiplicity", "n_w", "x_source", "n_rows", "x"]
    assert names[:12] == shared == [n for n, _ in binding.SensitivitySpec._fields_][:12]
    for n in shared:
        assert getattr(cls, n).offset == getattr(binding.SensitivitySpec, n).offset, n
    # sizeof and offsetof as the C compiler lays the header's struct out
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptnn.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ptnn_pd_spec));\n'
                   + "".join(f'    printf("{n} %zu\\n", offsetof(ptnn_pd_spec, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert int(lines[0]) == C.sizeof(cls)
    assert {ln.split()[0]: int(ln.split()[1]) for ln in lines[1:] if ln} == {n: getattr(cls, n).offset for n in names}
    # and the library's own sizeof, through the struct_bytes refusal
    lib = binding.load_library()
    assert lib.ptnn_partial_dependence(None, None) == -1 and "null argument" in lib.ptnn_last_error().decode()
    for size in (0, C.sizeof(cls) + 1, C.sizeof(binding.SensitivitySpec)):
        spec = cls()
        spec.struct_bytes = size
        assert lib.ptnn_partial_dependence(None, C.byref(spec)) == -1
        assert f"ptnn_pd_spec.struct_bytes = {size}, expected {C.sizeof(cls)}" in lib.ptnn_last_error().decode()


# ---- the library's argument checks, before the handle ----
GRID = np.array([[0.0, 0.5, 1.0], [2.0, -1.0, 2.0]], np.float32)
VALID = dict(nsteps=10, thin=1, x_source=1, n_rows=5, inputs=np.array([3, 0], np.int32), n_inputs=2, grid=GRID, n_grid=3)
W = np.zeros((2, 31), np.float32)
NAN_GRID, INF_GRID = GRID.copy(), GRID.copy()
NAN_GRID[1, 2] = np.nan
INF_GRID[0, 1] = -np.inf
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
    ("ice_order_stats_without_ranks", dict(ice_order_stats=np.zeros(90, np.float32)), "order_stats requested without ranks"),
    ("seventeen_ranks2", dict(n_ranks2=17, ranks2=np.arange(17, dtype=np.int64)), "n_ranks = 17 outside [0, 16]"),
    ("ranks2_null", dict(n_ranks2=1), "n_ranks = 1 but ranks is NULL"),
    ("pd_order_stats_without_ranks", dict(pd_order_stats=np.zeros(6, np.float32)), "order_stats requested without ranks"),
    ("range_order_stats_without_ranks", dict(range_order_stats=np.zeros(2, np.float32)), "order_stats requested without ranks"),
    # its own
    ("n_grid_zero", dict(n_grid=0), "n_grid = 0 outside [1, 64]"),
    ("n_grid_65", dict(n_grid=65), "n_grid = 65 outside [1, 64]"),
    ("grid_null", dict(grid=None), "grid is NULL"),
    ("inputs_empty", dict(n_inputs=0), "n_inputs = 0 with an input list"),
    ("inputs_negative_count", dict(n_inputs=-2), "n_inputs = -2 with an input list"),
    ("grid_nan", dict(grid=NAN_GRID), "grid[1, 2] = nan (input slot 1, position 2) is not finite"),
    ("grid_inf", dict(grid=INF_GRID), "grid[0, 1] = -inf (input slot 0, position 1) is not finite"),
    # two faults at once: the order of the checks
    ("thin_zero_and_x_source_unknown", dict(thin=0, x_source=7), "thin = 0"),
    ("x_source_unknown_and_n_rows_zero", dict(x_source=7, n_rows=0), "x_source = 7"),
    ("n_rows_zero_and_seventeen_ranks", dict(n_rows=0, n_ranks=17, ranks=np.arange(17, dtype=np.int64)), "n_rows = 0"),
    ("ranks_null_and_ranks2_null", dict(n_ranks=2, n_ranks2=1), "n_ranks = 2 but"),
    ("ranks2_null_and_n_grid_zero", dict(n_ranks2=1, n_grid=0), "n_ranks = 1 but"),
    ("n_grid_zero_and_grid_null", dict(n_grid=0, grid=None), "n_grid = 0"),
    ("grid_null_and_inputs_empty", dict(grid=None, n_inputs=0), "grid is NULL"),
    ("inputs_empty_and_grid_nan", dict(n_inputs=0, grid=NAN_GRID), "n_inputs = 0"),
    ("grid_inf_and_grid_nan", dict(grid=np.where(np.isnan(NAN_GRID), np.nan, INF_GRID).astype(np.float32)), "grid[0, 1] = -inf"),
]


def _call(binding, fields):
    cls = binding.PdSpec
    spec, keep, types = cls(), [], dict(cls._fields_)
    spec.struct_bytes = C.sizeof(cls)
    for name, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(np.ascontiguousarray(v))
            v = keep[-1].ctypes.data_as(types[name])
        setattr(spec, name, v)
    lib = binding.load_library()
    rc = lib.ptnn_partial_dependence(None, C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


@pytest.mark.parametrize("fields", [VALID, dict(VALID, inputs=None, n_inputs=0), dict(VALID, inputs=None, grid=NAN_GRID),
                                    dict(VALID, w=W, n_w=2, nsteps=0, thin=0), dict(VALID, x_source=0, x=np.zeros((5, 4), np.float32)),
                                    dict(VALID, n_ranks=16, ranks=np.arange(16, dtype=np.int64), n_ranks2=1, ranks2=np.zeros(1, np.int64),
                                         ice_order_stats=np.zeros(16 * 90, np.float32), range_order_stats=np.zeros(2, np.float32))],
                         ids=["trace", "all_inputs", "all_inputs_grid_checked_with_the_handle", "host_vectors", "host_rows", "ranks"])
def test_valid_specs_reach_the_handle(binding, fields):
    rc, text = _call(binding, fields)
    assert rc < 0 and "handle" in text.lower(), text


@pytest.mark.parametrize("name, over, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_spec_refusals(binding, name, over, text):
    rc, got = _call(binding, dict(VALID, **over))
    assert rc == -1 and text in got, got
