"""Accumulated local effects without a GPU: the float64 reference (tests/ale_ref.py) against closed forms and its own identities,
its net form against the oracle's forward pass on rebuilt rows, a numpy float32 emulation of the device's delta form under the
derived error bound, ale_edges, the symbol table and the layout of AleSpec against the header's struct, the argument checks of
ptnn_accumulated_effects through the loaded library with a NULL handle (every call checks its spec before it looks at the handle),
and the front's argument errors against the recording stand-in for `_lib.Sampler` of tests/test_analysis_front_cpu.py."""
import ast
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ale_ref as ref
import test_analysis_front_cpu as front
from parity import orc
from test_analysis_front_cpu import BAD_ROWS, MANY_PCTS, W, fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__
    __graft_entry__.build()
    sys.path.insert(0, ROOT)
    import ptnn_amd  # noqa: F401
    from ptnn_amd import _lib
    return _lib


# ---- the reference against closed forms
def test_first_order_of_a_square_plus_a_line():
    rng = np.random.default_rng(1)
    X = rng.uniform(-2, 2, (200, 2))
    z = np.percentile(X[:, 0], np.linspace(0, 100, 8))
    f = lambda A: (A[:, 0] ** 2 + A[:, 1])[:, None]                     # noqa: E731
    ale, nk = ref.ale_f(f, X, 0, z)
    assert nk.sum() == 200 and ale.shape == (8, 1)
    g = z ** 2 - z[0] ** 2
    want = g - (nk * g[1:]).sum() / 200
    np.testing.assert_allclose(ale[:, 0], want, rtol=0, atol=1e-12)
    assert abs((nk * ale[1:, 0]).sum()) <= 1e-12                        # sum_k n_k ALE[k] = 0
    # the line: its effect is z_k minus the count-weighted mean, whatever x0 does
    z1 = np.percentile(X[:, 1], np.linspace(0, 100, 5))
    ale1, n1 = ref.ale_f(f, X, 1, z1)
    np.testing.assert_allclose(ale1[:, 0], (z1 - z1[0]) - (n1 * (z1[1:] - z1[0])).sum() / 200, rtol=0, atol=1e-12)


def test_second_order_of_a_product_on_a_cartesian_design():
    u, v = np.array([-1.0, -0.25, 0.5, 2.0, 2.5]), np.array([0.0, 1.0, 1.5, 4.0, 4.5])
    K2 = 4
    X = np.array([[u[k], v[m]] for k in range(1, K2 + 1) for m in range(1, K2 + 1)])      # one row per cell, on its upper corner
    ale2, N = ref.ale2_f(lambda A: (A[:, 0] * A[:, 1])[:, None], X, 0, 1, u, v)
    assert np.all(N == 1)
    a, b = u - u[0], v - v[0]
    want = np.outer(a - a[1:].mean(), b - b[1:].mean())                 # both main effects of the product are removed
    np.testing.assert_allclose(ale2[:, :, 0], want, rtol=0, atol=1e-12)
    bk, bm = ref.bins(X[:, 0], u), ref.bins(X[:, 1], v)
    inter = ref.interaction(ale2.astype(np.float32), bk, bm, K2)
    np.testing.assert_allclose(inter[0], np.sqrt((want[1:, 1:] ** 2).mean()), rtol=1e-6)


def test_an_additive_function_has_no_second_order_effect():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((150, 3))
    u, v = np.percentile(X[:, 2], np.linspace(0, 100, 6)), np.percentile(X[:, 0], np.linspace(0, 100, 6))
    f = lambda A: np.stack([np.sin(A[:, 0]) + A[:, 2] ** 3 + A[:, 1], A[:, 0] - A[:, 2]], axis=1)      # noqa: E731
    ale2, N = ref.ale2_f(f, X, 2, 0, u, v)
    assert N.sum() == 150 and ale2.shape == (6, 6, 2) and np.max(np.abs(ale2)) <= 1e-12


# ---- bins, padding, empty bins
def test_bins_at_below_and_above_the_edges():
    z = np.array([0.0, 1.0, 2.0, 3.0, 3.0, 3.0])                        # K* = 3, two padded edges
    assert ref.last_bin(z) == 3
    x = np.array([-5.0, 0.0, 0.5, 1.0, 1.0000001, 2.0, 2.5, 3.0, 7.0])
    assert ref.bins(x, z).tolist() == [1, 1, 1, 1, 2, 2, 3, 3, 3]
    assert ref.counts(ref.bins(x, z), 5).tolist() == [4, 2, 3, 0, 0]    # a padded bin is always empty


def test_padded_edges_change_nothing():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((80, 2))
    f = lambda A: np.tanh(A[:, :1] * A[:, 1:] + A[:, :1])               # noqa: E731
    z = np.percentile(X[:, 0], np.linspace(0, 100, 5))
    zp = np.concatenate([z, [z[-1]] * 3])
    ale, nk = ref.ale_f(f, X, 0, z)
    alep, nkp = ref.ale_f(f, X, 0, zp)
    assert np.array_equal(alep[:5], ale) and np.all(alep[5:] == ale[4]) and nkp.tolist() == nk.tolist() + [0, 0, 0]
    v = np.percentile(X[:, 1], np.linspace(0, 100, 4))
    s, N = ref.ale2_f(f, X, 0, 1, z, np.concatenate([v, [v[-1]]]))
    sp, Np = ref.ale2_f(f, X, 0, 1, zp[:5], np.concatenate([v, [v[-1]]]))
    assert np.array_equal(s, sp) and np.all(N[:, 3] == 0)
    s0, N0 = ref.ale2_f(f, X, 0, 1, z, np.concatenate([v, [v[-1], v[-1]]])[:5])
    assert np.array_equal(s0[:, :4], s[:, :4]) and np.array_equal(s0[:, 4], s[:, 3])


def test_an_empty_middle_bin_is_a_flat_step():
    X = np.array([[0.1, 0.0], [0.2, 1.0], [0.9, 2.0], [0.95, -1.0], [0.15, 0.5]])
    z = np.array([0.0, 0.25, 0.5, 0.75, 1.0])                           # bins 2 and 3 hold no row
    ale, nk = ref.ale_f(lambda A: np.exp(A[:, :1]) + A[:, 1:], X, 0, z)
    assert nk.tolist() == [3, 0, 0, 2] and ale[1, 0] == ale[2, 0] == ale[3, 0] and ale[4, 0] > ale[3, 0] > ale[0, 0]
    assert abs((nk * ale[1:, 0]).sum()) <= 1e-15


# ---- the net form, its bound, and the device's arithmetic emulated in float32
@pytest.mark.parametrize("task,topo", [(orc.TASK_REG, (4, 5, 1)), (orc.TASK_CLS, (6, 7, 3))], ids=["reg", "cls"])
def test_net_reference_is_the_oracle_on_rebuilt_rows(task, topo):
    I, H, O = topo
    rng = np.random.default_rng(5 + I)
    X = rng.standard_normal((9, I))
    w = rng.standard_normal(orc.num_param(topo))
    z, v = np.array([-0.5, 0.0, 0.75, 0.75]), np.array([-1.0, 0.25, 1.0])
    d, b = ref.local1(X, w, topo, task, 2, z)
    D2, bk, bm = ref.local2(X, w, topo, task, 2, 0, z, v)
    assert np.array_equal(b, bk)

    def f(n, xj, xl=None):                                              # rebuilt element by element
        row = np.array([[xj if i == 2 else (xl if i == 0 and xl is not None else X[n, i]) for i in range(I)]])
        out = orc.forward(row, w, topo)[1]
        return (np.exp(out) / np.exp(out).sum(axis=1, keepdims=True))[0] if task == orc.TASK_CLS else out[0]
    for n in range(9):                  # one row at a time sums in another order than the batch: a few float64 roundings apart
        assert np.all(np.abs(d[n] - (f(n, z[b[n]]) - f(n, z[b[n] - 1]))) <= 1e-14)
        want = (f(n, z[bk[n]], v[bm[n]]) - f(n, z[bk[n] - 1], v[bm[n]])) - (f(n, z[bk[n]], v[bm[n] - 1]) - f(n, z[bk[n] - 1], v[bm[n] - 1]))
        assert np.all(np.abs(D2[n] - want) <= 1e-14)
    T1, T2 = ref.bound1(X, w, topo, task, 2, z), ref.bound2(X, w, topo, task, 2, 0, z, v)
    assert T1.shape == d.shape and T2.shape == D2.shape and np.all(T1 > 0) and np.all(T2 > T1 * 0) and np.all(np.isfinite(T2))


@pytest.mark.parametrize("task,topo", [(orc.TASK_REG, (4, 5, 1)), (orc.TASK_REG, (5, 90, 1)), (orc.TASK_CLS, (4, 30, 3)), (orc.TASK_CLS, (6, 40, 18))],
                         ids=["reg-4-5-1", "reg-5-90-1", "cls-4-30-3", "cls-6-40-18"])
def test_float32_emulation_of_the_delta_form_is_within_the_bound(task, topo):
    """The device's arithmetic in numpy float32 against the float64 reference: err <= u T with room, before any GPU run."""
    I, H, O = topo
    rng = np.random.default_rng(17 + H)
    X32 = rng.standard_normal((65, I)).astype(np.float32)
    X = X32.astype(np.float64)
    z = np.percentile(X[:, 1], np.linspace(0, 100, 5)).astype(np.float32)
    v = np.percentile(X[:, 3], [0, 50, 100]).astype(np.float32)
    u2 = np.percentile(X[:, 1], [0, 50, 100]).astype(np.float32)
    worst1 = worst2 = 0.0
    for k in range(3):
        w32 = (rng.standard_normal(orc.num_param(topo)) * 0.8).astype(np.float32)
        w = w32.astype(np.float64)
        d, b = ref.local1(X, w, topo, task, 1, z.astype(np.float64))
        dev = (ref.emulate(X32, w32, topo, task, 1, z[b]).astype(np.float64) - ref.emulate(X32, w32, topo, task, 1, z[b - 1])).astype(np.float32)
        worst1 = max(worst1, float(np.max(np.abs(dev - d) / (ref.U32 * ref.bound1(X, w, topo, task, 1, z.astype(np.float64))))))
        D2, bk, bm = ref.local2(X, w, topo, task, 1, 3, u2.astype(np.float64), v.astype(np.float64))
        e = lambda a, c: ref.emulate(X32, w32, topo, task, 1, a, 3, c).astype(np.float64)      # noqa: E731
        dev2 = ((e(u2[bk], v[bm]) - e(u2[bk - 1], v[bm])) - (e(u2[bk], v[bm - 1]) - e(u2[bk - 1], v[bm - 1]))).astype(np.float32)
        worst2 = max(worst2, float(np.max(np.abs(dev2 - D2) / (ref.U32 * ref.bound2(X, w, topo, task, 1, 3, u2.astype(np.float64), v.astype(np.float64))))))
    print(f"float32 emulation {topo}: worst err / (u T1) = {worst1:.4f}, worst err / (u T2) = {worst2:.4f}")
    assert worst1 <= 1.0 and worst2 <= 1.0


def test_reference_reductions_follow_the_stated_order():
    d = np.array([[[0.25], [0.5], [1.0], [0.125]]], np.float32)         # one sample, 4 rows
    b = np.array([1, 3, 1, 3])
    m = ref.bin_means(d, b, 3)
    assert m[0, :, 0].tolist() == [0.625, 0.0, 0.3125]
    ale = ref.curve(d, b, 3)
    g = np.array([0.0, 0.625, 0.625, 0.9375])
    assert np.array_equal(ale[0, :, 0], g - (2 * 0.625 + 2 * 0.9375) / 4)
    assert ref.ranges(ale.astype(np.float32))[0, 0] == np.float32(0.9375)


# ---- ale_edges
def test_ale_edges(binding):
    from ptnn_amd import ale, parallel_tempering as pt
    assert pt.ale_edges is ale.ale_edges and pt.AccumulatedEffects._fields[:3] == ("inputs", "edges", "bin_count")
    assert pt.ParallelTemperingBase.accumulated_effects is ale.accumulated_effects
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((37, 5))
    e = ale.ale_edges(rows, [3, 0], 8)
    assert e.dtype == np.float32 and e.shape == (2, 9)
    for a, j in enumerate((3, 0)):
        assert np.array_equal(e[a], np.percentile(rows[:, j], np.linspace(0, 100, 9)).astype(np.float32))
    # a column with ties: duplicate quantiles removed, the tail padded with the last edge
    rows[:, 1] = np.repeat([0.0, 1.0, 2.5], [20, 10, 7])
    e = ale.ale_edges(rows, [1, 2], 6)
    assert e[0].tolist() == [0.0, 1.0, 2.5, 2.5, 2.5, 2.5, 2.5] and np.all(np.diff(e[1]) > 0)
    assert ale._strip(e[0]).tolist() == [0.0, 1.0, 2.5] and ale._strip(e[1]).size == 7
    assert ale.ale_edges(rows, [4], 63).shape == (1, 64) and ale.ale_edges(rows, [4], 15, 16).shape == (1, 16)
    rows[:, 2] = 4.0
    for args, text in ((([0], 0), "bins = 0"), (([0], 64), "bins = 64"), (([0], 16, 16), "between 1 and 15"), (([0], True), "bins = True"),
                       (([0], 2.0), "bins = 2.0"), (([0, 2], 4), "input 2: its column needs two distinct finite values")):
        with pytest.raises(ValueError, match=text):
            ale.ale_edges(rows, *args)


# ---- the symbol, the ABI and the struct
def test_symbol_and_abi(binding):
    assert "ptnn_accumulated_effects" in binding.SYMBOLS
    lib = binding.load_library()
    assert lib.ptnn_abi_version() == 4 == binding.ABI_VERSION
    assert lib.ptnn_accumulated_effects is not None
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    assert "int ptnn_accumulated_effects(ptnn_handle *h, const ptnn_ale_spec *spec);" in header
    for name, value in (("EDGES", 64), ("EDGES2", 16), ("PAIRS", 16)):
        assert getattr(binding, "ALE_MAX_" + name) == value and f"#define PTNN_ALE_MAX_{name} {value}" in header


def _header_fields():
    header = open(os.path.join(ROOT, "include", "ptnn.h")).read()
    body = re.search(r"typedef struct ptnn_ale_spec \{(.*?)\} ptnn_ale_spec;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", part.split()[-1]) for part in decl.split(",")]
    return names


def test_spec_layout_is_the_headers(binding, tmp_path):
    cls = binding.AleSpec
    names = [n for n, _ in cls._fields_]
    assert names == _header_fields()
    # the selection and row fields of ptnn_pd_spec, field for field, open the struct
    assert names[:14] == [n for n, _ in binding.PdSpec._fields_][:14]
    for n in names[:14]:
        assert getattr(cls, n).offset == getattr(binding.PdSpec, n).offset, n
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptnn.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ptnn_ale_spec));\n'
                   + "".join(f'    printf("{n} %zu\\n", offsetof(ptnn_ale_spec, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert int(lines[0]) == C.sizeof(cls)
    assert {ln.split()[0]: int(ln.split()[1]) for ln in lines[1:] if ln} == {n: getattr(cls, n).offset for n in names}
    lib = binding.load_library()
    assert lib.ptnn_accumulated_effects(None, None) == -1 and "null argument" in lib.ptnn_last_error().decode()
    for size in (0, C.sizeof(cls) + 1, C.sizeof(binding.PdSpec)):
        spec = cls()
        spec.struct_bytes = size
        assert lib.ptnn_accumulated_effects(None, C.byref(spec)) == -1
        assert f"ptnn_ale_spec.struct_bytes = {size}, expected {C.sizeof(cls)}" in lib.ptnn_last_error().decode()


# ---- the library's argument checks, before the handle
EDGES = np.array([[0.0, 0.5, 1.0, 1.0], [-1.0, 2.0, 3.0, 4.0]], np.float32)
PAIRS = np.array([[0, 2], [3, 2]], np.int32)
EDGES2 = np.array([[[0.0, 1.0, 2.0], [0.0, 1.0, 1.0]], [[-1.0, 0.0, 5.0], [0.5, 1.0, 1.5]]], np.float32)
VALID = dict(nsteps=10, thin=1, x_source=1, n_rows=5, inputs=np.array([3, 0], np.int32), n_inputs=2, edges=EDGES, n_edges=4,
             pairs=PAIRS, n_pairs=2, edges2=EDGES2, n_edges2=3)
WH = np.zeros((2, 31), np.float32)


def _edit(a, idx, v):
    b = a.copy()
    b[idx] = v
    return b


FAULTS = [
    # ptnn_partial_dependence's checks, in its order
    ("thin_zero", dict(thin=0), "thin = 0 must be >= 1"),
    ("replicas_empty", dict(replicas=np.zeros(1, np.int32), n_replicas=0), "n_replicas = 0 with a replica list"),
    ("n_w_zero", dict(w=WH, n_w=0), "n_w = 0 host vectors: need at least one"),
    ("x_source_unknown", dict(x_source=7), "x_source = 7"),
    ("x_host_null", dict(x_source=0), "needs x"),
    ("n_rows_zero", dict(n_rows=0), "n_rows = 0 must be >= 1"),
    ("seventeen_ranks", dict(n_ranks=17, ranks=np.arange(17, dtype=np.int64)), "n_ranks = 17 outside [0, 16]"),
    ("ranks_null", dict(n_ranks=2), "n_ranks = 2 but ranks is NULL"),
    ("local_order_stats_without_ranks", dict(local_order_stats=np.zeros(20, np.float32)), "order_stats requested without ranks"),
    ("seventeen_ranks2", dict(n_ranks2=17, ranks2=np.arange(17, dtype=np.int64)), "n_ranks = 17 outside [0, 16]"),
    ("ranks2_null", dict(n_ranks2=1), "n_ranks = 1 but ranks is NULL"),
    ("ale_order_stats_without_ranks", dict(ale_order_stats=np.zeros(8, np.float32)), "order_stats requested without ranks"),
    ("range_order_stats_without_ranks", dict(range_order_stats=np.zeros(2, np.float32)), "order_stats requested without ranks"),
    ("ale2_order_stats_without_ranks", dict(ale2_order_stats=np.zeros(18, np.float32)), "order_stats requested without ranks"),
    ("inter_order_stats_without_ranks", dict(inter_order_stats=np.zeros(2, np.float32)), "order_stats requested without ranks"),
    # its own
    ("n_pairs_negative", dict(n_pairs=-1), "n_pairs = -1 outside [0, 16]"),
    ("n_pairs_17", dict(n_pairs=17), "n_pairs = 17 outside [0, 16]"),
    ("no_term", dict(edges=None, n_pairs=0), "no term: edges is NULL"),
    ("n_edges_one", dict(n_edges=1), "n_edges = 1 outside [2, 64]"),
    ("n_edges_65", dict(n_edges=65), "n_edges = 65 outside [2, 64]"),
    ("inputs_empty", dict(n_inputs=0), "n_inputs = 0 with an input list"),
    ("edge_nan", dict(edges=_edit(EDGES, (1, 2), np.nan)), "edges[1, 2] = nan (row 1, position 2) is not finite"),
    ("edge_inf", dict(edges=_edit(EDGES, (0, 3), np.inf)), "edges[0, 3] = inf (row 0, position 3) is not finite"),
    ("first_bin_without_width", dict(edges=_edit(EDGES, (0, 1), 0.0)), "edges[0, 1] = 0 <= edges[0, 0] = 0: the first bin needs a width"),
    ("first_edges_decrease", dict(edges=_edit(EDGES, (1, 1), -2.0)), "edges[1, 1] = -2 <= edges[1, 0] = -1"),
    ("edges_decrease", dict(edges=_edit(EDGES, (1, 3), 2.5)), "edges[1, 3] = 2.5 < edges[1, 2] = 3: edges increase"),
    ("edges_increase_after_padding", dict(edges=np.array([[0.0, 1.0, 1.0, 2.0], [0.0, 1.0, 2.0, 3.0]], np.float32)),
     "edges[0, 3] = 2 increases after repeated edges"),
    ("pairs_null", dict(pairs=None), "n_pairs = 2 but pairs is NULL"),
    ("n_edges2_one", dict(n_edges2=1), "n_edges2 = 1 outside [2, 16]"),
    ("n_edges2_17", dict(n_edges2=17), "n_edges2 = 17 outside [2, 16]"),
    ("edges2_null", dict(edges2=None), "edges2 is NULL"),
    ("edge2_nan", dict(edges2=_edit(EDGES2, (1, 0, 2), np.nan)), "edges2[2, 2] = nan (row 2, position 2) is not finite"),
    ("edge2_first_bin", dict(edges2=_edit(EDGES2, (0, 1, 1), -1.0)), "edges2[1, 1] = -1 <= edges2[1, 0] = 0"),
    ("pair_of_one_input", dict(pairs=np.array([[0, 2], [3, 3]], np.int32)), "pairs[1] = (3, 3): a pair needs two different inputs"),
    ("pair_twice", dict(pairs=np.array([[0, 2], [0, 2]], np.int32)), "pairs[1] = (0, 2) is given twice (pairs[0])"),
    ("pair_twice_reversed", dict(pairs=np.array([[0, 2], [2, 0]], np.int32)), "pairs[1] = (2, 0) is given twice (pairs[0])"),
    # two faults at once: the order of the checks
    ("thin_zero_and_x_source_unknown", dict(thin=0, x_source=7), "thin = 0"),
    ("n_rows_zero_and_n_pairs_17", dict(n_rows=0, n_pairs=17), "n_rows = 0"),
    ("ranks2_null_and_n_edges_one", dict(n_ranks2=1, n_edges=1), "n_ranks = 1 but"),
    ("n_pairs_17_and_n_edges_one", dict(n_pairs=17, n_edges=1), "n_pairs = 17"),
    ("n_edges_one_and_inputs_empty", dict(n_edges=1, n_inputs=0), "n_edges = 1"),
    ("edge_nan_and_pairs_null", dict(edges=_edit(EDGES, (1, 2), np.nan), pairs=None), "edges[1, 2] = nan"),
    ("edges2_null_and_pair_twice", dict(edges2=None, pairs=np.array([[0, 2], [2, 0]], np.int32)), "edges2 is NULL"),
    ("edge2_nan_and_pair_of_one_input", dict(edges2=_edit(EDGES2, (1, 0, 2), np.nan), pairs=np.array([[1, 1], [0, 2]], np.int32)), "edges2[2, 2] = nan"),
]


def _call(binding, fields):
    cls = binding.AleSpec
    spec, keep, types = cls(), [], dict(cls._fields_)
    spec.struct_bytes = C.sizeof(cls)
    for name, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(np.ascontiguousarray(v))
            v = keep[-1].ctypes.data_as(types[name])
        setattr(spec, name, v)
    lib = binding.load_library()
    rc = lib.ptnn_accumulated_effects(None, C.byref(spec))
    return rc, lib.ptnn_last_error().decode()


@pytest.mark.parametrize("fields", [VALID, dict(VALID, inputs=None, n_inputs=0), dict(VALID, inputs=None, edges=_edit(EDGES, (0, 0), np.nan)),
                                    dict(VALID, n_pairs=0, pairs=None, edges2=None, n_edges2=0), dict(VALID, edges=None, inputs=None, n_edges=0),
                                    dict(VALID, w=WH, n_w=2, nsteps=0, thin=0), dict(VALID, x_source=0, x=np.zeros((5, 4), np.float32)),
                                    dict(VALID, n_ranks=16, ranks=np.arange(16, dtype=np.int64), n_ranks2=1, ranks2=np.zeros(1, np.int64),
                                         local_order_stats=np.zeros(16 * 20, np.float32), inter_order_stats=np.zeros(2, np.float32))],
                         ids=["trace", "all_inputs", "all_inputs_edges_checked_with_the_handle", "first_order_only", "pairs_only", "host_vectors",
                              "host_rows", "ranks"])
def test_valid_specs_reach_the_handle(binding, fields):
    rc, text = _call(binding, fields)
    assert rc < 0 and "handle" in text.lower(), text


@pytest.mark.parametrize("name, over, text", FAULTS, ids=[f[0] for f in FAULTS])
def test_spec_refusals(binding, name, over, text):
    rc, got = _call(binding, dict(VALID, **over))
    assert rc == -1 and text in got, got


# ---- the front's argument errors against the stand-in sampler
class AleStandIn(front.StandIn):
    def accumulated_effects(self, *args, **kw):
        self._log("accumulated_effects", args, kw)
        n, O, M = self._n_rows(args[0]), self.O, self._count(kw)
        A, E = np.asarray(kw["edges"]).shape
        Q = 0 if kw["pairs"] is None else len(kw["pairs"])
        E2 = np.asarray(kw["edges2"]).shape[2] if Q else 0
        k, k2, T = len(kw["ranks"]), len(kw["ranks2"]), A + Q
        f32 = lambda shape, salt: fill(shape, salt, dtype=np.float32)     # noqa: E731
        return dict(bin_count=np.ones((A, E - 1), np.int64), cell_count=np.ones((Q, E2 - 1, E2 - 1), np.int64) if Q else None,
                    ale_mean=fill((A, E, O), 1), ale_order_stats=f32((k2, A, E, O), 2) if k2 else None, range_mean=fill((A, O), 3),
                    range_order_stats=f32((k2, A, O), 4) if k2 else None, sample_ale=f32((M, A, E, O), 5), sample_range=f32((M, A, O), 6),
                    ale2_mean=fill((Q, E2, E2, O), 7) if Q else None, ale2_order_stats=f32((k2, Q, E2, E2, O), 8) if Q and k2 else None,
                    inter_mean=fill((Q, O), 9) if Q else None, inter_order_stats=f32((k2, Q, O), 10) if Q and k2 else None,
                    sample_ale2=f32((M, Q, E2, E2, O), 11) if Q else None, sample_inter=f32((M, Q, O), 12) if Q else None,
                    local_mean=fill((n, T, O), 13) if kw["local_mean"] else None, local_order_stats=f32((k, n, T, O), 14) if k else None,
                    samples=f32((M, n, T, O), 15) if kw["samples"] else None, n_samples=M, n_distinct=-(-M // 2))


def make(key, calls):
    pt = front.make(key, calls)
    if isinstance(pt._sampler, front.StandIn):
        s = object.__new__(AleStandIn)
        s.__dict__.update(pt._sampler.__dict__)
        pt._sampler = s
    return pt


def refused(key, text, *args, **kw):
    calls = []
    with pytest.raises(ValueError, match=text):
        make(key, calls).accumulated_effects(*args, **kw)
    assert calls == []                                                  # refused before the device is asked for anything


def test_front_valid_calls(binding):
    from ptnn_amd import ale
    calls = []
    pt = make("reg", calls)
    res = pt.accumulated_effects()
    (tag, fn, args, got), = calls
    assert (tag, fn, args) == ("self", "accumulated_effects", ["train"])
    M = 120
    spots, ranks = pt._band_ranks(M, [5, 95])
    rows = np.asarray(pt.traindata)[:, :4].astype(np.float32)
    want = dict(replicas=None, step0=10, nsteps=30, thin=1, inputs=np.arange(4, dtype=np.int32), edges=ale.ale_edges(rows, range(4), 16),
                pairs=None, edges2=None, ranks=[], ranks2=ranks, local_mean=False, sample_ale=True, sample_range=True, sample_ale2=False,
                sample_inter=False, samples=False)
    assert got == front.enc(want)
    assert res.n_samples == M and res.inputs.tolist() == [0, 1, 2, 3] and len(res.edges) == 4 and res.edges[0].dtype == np.float64
    assert res.pairs is None and res.pair_edges is None and res.ale2_mean is None and res.ale2_percentiles == {} and res.interaction is None
    assert res.local_mean is None and res.local_percentiles == {} and res.samples is None
    assert np.array_equal(res.ale_percentiles[5], pt._bands(fill((len(ranks), 4, 17, 1), 2, dtype=np.float32), [5, 95], spots, ranks)[5])
    sr = fill((M, 4, 1), 6, dtype=np.float32)
    assert np.array_equal(res.top_prob, np.stack([(np.argmax(sr, axis=1) == a).sum(axis=0) for a in range(4)]) / M)
    # pairs="all", explicit edges and pair edges, local effects and samples, host weights
    calls.clear()
    res = pt.accumulated_effects("test", inputs=[3, 1, 0], edges=[[0.0, 0.5, 1.0], [0.0, 1.0], [0.25, 0.5, 0.75, 1.0]], pairs="all",
                                 pair_bins=3, local=True, return_samples=True, weights=W, percentiles=[50])
    got = dict(calls[0][3]["d"])
    assert got["'pairs'"] == front.enc(np.array([[3, 1], [3, 0], [1, 0]], np.int32))
    assert got["'edges'"] == front.enc(np.array([[0, 0.5, 1, 1], [0, 1, 1, 1], [0.25, 0.5, 0.75, 1]], np.float32))
    assert got["'ranks'"] == got["'ranks2'"] and got["'local_mean'"] is True and got["'samples'"] is True and got["'sample_inter'"] is True
    assert [e.tolist() for e in res.edges] == [[0.0, 0.5, 1.0], [0.0, 1.0], [0.25, 0.5, 0.75, 1.0]]
    assert res.pairs.tolist() == [[3, 1], [3, 0], [1, 0]] and len(res.pair_edges) == 3 and res.cell_count.shape == (3, 3, 3)
    assert res.interaction.shape == (3, 1) and sorted(res.interaction_percentiles) == [50] and res.local_mean.shape == (pt._sampler.nte, 6, 1)
    calls.clear()
    res = pt.accumulated_effects(inputs=[2], bins=4, pairs=[(0, 1)], pair_edges=[([0.0, 1.0], [0.0, 0.5, 1.0])], percentiles=())
    got = dict(calls[0][3]["d"])
    assert got["'edges2'"] == front.enc(np.array([[[0, 1, 1], [0, 0.5, 1]]], np.float32)) and got["'ranks2'"] == []
    assert res.ale_percentiles == {} and res.pair_edges[0][0].tolist() == [0.0, 1.0]


FRONT_FAULTS = [
    ("x_unknown_name", ("valid",), {}, "x must be 'train', 'test' or an array, not 'valid'"),
    ("x_too_few_columns", (BAD_ROWS,), {}, "at least n_in = 4 columns"),
    ("input_out_of_range", (), dict(inputs=[0, 4]), r"integer indices in \[0, 4\)"), ("inputs_empty", (), dict(inputs=[]), "integer indices"),
    ("input_twice", (), dict(inputs=[2, 2]), "given twice"),
    ("bins_zero", (), dict(bins=0), "bins = 0: an integer between 1 and 63"), ("bins_64", (), dict(bins=64), "bins = 64"),
    ("constant_column", (np.concatenate([fill((9, 3), 2), np.ones((9, 1))], axis=1),), {}, "input 3: its column needs two distinct"),
    ("edges_wrong_count", (), dict(edges=[[0.0, 1.0]]), r"one array per selected input \(4\), got 1"),
    ("edges_nan", (), dict(inputs=[1], edges=[[0.0, np.nan]]), r"edges\[0\]: an edge is not a finite float32"),
    ("edges_not_increasing", (), dict(inputs=[1], edges=[[0.0, 1.0, 1.0]]), r"edges\[0\]: at least two edges, strictly increasing"),
    ("edges_one", (), dict(inputs=[1], edges=[[0.0]]), "at least two edges"),
    ("edges_65", (), dict(inputs=[1], edges=[np.arange(65.0)]), r"edges\[0\] = 65 edges: at most 64"),
    ("pairs_unknown_name", (), dict(pairs="each"), "pairs must be None, 'all' or a list"),
    ("pairs_not_pairs", (), dict(pairs=[0, 1]), r"a list of pairs \(j, l\)"), ("pairs_out_of_range", (), dict(pairs=[(0, 4)]), r"indices in \[0, 4\)"),
    ("pairs_empty", (), dict(pairs=[]), "a list of pairs"),
    ("pairs_17", (), dict(pairs=[(0, 1)] * 17), "17 pairs: at most 16"),
    ("pair_of_one_input", (), dict(pairs=[(1, 1)]), "two different inputs per pair"), ("pair_twice", (), dict(pairs=[(0, 1), (1, 0)]), "no pair twice"),
    ("pair_bins_16", (), dict(pairs="all", pair_bins=16), "between 1 and 15"),
    ("pair_edges_wrong_count", (), dict(pairs=[(0, 1)], pair_edges=[]), r"two arrays per pair \(1 pairs\)"),
    ("pair_edges_17", (), dict(pairs=[(0, 1)], pair_edges=[(np.arange(17.0), [0.0, 1.0])]), r"pair_edges\[0\] = 17 edges: at most 16"),
    ("percentile_above_100", (), dict(percentiles=[5, 101]), "percentiles must lie in"),
    ("no_sample_trace", (), dict(burn_in=1.0), "holds no sample"), ("too_many_percentiles", (), dict(percentiles=MANY_PCTS), "at most 16"),
    # the order of the checks
    ("x_unknown_name_and_input_twice", ("valid",), dict(inputs=[2, 2]), "x must be"), ("input_twice_and_bins_zero", (), dict(inputs=[2, 2], bins=0), "given twice"),
    ("bins_zero_and_pairs_unknown", (), dict(bins=0, pairs="each"), "bins = 0"),
    ("pair_twice_and_percentile_above_100", (), dict(pairs=[(0, 1), (1, 0)], percentiles=[101]), "no pair twice"),
]


@pytest.mark.parametrize("name, args, kw, text", FRONT_FAULTS, ids=[f[0] for f in FRONT_FAULTS])
def test_front_refusals(binding, name, args, kw, text):
    refused("reg", text, *args, **kw)


def test_front_needs_the_handle(binding):
    refused("reg_none", "accumulated_effects needs the chains' device handle")
    refused("reg_sharded", "accumulated_effects runs on one GPU")


def test_every_raise_of_the_module_is_reached(binding):
    from ptnn_amd import ale
    path = inspect.getsourcefile(ale)
    text = open(path).read()
    lines = text.splitlines()
    sites = {n.lineno: lines[n.lineno - 1].strip() for n in ast.walk(ast.parse(text)) if isinstance(n, ast.Raise)}
    assert len(sites) >= 12
    hit = set()

    def local(frame, event, arg):
        if event == "line":
            hit.add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code.co_filename == path else None
    before = sys.gettrace()
    sys.settrace(tracer)
    try:
        for _, args, kw, text in FRONT_FAULTS:
            refused("reg", text, *args, **kw)
    finally:
        sys.settrace(before)
    missed = {t for ln, t in sites.items() if ln not in hit}
    assert missed == set()
