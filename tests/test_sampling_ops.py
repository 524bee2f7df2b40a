"""LinearInterpolator and RegriddingOperator on host fields, and the kernels' per-element bodies run on the host
(tests/emu/emu_sample.cpp): against the reference's own outputs (tests/golden/sampling_ops.npz, written by
tests/golden/make_golden_sampling.py) and against exact longdouble sums within the derived bounds of tests/sampling_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import nifty_amd as ift
from nifty_amd import sampling_operators as so

from tests import sampling_cases as sc
from tests.goldenlib import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = load("sampling_ops")


def interp_case(name):
    spaces = sc.INTERP_CASES[name]
    shape, dist = sc.grid_of(spaces)
    points = Z[f"interp.{name}.points"]
    op = ift.LinearInterpolator(tuple(ift.RGSpace(shp, dst) for shp, dst in spaces), points)
    return op, shape, dist, points


def regrid_case(name):
    desc, new_shape, space = sc.REGRID_CASES[name]
    dom = tuple(ift.RGSpace(v) if kind == "rg" else ift.UnstructuredDomain(v) for kind, v in desc)
    return ift.RegriddingOperator(dom, new_shape, space)


check = sc.check


@pytest.mark.parametrize("name", list(sc.INTERP_CASES))
def test_interpolator_against_golden_and_exact(name):
    op, shape, dist, points = interp_case(name)
    assert points.shape[1] <= 300 and op.target.shape == (points.shape[1],)
    x, y = Z[f"interp.{name}.x"], Z[f"interp.{name}.y"]
    ex = sc.interp_exact(shape, dist, points, x, y)
    bd = sc.interp_bounds(shape, ex)
    t = op(ift.makeField(op.domain, x)).asnumpy()
    a = op.adjoint(ift.makeField(op.target, y)).asnumpy()
    assert t.dtype == np.float64 and a.dtype == np.float64 and a.shape == shape
    check(t, ex["times"], bd["times"], "TIMES vs exact")
    check(a, ex["adjoint"], bd["adjoint"], "ADJOINT vs exact")
    check(Z[f"interp.{name}.times"], ex["times"], bd["times"], "reference TIMES vs exact")
    check(Z[f"interp.{name}.adjoint"], ex["adjoint"], bd["adjoint"], "reference ADJOINT vs exact")
    check(t, Z[f"interp.{name}.times"], bd["times"], "TIMES vs golden", 2.0)  # two rounded sides
    check(a, Z[f"interp.{name}.adjoint"], bd["adjoint"], "ADJOINT vs golden", 2.0)


@pytest.mark.parametrize("name", list(sc.INTERP_CASES))
def test_interpolator_single_precision_and_complex(name):
    op, shape, dist, points = interp_case(name)
    x, y = Z[f"interp.{name}.x"].astype(np.float32), Z[f"interp.{name}.y"].astype(np.float32)
    ex = sc.interp_exact(shape, dist, points, x, y)
    bd = sc.interp_bounds(shape, ex, single=True)
    t, a = op(ift.makeField(op.domain, x)), op.adjoint(ift.makeField(op.target, y))
    assert t.val.dtype == torch.float32 and a.val.dtype == torch.float32
    check(t.asnumpy(), ex["times"], bd["times"], "fp32 TIMES vs exact")
    check(a.asnumpy(), ex["adjoint"], bd["adjoint"], "fp32 ADJOINT vs exact")
    # complex fields: the real map on both planes
    xc = Z[f"interp.{name}.x"] + 1j * Z[f"interp.{name}.x"][::-1]
    tc = op(ift.makeField(op.domain, xc)).asnumpy()
    assert tc.dtype == np.complex128
    np.testing.assert_array_equal(tc.real, op(ift.makeField(op.domain, xc.real.copy())).asnumpy())
    np.testing.assert_array_equal(tc.imag, op(ift.makeField(op.domain, xc.imag.copy())).asnumpy())
    yc = (Z[f"interp.{name}.y"] * (1 + 2j)).astype(np.complex64)
    ac = op.adjoint(ift.makeField(op.target, yc))
    assert ac.val.dtype == torch.complex64


@pytest.mark.parametrize("name", list(sc.INTERP_CASES))
def test_interpolator_is_a_consistent_linear_operator(name):
    op = interp_case(name)[0]
    ift.extra.check_linear_operator(op, np.float64, np.float64, atol=1e-12, rtol=1e-12)


def test_interpolator_wraps_far_points_and_is_exact_on_nodes():
    sp = ift.RGSpace((5, 7), (0.2, 1.12))
    x = np.random.default_rng(1).standard_normal(sp.shape)
    nodes = np.array([[3 * 0.2, 0.0, 4 * 0.2], [2 * 1.12, 6 * 1.12, 6 * 1.12]])
    got = ift.LinearInterpolator(sp, nodes)(ift.makeField(sp, x)).asnumpy()
    np.testing.assert_allclose(got, [x[3, 2], x[0, 6], x[4, 6]], rtol=1e-14)
    period = np.array([[1.0], [7 * 1.12]])
    base = np.array([[0.37], [3.3]])
    ref = ift.LinearInterpolator(sp, base)(ift.makeField(sp, x)).asnumpy()
    for k in (-1000, -1, 1, 12345):
        far = ift.LinearInterpolator(sp, base + k * period)(ift.makeField(sp, x)).asnumpy()
        np.testing.assert_allclose(far, ref, rtol=1e-9)  # (the far position itself carries |k| ulps of the period)
    last = ift.LinearInterpolator(sp, np.array([[4.5 * 0.2], [6.5 * 1.12]]))(ift.makeField(sp, x)).asnumpy()
    np.testing.assert_allclose(last, 0.25 * (x[4, 6] + x[0, 6] + x[4, 0] + x[0, 0]), rtol=1e-13)


def test_interpolator_argument_errors():
    sp = ift.RGSpace((4, 4))
    with pytest.raises(TypeError):
        ift.LinearInterpolator(ift.UnstructuredDomain(5), np.zeros((1, 3)))
    with pytest.raises(TypeError):
        ift.LinearInterpolator((ift.RGSpace(4), ift.RGSpace((4, 4))), np.zeros((3, 3)))
    with pytest.raises(TypeError):
        ift.LinearInterpolator(sp, np.zeros((3, 5)))
    with pytest.raises(TypeError):
        ift.LinearInterpolator(sp, np.zeros(5))
    with pytest.raises(TypeError):
        ift.LinearInterpolator(sp, [[0.0, 1.0], [0.0, 1.0]])
    op = ift.LinearInterpolator(sp, np.zeros((2, 3)))
    assert op.capability == op.TIMES | op.ADJOINT_TIMES and op.target[0] == ift.UnstructuredDomain(3)
    empty = ift.LinearInterpolator(sp, np.zeros((2, 0)))
    assert empty.adjoint(ift.full(empty.target, 1.0)).asnumpy().shape == (4, 4)


def test_interpolator_on_four_axes_on_the_host():
    sp = ift.RGSpace((3, 4, 2, 5))
    rng = np.random.default_rng(3)
    pts = rng.random((4, 50)) * 2 - 0.5
    op = ift.LinearInterpolator(sp, pts)
    x = rng.standard_normal(sp.shape)
    ex = sc.interp_exact(sp.shape, sp.distances, pts, x)
    # 2^4 - 1 additions and 2 * 4 steps per term: k = 2^d + 2 d - 1 (the d <= 3 form 2^d + d + 2 is one short here)
    ok, worst = sc.err_ok(op(ift.makeField(sp, x)).asnumpy(), ex["times"], (sc.gamma(16 + 8 - 1) * ex["times_abs"]).astype(np.float64))
    assert ok, worst
    ift.extra.check_linear_operator(op, np.float64, np.float64, atol=1e-12, rtol=1e-12, _device_ids_override=[-1])


def test_plan_size_does_not_depend_on_the_grid():
    rng = np.random.default_rng(5)
    pts = rng.random((3, 10000))
    small = so.InterpolationPlan((16, 16, 16), (1 / 16,) * 3, pts)
    big = so.InterpolationPlan((1024, 1024, 1024), (1 / 1024,) * 3, pts)
    assert big.nbytes <= (8 * 3 + 24) * 10000 + 8 and small.nbytes <= big.nbytes
    for plan in (small, big):
        assert np.all(np.diff(plan.cell) >= 0) and sorted(plan.perm) == list(range(10000))
        assert plan.cell_start[0] == 0 and plan.cell_start[-1] == 10000 and np.all(np.diff(plan.cell_start) > 0)
        assert len(np.unique(plan.cell)) == len(plan.cell_start) - 1
    # stable: the points of one cell keep the caller's order
    one = so.InterpolationPlan((4,), (0.25,), np.full((1, 300), 0.3))
    assert list(one.perm) == list(range(300)) and list(one.long_cell) == [0] and list(one.cell_start) == [0, 300]


@pytest.mark.parametrize("name", list(sc.REGRID_CASES))
def test_regridding_against_golden_and_exact(name):
    op = regrid_case(name)
    shape, axes, old, new, dists, tshape = sc.regrid_layout(sc.REGRID_CASES[name])
    assert op.domain.shape == shape and op.target.shape == tshape
    sp_new = op.target[sc.REGRID_CASES[name][2]]
    assert sp_new.shape == tuple(new) and sp_new.distances == tuple(d * o / n for d, o, n in zip(dists, old, new))
    x, y = Z[f"regrid.{name}.x"], Z[f"regrid.{name}.y"]
    ex = sc.regrid_exact(shape, axes, old, new, dists, x, y)
    for single in (False, True):
        bd = sc.regrid_bounds(ex if not single else sc.regrid_exact(shape, axes, old, new, dists, x.astype(np.float32), y.astype(np.float32)),
                              single)
        e = ex if not single else sc.regrid_exact(shape, axes, old, new, dists, x.astype(np.float32), y.astype(np.float32))
        dt = np.float32 if single else np.float64
        t = op(ift.makeField(op.domain, x.astype(dt)))
        a = op.adjoint(ift.makeField(op.target, y.astype(dt)))
        assert t.asnumpy().dtype == dt and a.asnumpy().dtype == dt
        check(t.asnumpy(), e["times"], bd["times"], f"TIMES vs exact ({dt.__name__})")
        check(a.asnumpy(), e["adjoint"], bd["adjoint"], f"ADJOINT vs exact ({dt.__name__})")
    bd = sc.regrid_bounds(ex)
    check(op(ift.makeField(op.domain, x)).asnumpy(), Z[f"regrid.{name}.times"], bd["times"], "TIMES vs golden", 2.0)
    if f"regrid.{name}.adjoint" in Z.files:
        check(op.adjoint(ift.makeField(op.target, y)).asnumpy(), Z[f"regrid.{name}.adjoint"], bd["adjoint"], "ADJOINT vs golden", 2.0)
    else:  # an axis of old length 1: the identity in both directions here (the reference's adjoint raises)
        assert name == "length_one"
        np.testing.assert_array_equal(op.adjoint(ift.makeField(op.target, y)).asnumpy(), y)
        np.testing.assert_array_equal(op(ift.makeField(op.domain, x)).asnumpy(), x)
    ift.extra.check_linear_operator(op, np.float64, np.float64, atol=1e-12, rtol=1e-12)


def test_regridding_keeps_a_fraction_above_one_at_the_clamped_end():
    op = regrid_case("clamped")
    b, f = sc.regrid_tables(5, 5)
    assert list(b) == [0, 1, 2, 3, 3] and f[-1] == 1.0
    x = np.arange(5.0) ** 2
    np.testing.assert_array_equal(op(ift.makeField(op.domain, x)).asnumpy(), x)
    b, f = sc.regrid_tables(7, 4)
    assert np.all(np.diff(b) >= 0) and np.all(b <= 5)


def test_regridding_argument_errors():
    with pytest.raises(TypeError):
        ift.RegriddingOperator(ift.UnstructuredDomain(5), (3,))
    with pytest.raises(ValueError):
        ift.RegriddingOperator(ift.RGSpace((8, 8)), (4,))
    with pytest.raises(ValueError):
        ift.RegriddingOperator(ift.RGSpace(8), (9,))
    with pytest.raises(ValueError):
        ift.RegriddingOperator(ift.RGSpace(8), (0,))
    op = ift.RegriddingOperator(ift.RGSpace(8, 0.5), (4,))
    assert op.target[0].distances == (1.0,) and op.capability == op.TIMES | op.ADJOINT_TIMES


def test_compat_resolves_the_reference_module_paths():
    """in a child process: install() registers aliases in sys.modules"""
    code = ("import nifty_amd.compat as c; c.install(); "
            "from nifty.cl.operators.linear_interpolation import LinearInterpolator as A; "
            "from nifty.cl.operators.regridding_operator import RegriddingOperator as B; "
            "import nifty.cl as ift; assert A is ift.LinearInterpolator and B is ift.RegriddingOperator; print('ok')")
    import sys

    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr


# ---- the kernels' bodies on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = str(tmp_path_factory.mktemp("emu") / "libnk_emu_sample.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, os.path.join(ROOT, "tests", "emu", "emu_sample.cpp")])
    return ctypes.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_times(emu, plan, x):
    n = np.array(plan.shape, dtype=np.int64)
    x = np.ascontiguousarray(x)
    y = np.full(plan.npoints, np.nan, dtype=x.dtype)
    rc = emu.emu_sample_times(plan.ndim, _p(n), ctypes.c_int64(plan.npoints), _p(plan.cell), _p(plan.frac), _p(plan.perm), _p(x), _p(y),
                              int(x.dtype == np.float64))
    assert rc == 0
    return y


def emu_adjoint(emu, plan, y):
    n = np.array(plan.shape, dtype=np.int64)
    y = np.ascontiguousarray(y)
    out = np.full(plan.shape, np.nan, dtype=y.dtype)
    rc = emu.emu_sample_adjoint(plan.ndim, _p(n), ctypes.c_int64(plan.npoints), ctypes.c_int64(len(plan.cell_start) - 1), _p(plan.cell),
                                _p(plan.frac), _p(plan.perm), _p(plan.cell_start), ctypes.c_int64(len(plan.long_cell)),
                                _p(plan.long_cell), _p(y), _p(out), int(y.dtype == np.float64))
    assert rc == 0
    return out


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("name", list(sc.INTERP_CASES))
def test_emulated_interpolation_kernels(emu, name, single):
    op, shape, dist, points = interp_case(name)
    dt = np.float32 if single else np.float64
    x, y = Z[f"interp.{name}.x"].astype(dt), Z[f"interp.{name}.y"].astype(dt)
    ex = sc.interp_exact(shape, dist, points, x, y)
    bd = sc.interp_bounds(shape, ex, single)
    check(emu_times(emu, op.plan, x), ex["times"], bd["times"], "emulated TIMES")
    check(emu_adjoint(emu, op.plan, y), ex["adjoint"], bd["adjoint"], "emulated ADJOINT")


@pytest.mark.parametrize("single", [False, True])
def test_emulated_adjoint_of_a_long_cell(emu, single):
    """5000 points in one cell (one workgroup, the fixed tree) plus one elsewhere"""
    rng = np.random.default_rng(11)
    shape, dist = (6, 5), (0.5, 0.25)
    pts = np.concatenate([(np.array([[2.0], [3.0]]) + rng.random((2, 5000))) * np.array(dist)[:, None], [[0.1], [0.1]]], axis=1)
    plan = so.InterpolationPlan(shape, dist, pts)
    assert list(np.diff(plan.cell_start)) == [1, 5000] and list(plan.long_cell) == [1]
    dt = np.float32 if single else np.float64
    x, y = rng.standard_normal(shape).astype(dt), rng.standard_normal(5001).astype(dt)
    ex = sc.interp_exact(shape, dist, pts, x, y)
    assert ex["L"] == 5000
    bd = sc.interp_bounds(shape, ex, single)
    check(emu_times(emu, plan, x), ex["times"], bd["times"], "emulated TIMES")
    got = emu_adjoint(emu, plan, y)
    check(got, ex["adjoint"], bd["adjoint"], "emulated ADJOINT")
    check(plan.adjoint_host(y), ex["adjoint"], sc.interp_bounds(shape, ex)["adjoint"], "host ADJOINT")


@pytest.mark.parametrize("name", [n for n in sc.REGRID_CASES if n != "length_one"])
def test_emulated_regridding_kernels(emu, name):
    op = regrid_case(name)
    shape, axes, old, new, dists, tshape = sc.regrid_layout(sc.REGRID_CASES[name])
    for single in (False, True):
        dt = np.float32 if single else np.float64
        x, y = Z[f"regrid.{name}.x"].astype(dt), Z[f"regrid.{name}.y"].astype(dt)
        ex = sc.regrid_exact(shape, axes, old, new, dists, x, y)
        bd = sc.regrid_bounds(ex, single)
        for adj, v, key in ((0, x, "times"), (1, y, "adjoint")):
            shp = list(v.shape)
            todo = op._axes()
            for k, (d, t) in enumerate(todo):
                n_old, n_new = op.domain.shape[d], op.target.shape[d]
                odt = dt if k == len(todo) - 1 else np.float64
                outer, inner = int(np.prod(shp[:d])), int(np.prod(shp[d + 1:]))
                shp[d] = n_old if adj else n_new
                out = np.full(shp, np.nan, dtype=odt)
                v = np.ascontiguousarray(v)
                tab = op._rstart[t] if adj else op._bindex[t]
                emu.emu_regrid(adj, ctypes.c_int64(outer), ctypes.c_int64(n_old), ctypes.c_int64(n_new), ctypes.c_int64(inner), _p(tab),
                               _p(op._frac[t]), _p(v), int(v.dtype == np.float64), _p(out), int(odt == np.float64))
                v = out
            check(v, ex[key], bd[key], f"emulated regridding {key} ({dt.__name__})")
