"""LinearInterpolator and RegriddingOperator on device fields (nk_sample.hip): within the derived bounds of
tests/sampling_cases.py of the exact longdouble sums, against the host path, exact transposes, bit-reproducible, in fp64 and
fp32 -- on the host cases and on the smallest shapes at which the device path can still go wrong (several workgroups of
points and cells, long clustered lists, wrapping corners, coinciding corners, a single point) -- and one small inference."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nifty_amd as ift
from nifty_amd import _lib as L

from tests import sampling_cases as sc
from tests.goldenlib import load

pytestmark = pytest.mark.gpu
check = sc.check


def _clustered(shape, dist, cell, rng, n=5000, extra=True):
    """n points inside grid cell `cell`, plus (extra) one point elsewhere"""
    pts = (np.array(cell, dtype=np.float64)[:, None] + rng.random((len(shape), n))) * np.array(dist)[:, None]
    if extra:
        pts = np.concatenate([pts, (np.full((len(shape), 1), 0.25)) * np.array(dist)[:, None]], axis=1)
    return pts


def _device_interp_cases():
    cases = {}
    z = load("sampling_ops")
    for name, spaces in sc.INTERP_CASES.items():
        cases["host_" + name] = (spaces, z[f"interp.{name}.points"])
    rng = np.random.default_rng(300)

    def drawn(spaces, n):
        shape, dist = sc.grid_of(spaces)
        return spaces, sc.interp_points(shape, dist, rng, n)

    # more than one workgroup of points and of occupied cells
    cases["blocks_3d"] = drawn([((33, 20, 18), (0.2, 1.12, 0.7))], 10000)
    cases["blocks_2d"] = drawn([((257, 130), None)], 10000)
    # long lists: 5000 points in one cell plus one elsewhere; 5000 points in the last cell of every axis (every corner wraps)
    for name, shape, dist, cell, extra in (("cluster_2d", (6, 5), (0.5, 0.25), (2, 3), True), ("cluster_3d", (4, 5, 3), (0.5, 0.25, 1.0), (1, 2, 1), True),
                                           ("cluster_last_1d", (9,), (0.3,), (8,), False), ("cluster_last_2d", (6, 5), (0.5, 0.25), (5, 4), False),
                                           ("cluster_last_3d", (4, 5, 3), (0.5, 0.25, 1.0), (3, 4, 2), False)):
        cases[name] = ([(shape, dist)], _clustered(shape, dist, cell, rng, extra=extra))
    cases["one_point"] = ([((5, 7), (0.2, 1.12))], np.array([[0.93], [-3.1]]))
    # corners that coincide: axes of length 1 and 2
    cases["len1"] = drawn([((1,), None)], 40)
    cases["len2"] = drawn([((2,), None)], 40)
    cases["len21"] = drawn([((2, 1), None)], 40)
    cases["len121"] = drawn([((1, 2, 1), None)], 40)
    return cases


INTERP = _device_interp_cases()
REGRID = dict(sc.REGRID_CASES)
REGRID["blocks_2d"] = ([("rg", (130, 67))], (64, 67), 0)
REGRID["blocks_middle"] = ([("u", 9), ("rg", (40,)), ("u", 12)], (17,), 1)


@functools.lru_cache(maxsize=None)
def interp_setup(name, single):
    """operator, inputs, exact sums and bounds of one case: made once, shared by the tests, never modified"""
    spaces, points = INTERP[name]
    shape, dist = sc.grid_of(spaces)
    op = ift.LinearInterpolator(tuple(ift.RGSpace(shp, dst) for shp, dst in spaces), points)
    rng = np.random.default_rng(17)
    dt = np.float32 if single else np.float64
    x, y = rng.standard_normal(shape).astype(dt), rng.standard_normal(points.shape[1]).astype(dt)
    ex = sc.interp_exact(shape, dist, points, x, y)
    for a in (x, y, *[v for v in ex.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return op, x, y, ex, sc.interp_bounds(shape, ex, single)


@functools.lru_cache(maxsize=None)
def regrid_setup(name, single):
    desc, new_shape, space = REGRID[name]
    dom = tuple(ift.RGSpace(v) if kind == "rg" else ift.UnstructuredDomain(v) for kind, v in desc)
    op = ift.RegriddingOperator(dom, new_shape, space)
    shape, axes, old, new, dists, tshape = sc.regrid_layout(REGRID[name])
    rng = np.random.default_rng(19)
    dt = np.float32 if single else np.float64
    x, y = rng.standard_normal(shape).astype(dt), rng.standard_normal(tshape).astype(dt)
    ex = sc.regrid_exact(shape, axes, old, new, dists, x, y)
    for a in (x, y):
        a.setflags(write=False)
    return op, x, y, ex, sc.regrid_bounds(ex, single)


def _device_checks(op, x, y, ex, bd, single):
    xf, yf = ift.makeField(op.domain, x), ift.makeField(op.target, y)
    xd, yd = xf.at(0), yf.at(0)
    t1, t2, a1, a2 = op(xd), op(xd), op.adjoint(yd), op.adjoint(yd)
    tdt = torch.float32 if single else torch.float64
    assert t1.device_id == 0 and a1.device_id == 0 and t1.val.dtype == tdt and a1.val.dtype == tdt
    assert t1.val.shape == tuple(op.target.shape) and a1.val.shape == tuple(op.domain.shape)
    # the same bits from run to run, both modes
    assert torch.equal(t1.val, t2.val) and torch.equal(a1.val, a2.val)
    dt, da = t1.asnumpy(), a1.asnumpy()
    check(dt, ex["times"], bd["times"], "device TIMES vs exact")
    check(da, ex["adjoint"], bd["adjoint"], "device ADJOINT vs exact")
    check(dt, op(xf).asnumpy(), bd["times"], "device TIMES vs host", 2.0)  # two rounded sides
    check(da, op.adjoint(yf).asnumpy(), bd["adjoint"], "device ADJOINT vs host", 2.0)
    # exact transposes on the device: <y, A x> = <A^T y, x> to 1e-12 |x| |y| (products and sums in fp64 here).  fp32 outputs
    # carry their one final rounding, relative u32 per entry, so each side may move by u32 sum |y_i| |(A x)_i| at most
    x64, y64, t64, a64 = (v.astype(np.float64) for v in (x, y, dt, da))
    lhs, rhs = float(np.vdot(y64, t64)), float(np.vdot(a64, x64))
    tol = 1e-12 * np.linalg.norm(x64) * np.linalg.norm(y64)
    if single:
        tol += sc.U32 * (float(np.abs(y64).ravel() @ np.abs(t64).ravel()) + float(np.abs(a64).ravel() @ np.abs(x64).ravel()))
    print(f"<y, A x> - <A^T y, x> = {abs(lhs - rhs):.3e}, allowed {tol:.3e}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(INTERP))
def test_interpolator_on_the_device(name, single):
    op, x, y, ex, bd = interp_setup(name, single)
    if name.startswith("cluster"):
        assert len(op.plan.long_cell) == 1 and ex["L"] >= 5000
    if name.startswith("blocks"):
        assert len(op.plan.cell_start) - 1 > 2 * 256  # several workgroups of occupied cells
    _device_checks(op, x, y, ex, bd, single)


@pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(REGRID))
def test_regridding_on_the_device(name, single):
    op, x, y, ex, bd = regrid_setup(name, single)
    _device_checks(op, x, y, ex, bd, single)


def test_complex_fields_on_the_device():
    op, x, y, ex, bd = interp_setup("host_2d", False)
    xc, yc = x + 1j * x[::-1], y * (1 - 2j)
    t = op(ift.makeField(op.domain, xc).at(0))
    a = op.adjoint(ift.makeField(op.target, yc).at(0))
    assert t.val.dtype == torch.complex128 and a.val.dtype == torch.complex128 and t.device_id == 0
    np.testing.assert_array_equal(t.asnumpy().real, op(ift.makeField(op.domain, x).at(0)).asnumpy())
    np.testing.assert_array_equal(a.asnumpy().imag, -2 * op.adjoint(ift.makeField(op.target, y).at(0)).asnumpy())
    rop, rx, ry, rex, rbd = regrid_setup("middle", False)
    rt = rop(ift.makeField(rop.domain, rx * (1 + 1j)).at(0)).asnumpy()
    np.testing.assert_array_equal(rt.real, rop(ift.makeField(rop.domain, rx).at(0)).asnumpy())
    np.testing.assert_array_equal(rt.imag, rt.real)
    ra = rop.adjoint(ift.makeField(rop.target, (ry * (1 + 1j)).astype(np.complex64)).at(0))
    assert ra.val.dtype == torch.complex64
    np.testing.assert_array_equal(ra.asnumpy().real, rop.adjoint(ift.makeField(rop.target, ry.astype(np.float32)).at(0)).asnumpy())


GUARD = 64


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["host_3d", "blocks_2d", "cluster_last_3d", "len121"])
def test_interpolation_abi_writes_inside_its_outputs(name, single):
    op, x, y, ex, bd = interp_setup(name, single)
    dp = op.plan.device_plan(torch.device("cuda:0"))
    tdt = torch.float32 if single else torch.float64
    code = L.NK_F32 if single else L.NK_F64
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    xd, yd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    npts, size = y.size, x.size
    pbuf, pts = _guarded(npts, tdt, 7.0)
    L.check(lib.nk_sample_times(ctypes.byref(dp.c), xd.data_ptr(), pts.data_ptr(), code, st))
    gbuf, grid = _guarded(size, tdt, 7.0)
    abuf, acc = _guarded(size, torch.float64, 7.0)
    L.check(lib.nk_sample_adjoint(ctypes.byref(dp.c), yd.data_ptr(), grid.data_ptr(), acc.data_ptr(), code, st))
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, npts, 7.0) and _guards_intact(gbuf, size, 7.0) and _guards_intact(abuf, size, 7.0)
    assert torch.equal(pts, op(ift.makeField(op.domain, x).at(0)).val)
    assert torch.equal(grid.reshape(x.shape), op.adjoint(ift.makeField(op.target, y).at(0)).val)


@pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])
def test_regridding_abi_writes_inside_its_outputs(single):
    op, x, y, ex, bd = regrid_setup("blocks_middle", single)
    bindex, frac, rstart = op._tables(torch.device("cuda:0"))
    tdt = torch.float32 if single else torch.float64
    code = L.NK_F32 if single else L.NK_F64
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    xd, yd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    tbuf, t = _guarded(y.size, tdt, 7.0)
    L.check(lib.nk_regrid_times(9, 40, 17, 12, bindex[0].data_ptr(), frac[0].data_ptr(), xd.data_ptr(), code, t.data_ptr(), code, st))
    abuf, a = _guarded(x.size, tdt, 7.0)
    L.check(lib.nk_regrid_adjoint(9, 40, 17, 12, rstart[0].data_ptr(), frac[0].data_ptr(), yd.data_ptr(), code, a.data_ptr(), code, st))
    torch.cuda.synchronize()
    assert _guards_intact(tbuf, y.size, 7.0) and _guards_intact(abuf, x.size, 7.0)
    assert torch.equal(t.reshape(y.shape), op(ift.makeField(op.domain, x).at(0)).val)
    assert torch.equal(a.reshape(x.shape), op.adjoint(ift.makeField(op.target, y).at(0)).val)


def test_abi_validates_before_launching():
    lib = L.load()
    op, x, y, ex, bd = interp_setup("host_2d", False)
    dp = op.plan.device_plan(torch.device("cuda:0"))
    xd = torch.from_numpy(x.copy()).cuda()
    assert lib.nk_sample_times(ctypes.byref(dp.c), xd.data_ptr(), None, L.NK_F64, None) == L.NK_ERR_INVALID
    assert lib.nk_sample_times(ctypes.byref(dp.c), xd.data_ptr(), xd.data_ptr(), 5, None) == L.NK_ERR_INVALID
    bad = L.SamplePlan.from_buffer_copy(dp.c)
    bad.ndim = 4
    assert lib.nk_sample_times(ctypes.byref(bad), xd.data_ptr(), xd.data_ptr(), L.NK_F64, None) == L.NK_ERR_UNSUPPORTED
    yd = torch.from_numpy(y.astype(np.float32)).cuda()
    g = torch.empty(x.shape, dtype=torch.float32, device="cuda:0")
    assert lib.nk_sample_adjoint(ctypes.byref(dp.c), yd.data_ptr(), g.data_ptr(), None, L.NK_F32, None) == L.NK_ERR_INVALID
    assert b"scratch" in lib.nk_last_error()
    assert lib.nk_regrid_times(1, 1, 1, 1, xd.data_ptr(), xd.data_ptr(), xd.data_ptr(), L.NK_F64, xd.data_ptr(), L.NK_F64, None) == L.NK_ERR_INVALID
    assert lib.nk_regrid_adjoint(1, 4, 5, 1, xd.data_ptr(), xd.data_ptr(), xd.data_ptr(), L.NK_F64, xd.data_ptr(), L.NK_F64, None) == L.NK_ERR_INVALID


def test_four_grid_axes_are_refused_on_the_device_and_served_on_the_host():
    sp = ift.RGSpace((3, 4, 2, 5))
    rng = np.random.default_rng(3)
    op = ift.LinearInterpolator(sp, rng.random((4, 50)))
    x = ift.makeField(sp, rng.standard_normal(sp.shape))
    assert op(x).asnumpy().shape == (50,)
    for mode_in, run in ((x.at(0), op), (op(x).at(0), op.adjoint)):
        with pytest.raises(NotImplementedError, match="4"):
            run(mode_in)


def _lognormal_field(sp):
    """exp(HT(A xi)) with a fixed power spectrum: every device sum of its Jacobian and adjoint is fixed-order"""
    h = sp.get_default_codomain()
    ht = ift.HarmonicTransformOperator(h, sp)
    k = h.get_k_length_array().asnumpy()
    amp = 1.0 / (1.0 + (k / 8.0) ** 2)
    xi = np.random.default_rng(8).standard_normal(h.shape)
    scale = 1.0 / np.std(ht(ift.makeField(h, amp * xi)).asnumpy())
    return (ht @ ift.makeOp(ift.makeField(h, scale * amp)) @ ift.FieldAdapter(h, "xi")).exp()


def _okl(lh, dev):
    ift.random.push_sseq_from_seed(71)
    try:
        ic_s = ift.AbsDeltaEnergyController(deltaE=0.0, iteration_limit=10)
        mk = lambda i: ift.NewtonCG(ift.AbsDeltaEnergyController(0.0, iteration_limit=2), max_cg_iterations=8)  # noqa: E731
        return ift.optimize_kl(lh, 1, 1, mk, ic_s, output_directory=None, return_final_position=True, device_id=dev, fuse=False)
    finally:
        ift.random.pop_sseq()


def test_interpolated_field_optimize_kl_on_the_device():
    """One optimize_kl iteration (2 mirrored samples) of a log-normal field with a fixed spectrum on (64, 64) seen at 500
    points through LinearInterpolator with a Gaussian likelihood: the run stays on cuda:0, two device runs give the same
    bits, and the KL matches the host run to 1e-6."""
    rng = np.random.default_rng(61)
    sp = ift.RGSpace((64, 64))
    signal = _lognormal_field(sp)
    r = ift.LinearInterpolator(sp, rng.random((2, 500)) * 3.0 - 1.0)
    ift.random.push_sseq_from_seed(62)
    try:
        truth = ift.from_random(signal.domain)
    finally:
        ift.random.pop_sseq()
    clean = r(signal(truth)).asnumpy()
    noise = 0.3 * np.sqrt(np.mean(clean ** 2))
    data = clean + noise * rng.standard_normal(500)
    runs, kl_vals = [], {}
    for dev in (-1, 0, 0):
        d = ift.makeField(r.target, data)
        d = d if dev < 0 else d.at(dev)
        icov = ift.ScalingOperator(r.target, 1.0 / noise ** 2, sampling_dtype=np.float64)
        lh = ift.GaussianEnergy(data=d, inverse_covariance=icov) @ (r @ signal)
        sl, mean = _okl(lh, dev)
        samples = list(sl.iterator())
        assert len(samples) == 2
        if dev >= 0:
            assert mean.device_id == dev and all(s.device_id == dev for s in samples)
            runs.append([mean.val["xi"]] + [s.val["xi"] for s in samples])
        ham = ift.StandardHamiltonian(lh)
        kl_vals.setdefault(dev, []).append(sum(float(np.real(ham(s).asnumpy())) for s in samples) / len(samples))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert kl_vals[0][0] == kl_vals[0][1]
    assert abs(kl_vals[0][0] - kl_vals[-1][0]) <= 1e-6 * abs(kl_vals[-1][0])
