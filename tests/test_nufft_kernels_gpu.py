"""The kernels of nk_nufft.hip through nk_nufft_spread / _interp / _crop / _pad directly, cell by cell and point by point
against the long-double references and derived bounds of tests/nufft_cases.py (factor 1), in fp64 and fp32: every cell of the
oversampled grid, every point, NaN pre-fills, guard bands around every buffer, equal bits from run to run, split against
unsplit lists, the transpose identities, no points at all, and the refusals of nu_validate.  Every comparison prints the case,
the type, the worst error / bound and where it occurred (profiles/nufft_kernel_errors.txt keeps those lines)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from nifty_amd import nufft

from tests import nufft_cases as nc

pytestmark = pytest.mark.gpu
LD = nc.LD
NAMES = list(nc.CASES)
GUARD = 64
FILL = 7.0
TYPES = pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])


def _guarded(n, dtype, inner=None):
    """n elements between two guard bands of FILL; the inside pre-filled with `inner` (NaN: every element has to be written)"""
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device="cuda:0")
    view = buf[GUARD:GUARD + n]
    if inner is not None:
        view.fill_(inner)
    return buf, view


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n:] == FILL).all())


def _real(a):
    """a complex numpy array as its interleaved reals"""
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype).reshape(-1)


def _upload(a):
    """a read-only input between guard bands; returns (buffer, view, the bits it has to keep)"""
    flat = np.array(_real(a) if np.iscomplexobj(a) else np.asarray(a).reshape(-1))
    buf, view = _guarded(flat.size, torch.from_numpy(flat).dtype)
    view.copy_(torch.from_numpy(flat))
    return buf, view, flat


def _unchanged(buf, view, flat):
    return _guards_intact(buf, flat.size) and np.array_equal(nc.bits(view.cpu().numpy()), nc.bits(flat))


@functools.lru_cache(maxsize=None)
def _plans(name, m=None, chunk=None):
    plan = nc.plan_of(name, m, chunk)
    return plan, plan.device_plan(torch.device("cuda:0"))


def _rdt(single):
    return torch.float32 if single else torch.float64


def _code(single):
    return L.NK_F32 if single else L.NK_F64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits_equal(a, b):
    return np.array_equal(nc.bits(a), nc.bits(b))


def run_spread(plan, dp, v, single):
    """nk_nufft_spread into a NaN grid; the grid, the values and the slab scratch between guard bands.  Returns [n..., 2]."""
    size = int(np.prod(plan.n))
    gbuf, grid = _guarded(2 * size, _rdt(single), float("nan"))
    vbuf, pts, vflat = _upload(v)
    nslab = 2 * nc.NU_CELLS * plan.n_slabs
    sbuf, slab = _guarded(nslab, torch.float64, float("nan"))
    L.check(L.load().nk_nufft_spread(ctypes.byref(dp.c), pts.data_ptr(), grid.data_ptr(), slab.data_ptr() if nslab else None,
                                     _code(single), _stream()), "nk_nufft_spread")
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, 2 * size) and _guards_intact(sbuf, nslab) and _unchanged(vbuf, pts, vflat)
    return grid.cpu().numpy().reshape(tuple(plan.n) + (2,))


def run_interp(plan, dp, g, single):
    """nk_nufft_interp of the grid g into NaN points between guard bands.  Returns [m, 2]."""
    gbuf, grid, gflat = _upload(g)
    pbuf, pts = _guarded(2 * plan.m, _rdt(single), float("nan"))
    L.check(L.load().nk_nufft_interp(ctypes.byref(dp.c), grid.data_ptr(), pts.data_ptr(), _code(single), _stream()), "nk_nufft_interp")
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, 2 * plan.m) and _unchanged(gbuf, grid, gflat)
    return pts.cpu().numpy().reshape(plan.m, 2)


def run_crop(plan, dp, g, single):
    gbuf, grid, gflat = _upload(g)
    total = int(np.prod(plan.nmodes))
    obuf, out = _guarded(total, _rdt(single), float("nan"))
    L.check(L.load().nk_nufft_crop(ctypes.byref(dp.c), grid.data_ptr(), out.data_ptr(), _code(single), _stream()), "nk_nufft_crop")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, total) and _unchanged(gbuf, grid, gflat)
    return out.cpu().numpy().reshape(plan.nmodes)


def run_pad(plan, dp, x, single):
    xbuf, xin, xflat = _upload(x)
    size = int(np.prod(plan.n))
    gbuf, grid = _guarded(2 * size, _rdt(single), float("nan"))
    L.check(L.load().nk_nufft_pad(ctypes.byref(dp.c), xin.data_ptr(), int(np.iscomplexobj(x)), grid.data_ptr(), _code(single),
                                  _stream()), "nk_nufft_pad")
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, 2 * size) and _unchanged(xbuf, xin, xflat)
    return grid.cpu().numpy().reshape(tuple(plan.n) + (2,))


def _tag(name, single, what):
    return f"{name} {'fp32' if single else 'fp64'} {what}"


@TYPES
@pytest.mark.parametrize("name", NAMES)
def test_spread_every_cell(name, single):
    plan, dp = _plans(name)
    v = nc.case_values(name, single)[0]
    ex = nc.spread_reference(name, single)
    grid = run_spread(plan, dp, v, single)
    assert grid.dtype == (np.float32 if single else np.float64) and not np.isnan(grid).any()  # every cell written
    nc.check(grid[..., 0], grid[..., 1], ex, _tag(name, single, "spread"))
    assert _bits_equal(grid, run_spread(plan, dp, v, single))
    if nc.CASES[name][2]:
        assert plan.n_slabs == nc.SLABS[name] and dp.c.n_split > 0
        whole_plan, whole_dp = _plans(name, None, 1 << 40)
        assert whole_plan.n_slabs == 0 and whole_dp.c.n_split == 0
        whole = run_spread(whole_plan, whole_dp, v, single)
        nc.check(whole[..., 0], whole[..., 1], ex, _tag(name, single, "spread unsplit"))
        two = {"re": grid[..., 0], "im": grid[..., 1], "bound_re": 2 * ex["bound_re"], "bound_im": 2 * ex["bound_im"]}
        nc.check(whole[..., 0], whole[..., 1], two, _tag(name, single, "spread unsplit vs split (two bounds)"))
    else:
        assert plan.n_slabs == 0


@TYPES
@pytest.mark.parametrize("m", [None, 1, 17], ids=["all", "m1", "m17"])
@pytest.mark.parametrize("name", NAMES)
def test_interp_every_point(name, m, single):
    plan, dp = _plans(name, m)
    g = nc.case_values(name, single)[1]
    ex = nc.interp_reference(name, single, m)
    pts = run_interp(plan, dp, g, single)
    assert plan.m == (m or plan.m) and not np.isnan(pts).any()
    nc.check(pts[:, 0], pts[:, 1], ex, _tag(name, single, f"interp m={plan.m}"))  # in the caller's order
    assert _bits_equal(pts, run_interp(plan, dp, g, single))


@TYPES
@pytest.mark.parametrize("name", NAMES)
def test_crop_and_pad_bits(name, single):
    plan, dp = _plans(name)
    v, g, x = nc.case_values(name, single)
    out = run_crop(plan, dp, g, single)
    want = nc.crop_bits(g, plan.corr_axes, plan.nmodes, plan.n)
    changed = int(np.count_nonzero(nc.bits(out) != nc.bits(want)))
    print(_tag(name, single, f"crop: {changed} of {want.size} entries differ in bits"))
    assert changed == 0
    band = np.zeros(plan.n, dtype=bool)
    band[nc._mode_cells(plan.nmodes, plan.n)] = True
    for xin, kind in ((x, "real"), ((x * (1 - 2j)).astype(v.dtype), "complex")):
        grid = run_pad(plan, dp, xin, single)
        want = nc.pad_bits(xin, plan.corr_axes, plan.nmodes, plan.n)
        assert not np.isnan(grid).any()  # every cell of the oversampled grid is written
        assert not nc.bits(grid)[~band].any()  # +0 in both parts outside the band
        changed = int(np.count_nonzero(nc.bits(grid) != nc.bits(want)))
        print(_tag(name, single, f"pad {kind}: {changed} of {want.size} entries differ in bits"))
        assert changed == 0
        if kind == "real":
            assert not nc.bits(grid[..., 1]).any()


def _cdot(ar, ai, br, bi):
    """sum a b of two complex arrays given by parts, in long double"""
    ar, ai, br, bi = (np.asarray(t).astype(LD).reshape(-1) for t in (ar, ai, br, bi))
    return (ar * br - ai * bi).sum(), (ar * bi + ai * br).sum()


@TYPES
@pytest.mark.parametrize("name", NAMES)
def test_transpose_identities(name, single):
    plan, dp = _plans(name)
    v, g, x = nc.case_values(name, single)
    sx, ix = nc.spread_reference(name, single), nc.interp_reference(name, single)
    grid, pts = run_spread(plan, dp, v, single), run_interp(plan, dp, g, single)
    # <g, spread(v)> = <interp(g), v> (bilinear): each side is off by at most its bounds contracted with |g|, |v|
    lr, li = _cdot(g.real, g.imag, grid[..., 0], grid[..., 1])
    rr, ri = _cdot(pts[:, 0], pts[:, 1], v.real, v.imag)
    tol = float((np.abs(g).astype(LD).reshape(-1) * (sx["bound_re"] + sx["bound_im"]).astype(LD).reshape(-1)).sum()
                + (np.abs(v).astype(LD) * (ix["bound_re"] + ix["bound_im"]).astype(LD)).sum())
    diff = float(np.hypot(lr - rr, li - ri))
    print(_tag(name, single, f"<g, spread v> - <interp g, v> = {diff:.3e}, allowed {tol:.3e} ({diff / tol:.3f})"))
    assert diff <= tol
    # <pad(x), G> = <x, crop(G)> on the real parts: the same correction product on both sides, then one product in double
    # (and one cast in fp32) per entry on either side
    pad, crop = run_pad(plan, dp, x, single), run_crop(plan, dp, g, single)
    lhs = (pad[..., 0].astype(LD) * g.real.astype(LD)).sum()
    rhs = (x.astype(LD) * crop.astype(LD)).sum()
    k = nc.U64 + (nc.U32 if single else 0.0)
    tol = float(k * (1 + 4 * k) * ((np.abs(pad[..., 0]).astype(LD) * np.abs(g.real).astype(LD)).sum() + (np.abs(x).astype(LD) * np.abs(crop).astype(LD)).sum()))
    diff = float(abs(lhs - rhs))
    print(_tag(name, single, f"<pad x, G> - <x, crop G> = {diff:.3e}, allowed {tol:.3e} ({diff / tol:.3f})"))
    assert diff <= tol


@TYPES
def test_no_points(single):
    plan = nufft.NufftPlan((13, 9), [1.0, 1.0], np.zeros((0, 2)), 1e-7)
    dp = plan.device_plan(torch.device("cuda:0"))
    assert plan.m == 0 and dp.c.m == 0 and plan.n == (27, 18)
    grid = run_spread(plan, dp, np.zeros(0, dtype=np.complex64 if single else np.complex128), single)
    assert not nc.bits(grid).any()  # every cell +0
    g = nc.case_values("ragged_2d", single)[1]
    assert run_interp(plan, dp, g, single).shape == (0, 2)  # NK_OK, guards and grid untouched
    assert L.load().nk_nufft_interp(ctypes.byref(dp.c), None, None, _code(single), None) == L.NK_OK  # nothing to touch


def _faulty(dp, **fields):
    bad = L.NufftPlan.from_buffer_copy(dp.c)
    for k, val in fields.items():
        if isinstance(val, tuple):
            getattr(bad, k)[val[0]] = val[1]
        else:
            setattr(bad, k, val)
    return bad


def test_refusals_before_any_launch():
    lib = L.load()
    plan, dp = _plans("ragged_2d")
    v, g, x = nc.case_values("ragged_2d", False)
    size, total = int(np.prod(plan.n)), int(np.prod(plan.nmodes))
    bufs = [_guarded(2 * size, torch.float64, 1.0), _guarded(2 * plan.m, torch.float64, 1.0), _guarded(total, torch.float64, 1.0)]
    grid, pts, modes = (b[1].data_ptr() for b in bufs)
    calls = {
        "spread": lambda c, code=L.NK_F64, gr=grid: lib.nk_nufft_spread(ctypes.byref(c), pts, gr, None, code, None),
        "interp": lambda c, code=L.NK_F64, gr=grid: lib.nk_nufft_interp(ctypes.byref(c), gr, pts, code, None),
        "crop": lambda c, code=L.NK_F64, gr=grid: lib.nk_nufft_crop(ctypes.byref(c), gr, modes, code, None),
        "pad": lambda c, code=L.NK_F64, gr=grid: lib.nk_nufft_pad(ctypes.byref(c), modes, 0, gr, code, None),
    }
    w = plan.w
    faults = [
        (dict(ndim=0), b"ndim must be 1, 2 or 3"), (dict(ndim=4), b"ndim must be 1, 2 or 3"),
        (dict(w=1), b"kernel width must be 2 .. 16"), (dict(w=17), b"kernel width must be 2 .. 16"),
        (dict(n=(0, 2 * w - 1)), b"oversampled length must be >= max(2 w, grid length)"),
        (dict(ntiles=(0, plan.ntiles[0] + 1)), b"tile geometry does not match"),
        (dict(ntiles=(0, plan.ntiles[0] - 1)), b"tile geometry does not match"),
        (dict(tile=(1, plan.tile[1] // 2), ntiles=(1, -(-plan.n[1] // (plan.tile[1] // 2)))), b"a tile must hold 256 cells"),
        (dict(corr=None), b"missing correction table"),
    ]
    for fields, message in faults:
        bad = _faulty(dp, **fields)
        for entry, call in calls.items():
            assert call(bad) == L.NK_ERR_INVALID, (fields, entry)
            assert message in lib.nk_last_error(), (fields, entry, lib.nk_last_error())
    for entry, call in calls.items():
        assert call(dp.c, 5) == L.NK_ERR_INVALID, entry
        assert b"dtype must be NK_F32 or NK_F64" in lib.nk_last_error(), entry
        assert call(dp.c, L.NK_F64, None) == L.NK_ERR_INVALID, entry
        assert b"nk_nufft_%s: bad argument" % entry.encode() in lib.nk_last_error(), entry
    split_plan, split_dp = _plans("split_2d")
    sgrid = torch.full((2 * int(np.prod(split_plan.n)),), 1.0, dtype=torch.float64, device="cuda:0")
    spts = torch.zeros(2 * split_plan.m, dtype=torch.float64, device="cuda:0")
    assert split_dp.c.n_split > 0
    assert lib.nk_nufft_spread(ctypes.byref(split_dp.c), spts.data_ptr(), sgrid.data_ptr(), None, L.NK_F64, None) == L.NK_ERR_INVALID
    assert b"split lists need the slab scratch" in lib.nk_last_error()
    torch.cuda.synchronize()
    # nothing ran: every buffer still holds its fill
    assert bool((sgrid == 1.0).all()) and all(bool((b[1] == 1.0).all()) and _guards_intact(b[0], b[1].numel()) for b in bufs)
