"""Host tests of tests/transform_cases.py -- the long-double reference, the derived bounds and the comparators that
tests/test_fused_transforms_gpu.py asserts on the device -- and of the host emulation's outputs under the same
comparators (tests/emu runs the kernels' phase functions thread by thread, on every route of the library)."""
import ctypes
import os

import numpy as np
import pytest

from nifty_amd._lib import Fuse
from tests import transform_cases as tc

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "libnk_emu.so")
ALL_SHAPES = [s for s, _, _ in tc.ROUTES]
DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("shape", [(2,), (30,), (64,), (4, 6), (6, 10), (2, 3, 4), (4, 2, 8)])
def test_long_double_reference_equals_a_direct_cas_sum(shape):
    x = np.random.default_rng(0).normal(size=shape)
    for sign in (1, -1):
        ref = tc.hartley_direct_mp(x, sign)
        got = tc.hartley_ld(x, len(shape), sign)
        # long double: eps 1.1e-19; a transform of <= 64 points stays far below 1e-17 max |ref|
        assert np.max(np.abs(got - ref)) < 1e-17 * np.max(np.abs(ref))


@pytest.mark.parametrize("shape", ALL_SHAPES + [s for s, _ in tc.SANDWICH[1:]])
def test_bounds_hold_for_scipy_in_the_same_precision(shape):
    """The derived 2-norm bound is not below what a sound transform in T does, and the long-double reference agrees with
    scipy.fft in fp64 to the fp64 bound."""
    x64 = np.random.default_rng(1).normal(size=shape)
    for dtype in DTYPES:
        x = x64.astype(dtype)
        ref = tc.hartley_ld(x, len(shape))
        got = tc.hartley_same_precision(x, len(shape))
        bound = tc.transform_rel_bound(shape, dtype, tc.route_of(shape, dtype) if shape in ALL_SHAPES else None) * tc.l2(ref)
        ok, e = tc.within_l2(got, ref, bound)
        assert ok, (dtype, e, bound)
        assert e > 0.0 or x.size <= 4  # ... and the comparison is not vacuous


@pytest.mark.parametrize("shape", [(30,), (10, 12), (64, 128), (6, 64, 96)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_impulse_reference_and_bound(shape, dtype):
    bound = tc.impulse_elem_bound(shape, dtype)
    for p in tc.impulse_positions(shape):
        x = np.zeros(shape, dtype=dtype)
        x[p] = 1.0
        for sign in (1, -1):
            ref = tc.impulse_reference(shape, p, sign)
            assert np.max(np.abs(tc.hartley_ld(x, len(shape), sign) - ref)) < 1e-17
            ok, worst = tc.within_elem(tc.hartley_same_precision(x, len(shape), sign), ref, bound)
            assert ok, (p, sign, worst)


def test_impulse_positions_cover_the_edges():
    pos = tc.impulse_positions((6, 64, 96))
    assert (0, 0, 0) in pos and (5, 0, 0) in pos and (0, 63, 0) in pos and (0, 0, 95) in pos
    assert (3, 0, 0) in pos and (0, 32, 0) in pos and (0, 0, 48) in pos
    assert any(p[-1] % 2 == 1 and p[0] for p in pos) and any(p[-1] % 2 == 0 and p[-1] and p[0] for p in pos)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(30,), (10, 12), (64, 128), (6, 64, 96)])
def test_comparators_reject_wrong_transforms(shape, dtype):
    x = np.random.default_rng(2).normal(size=shape).astype(dtype)
    nd = len(shape)
    ref = tc.hartley_ld(x, nd)
    bound = tc.transform_rel_bound(shape, dtype) * tc.l2(ref)
    good = tc.hartley_same_precision(x, nd)
    assert tc.within_l2(good, ref, bound)[0]
    flat = good.ravel().copy()
    order = np.argsort(np.abs(flat))
    # two swapped output elements (neighbours in magnitude around the median: the smallest change a swap can make there)
    i, j = order[flat.size // 2], order[flat.size // 2 + 1]
    sw = flat.copy()
    sw[i], sw[j] = flat[j], flat[i]
    assert flat[i] != flat[j] and not tc.within_l2(sw.reshape(shape), ref, bound)[0]
    # one element of median magnitude with its sign flipped
    sf = flat.copy()
    sf[i] = -sf[i]
    assert not tc.within_l2(sf.reshape(shape), ref, bound)[0]
    # the other Hartley convention
    assert not tc.within_l2(tc.hartley_same_precision(x, nd, -1), ref, bound)[0]
    # a NaN
    nn = flat.copy()
    nn[0] = np.nan
    assert not tc.within_l2(nn.reshape(shape), ref, bound)[0]
    # element-wise comparator (impulses): the same defects
    p = tc.impulse_positions(shape)[-1]
    xi = np.zeros(shape, dtype=dtype)
    xi[p] = 1.0
    iref, ib = tc.impulse_reference(shape, p), tc.impulse_elem_bound(shape, dtype)
    g = tc.hartley_same_precision(xi, nd).ravel()
    assert tc.within_elem(g.reshape(shape), iref, ib)[0]
    a, b = np.argmax(g), np.argmin(g)
    sw = g.copy()
    sw[a], sw[b] = g[b], g[a]
    assert not tc.within_elem(sw.reshape(shape), iref, ib)[0]
    sf = g.copy()
    sf[a] = -sf[a]
    assert not tc.within_elem(sf.reshape(shape), iref, ib)[0]
    assert not tc.within_elem(tc.hartley_same_precision(xi, nd, -1), iref, ib)[0]


def host_outputs(case, sign):
    """The outputs of a fused call computed in T by numpy on the host: a sound implementation of the call."""
    I, O, S, T = case.inputs, case.outputs, case.set, case.dtype
    pro = S["pro"]
    x = I["in"]
    if pro == 3:
        x = x * I["in2"]
    elif pro in (1, 2):
        a = I["amp"][case.pidx].astype(T)
        x = a * x
        if pro == 2:
            x = x + I["damp"][case.pidx].astype(T) * I["in2"]
    t = tc.hartley_same_precision(x.astype(T), len(case.shape), sign).astype(np.float64) * case.scale
    got = {k: v.copy() for k, v in O.items()}
    if case.epi == "affine":
        got["out"] = (t + case.offset).astype(T)
    elif case.epi.startswith("vjp"):
        amp_at = I["amp"][case.pidx]
        own = amp_at * t + (S.get("addend_scale", 0.0) * I["addend"].astype(np.float64) if "addend" in I else 0.0)
        out = own.astype(T)
        if S.get("accumulate"):
            out = O["out"] + out
        got["out"] = out
        xt = I["xi"].astype(np.float64) * t
        if "w8" in O:
            got["w8"] = tc.fold_to_octant(xt, case.shape)
        else:
            got["abar"] = O["abar"] + np.bincount(case.pidx.ravel(), weights=xt.ravel(), minlength=case.nb + 1)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(30,), (10, 12), (64, 64)])
def test_vjp_comparator_rejects_a_missing_mirror_image(shape, dtype):
    octant = shape == (64, 64)
    rel = tc.transform_rel_bound(shape, dtype)
    for epi in ("vjp_atomic", "vjp_w8" if octant else "vjp_atomic"):
        case = tc.FusedCase(shape, dtype, "plain", epi, octant, seed=3)
        ref = case.reference(1, rel)
        got = host_outputs(case, 1)
        got.pop("w8max", None)
        ref.pop("w8max", None)
        rows = tc.compare(case, ref, got)
        assert all(r[3] for r in rows), rows
        # drop ONE mirror image of one coefficient from its sum: the point (1, .., 1)'s partner under the flip of all axes
        o = tuple(n - 1 for n in shape)
        t = (case.scale * tc.hartley_ld(case.inputs["in"], len(shape))).astype(np.float64)
        miss = float(case.inputs["xi"][o]) * t[o]
        bad = {k: v.copy() for k, v in got.items()}
        if epi == "vjp_w8":
            bad["w8"][tuple([1] * len(shape))] -= miss
        else:
            bad["abar"][case.pidx[o]] -= miss
        rows = tc.compare(case, ref, bad)
        assert not all(r[3] for r in rows), (epi, rows)
        # ... and a touched extra bin / a touched abar beside w8
        bad = {k: v.copy() for k, v in got.items()}
        bad["abar"][-1] += 1e-9
        assert not all(r[3] for r in tc.compare(case, ref, bad))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pro", tc.PROLOGUES)
def test_prologue_bounds_hold_for_a_host_evaluation(pro, dtype):
    shape = (6, 10, 12)
    case = tc.FusedCase(shape, dtype, pro, "affine", False, seed=4)
    ref = case.reference(1, tc.transform_rel_bound(shape, dtype))
    rows = tc.compare(case, ref, host_outputs(case, 1))
    assert all(r[3] for r in rows), rows


# ---- the emulation's outputs under the same comparators --------------------------------------------------------------
needs_emu = pytest.mark.skipif(not os.path.exists(EMU), reason="emulation library not built (run __graft_entry__.build())")


def emu_fn(route):
    if route[0] == 2:
        return "emu3_hartley_fused"
    if route[0] == 0 and route[1] == 1:
        return "emu2_hartley_fused"
    return "emu_hartley_fused"  # generic kernels; follows the library's route on contiguous-first plans


def emu_call(f, shape, dtype, sign, batch=1, fn=None):
    lib = ctypes.CDLL(EMU)
    shp = (ctypes.c_int64 * len(shape))(*shape)
    dt = 0 if np.dtype(dtype) == np.float32 else 1
    info = (ctypes.c_int64 * 16)()
    assert lib.emu_plan_info(len(shape), shp, dt, ctypes.c_int64(batch), info) == 0
    route = tuple(info[11:15])
    rc = getattr(lib, fn or emu_fn(route))(len(shape), shp, dt, ctypes.c_int64(batch), ctypes.byref(f), 0 if sign == 1 else 1)
    assert rc == 0, rc
    return route


@needs_emu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_emulated_transform_meets_the_derived_bound(shape, dtype):
    route = tc.route_of(shape, dtype)
    x = np.random.default_rng(5).normal(size=(2,) + shape).astype(dtype)
    rel = tc.transform_rel_bound(shape, dtype, route)
    for sign in (1, -1):
        out = np.full_like(x, np.nan)
        f = Fuse()
        f.in_, f.out, f.scale = x.ctypes.data, out.ctypes.data, 0.75
        assert emu_call(f, shape, dtype, sign, batch=2) == route  # the emulation runs the route the table names
        ref = LD(0.75) * tc.hartley_ld(x, len(shape), sign)
        ok, e = tc.within_l2(out, ref, rel * tc.l2(ref) + tc.store_term(ref, dtype))
        assert ok, (sign, e, rel * tc.l2(ref))


@needs_emu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [s for s in ALL_SHAPES if np.prod(s) <= 1 << 19])
def test_emulated_impulses_meet_the_element_bound(shape, dtype):
    route = tc.route_of(shape, dtype)
    bound = tc.impulse_elem_bound(shape, dtype, route)
    for i, p in enumerate(tc.impulse_positions(shape)):
        sign = 1 if i % 2 == 0 else -1
        x = np.zeros((2,) + shape, dtype=dtype)
        x[(1,) + p] = 1.0  # the impulse sits in the second member of the batch
        out = np.full_like(x, np.nan)
        f = Fuse()
        f.in_, f.out, f.scale = x.ctypes.data, out.ctypes.data, 1.0
        emu_call(f, shape, dtype, sign, batch=2)
        assert not out[0].any()
        ok, worst = tc.within_elem(out[1], tc.impulse_reference(shape, p, sign), bound)
        assert ok, (p, sign, worst)


@needs_emu
@pytest.mark.parametrize("group", ["prologues", "epilogues", "vjp"])  # (one test per group: the largest grids stay at a few seconds)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", tc.CLASS_SHAPES)
def test_emulated_fused_classes_meet_their_bounds(shape, dtype, group):
    route = tc.route_of(shape, dtype)
    octant = route[0] == 2
    rel = tc.transform_rel_bound(shape, dtype, route)
    combos = {"prologues": [(p, "affine") for p in tc.PROLOGUES + (tc.PROLOGUES_OCTANT if octant else [])],
              "epilogues": [("plain", e) for e in tc.EPILOGUES],
              "vjp": [("plain", e) for e in tc.VJPS + (["vjp_w8"] if octant else ["vjp_wfull"])]}[group]
    for i, (pro, epi) in enumerate(combos):
        sign = 1 if i % 2 == 0 else -1
        case = tc.FusedCase(shape, dtype, pro, epi, octant, seed=6)
        bufs = {k: v.copy() for k, v in list(case.inputs.items()) + list(case.outputs.items())}
        f = case.fill(Fuse(), lambda k: bufs[k].ctypes.data)
        if epi == "vjp_w8":
            bufs.pop("w8max", None)  # the fixed-order maximum is taken by the device's fold kernels
            f.w8max = None
        emu_call(f, shape, dtype, sign)
        ref = case.reference(sign, rel)
        ref.pop("w8max", None)
        rows = tc.compare(case, ref, {k: bufs[k] for k in case.outputs if k in bufs})
        assert all(r[3] for r in rows), (pro, epi, rows)


def emu_sandwich(f, shape, dtype, scale_first, sign):
    fn = ctypes.CDLL(EMU).emu4_hartley_sandwich
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                   ctypes.c_double, ctypes.c_int, ctypes.c_int]
    shp = (ctypes.c_int64 * len(shape))(*shape)
    rc = fn(len(shape), shp, 0 if np.dtype(dtype) == np.float32 else 1, 1, ctypes.addressof(f), scale_first, 0 if sign == 1 else 1, 0)
    assert rc == 0, rc


@needs_emu
@pytest.mark.parametrize("shape,dtype", [((64, 128), np.float64), ((64, 128), np.float32), ((64, 64, 128), np.float64)])
def test_emulated_octant_sandwich_meets_its_bounds(shape, dtype):
    """The metric application through the emulated sandwich: the three octant AMP_JVP prologues (da field, da by
    pidx_octant, the CG direction update written back to `in`), octant VJP epilogue with w8 and the curvature sum."""
    sf = 0.5 / np.sqrt(float(np.prod(shape)))
    for i, (pro, field) in enumerate((("jvp_dafield_oct", False), ("jvp_pidxoct_oct", True), ("jvp_cg_oct", False))):
        rel = tc.transform_rel_bound(shape, dtype, (2, 1, 1 if len(shape) == 3 else -1, 1),
                                     tc.sandwich_composed_axis(shape, dtype, field))
        sign = 1 if i % 2 == 0 else -1
        case = tc.FusedCase(shape, dtype, pro, "vjp_w8", True, seed=7, sandwich=(sf, 0.7, field))
        case.outputs["value"] = np.array([0.25])
        case.outputs.pop("w8max", None)  # the fixed-order maximum is taken by the device's fold kernels
        bufs = {k: v.copy() for k, v in list(case.inputs.items()) + list(case.outputs.items())}
        f = case.fill(Fuse(), lambda k: bufs[k].ctypes.data)
        emu_sandwich(f, shape, dtype, sf, sign)
        ref = case.reference(sign, rel)
        ref.pop("w8max", None)
        rows = tc.compare(case, ref, {k: bufs[k] for k in case.outputs})
        assert all(r[3] for r in rows), (pro, rows)
        if pro == "jvp_cg_oct":  # the comparator sees a direction that was not updated
            bufs["in"] = case.outputs["in"].copy()
            assert not all(r[3] for r in tc.compare(case, ref, {k: bufs[k] for k in case.outputs}))


@needs_emu
@pytest.mark.parametrize("epi", ["lh_gauss_id", "lh_gaussf_exp", "lh_poisson_exp"])
def test_emulated_io32_forward_meets_its_bounds(epi):
    shape = (64, 128)
    case = tc.FusedCase(shape, np.float64, "amp_afield_oct", epi, True, seed=8, io32=True)
    bufs = {k: v.copy() for k, v in list(case.inputs.items()) + list(case.outputs.items())}
    f = case.fill(Fuse(), lambda k: bufs[k].ctypes.data)
    emu_call(f, shape, np.float64, 1)
    rows = tc.compare(case, case.reference(1, tc.transform_rel_bound(shape, np.float64, (2, 1, -1, 1))), {k: bufs[k] for k in case.outputs})
    assert bufs["out"].dtype == np.float32 and all(r[3] for r in rows), rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_comparator_rejects_a_dropped_wavefront_partial(dtype):
    """The energy sum is asserted at the depth of the device's slot-and-fold tree (tc.reduction_depth): a sum that misses
    the partial of one wavefront (64 of the 4096 terms) fails, a sum formed in fp64 in any order passes."""
    shape = (64, 64)
    case = tc.FusedCase(shape, dtype, "plain", "lh_gauss_id", True, seed=9)
    depth = tc.reduction_depth(1 << 20)
    assert depth < 200  # against the 4096 + 4 of one running sum
    ref = case.reference(1, tc.transform_rel_bound(shape, dtype), depth)
    value, _, bound = ref["value"]
    I = case.inputs
    r = (case.scale * tc.hartley_ld(I["in"], 2) + case.offset).astype(np.float64) - I["data"].astype(np.float64)
    e = 0.5 * case.set["icov_scalar"] * r * r
    good = case.outputs["value"] + np.sum(e[::-1])
    assert tc.within_elem(good, value, bound)[0]
    assert not tc.within_elem(good - np.sum(e[0]), value, bound)[0]
