"""Host tests of tests/transform_cases.py -- the long-double reference, the derived bounds and the comparators that
tests/test_fused_transforms_gpu.py asserts on the device -- and of the host emulation's outputs under the same
comparators (tests/emu runs the kernels' phase functions thread by thread, on every route of the library).  The second half
does the same for the complex side (tests/test_complex_transforms_gpu.py): the complex reference against a direct mpmath DFT,
the c2c and chirp-z bounds against scipy.fft and a numpy restatement of the chirp-z in the same precision on every shape and
length -- and on the very inputs -- of the device tests, the accuracy of the host-built filter tables, and the lengths of
the seam tests re-derived from the limits in the code."""
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


@pytest.mark.parametrize("shape", [s for s in ALL_SHAPES if np.prod(s) <= 64 * 128] + [(7, 9), (5, 6, 7)])
def test_bin_index_from_integer_k2_equals_the_power_space(shape):
    """real_pindex ranks the integer k^2 (pindex_from_k2) instead of building a PowerSpace: the same index and bin count
    on every shape of the route table up to (64, 128) and on two grids with odd axes (no Nyquist plane on those axes)."""
    want, nb_want = tc.pindex_powerspace(shape)
    got, nb = tc.pindex_from_k2(shape)
    assert nb == nb_want and got.dtype == want.dtype == np.int32 and got.shape == want.shape == tuple(shape)
    assert np.array_equal(got, want)
    if all(n % 2 == 0 for n in shape):  # real_pindex asserts a Nyquist-only bin
        cached, nb_cached = tc.real_pindex(shape)
        assert nb_cached == nb and np.array_equal(cached, want) and not cached.flags.writeable


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


# ---- complex transforms: the reference, and the bounds against sound implementations in T -------------------------------
@pytest.mark.parametrize("shape", [(2,), (30,), (64,), (4, 6), (6, 10), (2, 3, 4), (4, 2, 8)])
def test_complex_long_double_reference_equals_a_direct_dft(shape):
    x = tc.normal_complex(shape, np.float64, 0)
    for inverse in (False, True):
        ref = tc.fft_direct_mp(x, inverse)
        got = tc.fft_ld(x, len(shape), inverse)
        assert np.max(np.abs(got - ref)) < 1e-17 * np.max(np.abs(ref))
        assert tc.err_l2c(np.conj(tc.fft_ld(np.conj(x), len(shape), not inverse)), ref) < 1e-17 * tc.l2c(ref)


def test_c2c_set_up_restated():
    """The figures the device tests assert: the strided passes that need more than 64 KiB, the longest lines."""
    for dt, (shape, lds) in tc.C2C_BIG_LDS.items():
        for batch in (1, 3):
            assert tc.c2c_lds_bytes(shape, dt, batch)[2] == lds > 64 * 1024
    (a, la), (b, lb) = tc.C2C_TWO_PLANS
    assert tc.c2c_lds_bytes(a, np.float64)[2] == la > lb == tc.c2c_lds_bytes(b, np.float64)[2] > 64 * 1024
    assert tc.c2c_lds_bytes((1000, 8), np.float64)[2] == 64000  # the listed shape stays just below
    assert tc.c2c_longest(np.float64) == 8640 and tc.c2c_longest(np.float32) == 17280
    for dt in DTYPES:
        nl = tc.c2c_longest(dt)
        assert nl + nl // 16 + 1 <= tc.c2c_line_limit(dt) and tc.c2c_lds_bytes((nl,), dt, 3)[0] > 64 * 1024


@pytest.mark.parametrize("dtype", DTYPES)
def test_c2c_bound_holds_for_scipy_in_the_same_precision(dtype):
    """every shape of the device test, its seeded batch of three, forward and inverse"""
    u = tc.unit_roundoff(dtype)
    for shape in tc.c2c_shapes(dtype):
        x = tc.normal_complex((3,) + shape, dtype, 51)
        rel = tc.c2c_rel_bound(shape, dtype)
        for inverse in (False, True):
            ref = tc.fft_ld(x, len(shape), inverse)
            ok, e = tc.within_l2c(tc.fft_same_precision(x, len(shape), inverse), ref, rel * tc.l2c(ref))
            print(f"ERR kind=c2c shape={'x'.join(map(str, shape))} dtype={np.dtype(dtype).name} mode=host/inv{int(inverse)} "
                  f"err={e / tc.l2c(ref):.3e} bound={rel:.3e} err_u={e / tc.l2c(ref) / u:.2f}")
            assert ok and e > 0.0, (shape, inverse, e, rel * tc.l2c(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(30,), (4096,), (15, 14), (9, 25, 28)])
def test_c2c_impulse_reference_and_bound(shape, dtype):
    bound = tc.c2c_impulse_elem_bound(shape, dtype)
    for p in tc.impulse_positions(shape):
        x = np.zeros(shape, dtype=tc.complex_dtype(dtype))
        x[p] = 1.0
        for inverse in (False, True):
            ref = tc.impulse_reference_c2c(shape, p, inverse)
            assert np.max(np.abs(tc.fft_ld(x, len(shape), inverse) - ref)) < 1e-17
            ok, worst = tc.within_elem_c(tc.fft_same_precision(x, len(shape), inverse), ref, bound)
            assert ok, (p, inverse, worst)
            if np.max(np.abs(ref.imag)) > 0.5:  # the other direction must not pass
                assert not tc.within_elem_c(tc.fft_same_precision(x, len(shape), not inverse), ref, bound)[0]


def chirp_lengths(dtype):
    """(n, m, kind) of every chirp-z length the device tests run in `dtype`"""
    out = [(n, m, "bluestein") for n, m, only in tc.BLUESTEIN_LENGTHS if only is None or np.dtype(only) == np.dtype(dtype)]
    out.append(tc.BLUESTEIN_GRID_STRIDE[:2] + ("bluestein",))
    csize = 8 if np.dtype(dtype) == np.float32 else 16
    seam = sorted({n for s in tc.SEAM_SHAPES for n in s if n % 2 or any(n % p == 0 for p in (11, 13, 17))})
    for n in seam:
        out += [(n, tc.smallest_m(n), "bluestein"), (n, tc.smallest_m(n), "composition")]
    for n, kind in tc.SEAM_LENGTHS[np.dtype(dtype)]:
        assert (tc.smallest_m(n) * csize <= 64 * 1024) == (kind == "one-launch")
        out.append((n, tc.smallest_m(n), "bluestein" if kind == "one-launch" else "composition"))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_chirp_z_bounds_hold_for_the_restatement_in_the_same_precision(dtype):
    """Every length of the device tests on their seeded rows: numpy's chirp-z with every intermediate in T stays inside
    bluestein_rel_bound (tables of backend._bluestein_tables) and composition_rel_bound (filter spectrum transformed in T)."""
    import torch

    from nifty_amd import backend as B

    u = tc.unit_roundoff(dtype)
    cdt = torch.complex64 if np.dtype(dtype) == np.float32 else torch.complex128
    for n, m, kind in chirp_lengths(dtype):
        rows = 3 if n * m < 1 << 20 else 2
        x = tc.normal_complex((rows, n), dtype, 52)
        for inverse in (False, True):
            wl, bl, bmax = tc.bluestein_filter_ld(n, m, inverse)
            if kind == "bluestein":
                w, bbr, _ = (t.numpy() for t in B._bluestein_tables(n, m, cdt, inverse, torch.device("cpu")))
                bhat = bbr[tc.bit_reverse(m)]
                w2, b2 = tc.bluestein_host_tables(n, m, dtype, inverse)
                assert np.array_equal(w, w2) and np.array_equal(bhat, b2)
            else:
                w, _ = tc.bluestein_host_tables(n, m, dtype, inverse)
                b = np.zeros(m, dtype=w.dtype)
                b[:n] = w.conj()
                b[m - n + 1:] = w.conj()[1:][::-1]
                bhat = scipy_fft_in(b)
            terr = tc.bluestein_table_error(bhat, n, m, inverse)
            assert np.max(np.abs(w.astype(tc.CLD) - wl)) <= (tc.MU_W64 * tc.U64 + (u if np.dtype(dtype) == np.float32 else 0.0))
            fn = tc.bluestein_rel_bound if kind == "bluestein" else tc.composition_rel_bound
            for hartley in (0, 1, -1):
                scale = 0.75 if hartley else 1.0
                xin = np.ascontiguousarray(x.real) if hartley == -1 else x  # real rows with one of the Hartley ends
                ref = tc.LD(scale) * tc.fft_ld(xin, 1, inverse)
                if hartley:
                    ref = ref.real + hartley * ref.imag
                got = tc.bluestein_same_precision(xin, n, m, w, bhat, scale, hartley)
                bound = fn(n, m, dtype, hartley=bool(hartley), inverse=inverse, table_err=terr)
                e = float(np.max(tc.row_errors(got, ref, xin, n, scale)))
                print(f"ERR kind={kind} n={n} m={m} dtype={np.dtype(dtype).name} mode=host/inv{int(inverse)}/h{hartley} err={e:.3e} "
                      f"bound={bound:.3e} err_u={e / u:.2f} table_err_u={terr / u:.2f} bmax={bmax / np.sqrt(n):.3f}")
                assert e <= bound and (e > 0.0 or n <= 2), (n, m, kind, inverse, hartley, e, bound)


def scipy_fft_in(b):
    import scipy.fft

    out = scipy.fft.fft(b)
    assert out.dtype == b.dtype
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_filter_tables_are_as_accurate_as_the_bound_assumes(dtype):
    """table_err of backend._bluestein_tables: rounded once in fp32 (the double transform behind it is far below u), and
    inside the norm-wise bound of a double transform of L levels on the perturbed filter in fp64."""
    u = tc.unit_roundoff(dtype)
    for n, m, only in tc.BLUESTEIN_LENGTHS:
        if only is not None and np.dtype(only) != np.dtype(dtype):
            continue
        for inverse in (False, True):
            _, bhat = tc.bluestein_host_tables(n, m, dtype, inverse)
            terr = tc.bluestein_table_error(bhat, n, m, inverse)
            bmax = tc.bluestein_filter_ld(n, m, inverse)[2]
            assert terr <= tc.host_table_error_ceiling(n, m, dtype, inverse), (n, m, terr / u)
            assert 1.0 <= bmax / np.sqrt(n) <= 2.5 or n <= 2, (n, m, bmax)


def test_chirp_z_comparator_rejects_wrong_rows():
    """a swapped pair of outputs, the other direction, a dropped final chirp and a wrong filter entry all leave the bound"""
    n, m, dtype = 211, 512, np.float32
    x = tc.normal_complex((3, n), dtype, 52)
    w, bhat = tc.bluestein_host_tables(n, m, dtype)
    ref = tc.fft_ld(x, 1)
    bound = tc.bluestein_rel_bound(n, m, dtype)
    good = tc.bluestein_same_precision(x, n, m, w, bhat)
    assert np.max(tc.row_errors(good, ref, x, n)) <= bound
    sw = good.copy()
    sw[1, 5], sw[1, 6] = good[1, 6], good[1, 5]
    assert np.max(tc.row_errors(sw, ref, x, n)) > bound
    assert np.max(tc.row_errors(np.conj(good), ref, x, n)) > bound
    bad = bhat.copy()
    bad[7] *= np.complex64(1.0 + 1e-3)  # one filter entry wrong in the fourth digit
    assert np.max(tc.row_errors(tc.bluestein_same_precision(x, n, m, w, bad), ref, x, n)) > bound
    nn = good.copy()
    nn[2, 0] = np.nan
    assert not np.max(tc.row_errors(nn, ref, x, n)) <= bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_lengths_follow_from_the_limits_in_the_code(dtype):
    """tc.SEAM_LENGTHS from the rules: the one-launch kernel takes rows of m complex values in 64 KiB, the composition a
    padded length that nk_fftn takes (one line of m + m / 16 + 1 complex values in 144 KiB) up to the seam's own cap."""
    from nifty_amd import backend as B

    csize = 8 if np.dtype(dtype) == np.float32 else 16
    m_one = B.BLUESTEIN_LDS_BYTES // csize
    m_comp = max(m for m in (1 << k for k in range(2, 20)) if m + m // 16 + 1 <= tc.c2c_line_limit(dtype) and m <= B._CHIRP_MAX)
    assert (m_one, m_comp) == ((4096, 8192) if csize == 16 else (8192, 16384))
    (a, pa), (b, pb), (c, pc) = tc.SEAM_LENGTHS[np.dtype(dtype)]
    # m = 2 n would serve the power of two n itself, which the planner takes: the longest REJECTED length is one below
    assert (a, pa) == (m_one // 2 - 1, "one-launch") and tc.smallest_m(a) == m_one
    assert (b, pb) == (m_one // 2 + 1, "composition") and tc.smallest_m(b) == 2 * m_one
    assert (c, pc) == (m_comp // 2 - 1, "composition") and tc.smallest_m(c) == m_comp and tc.smallest_m(m_comp // 2 + 1) == 2 * m_comp
    for n in (a, b, c, m_comp // 2 + 1):  # none of them is a length of the native planner
        assert n % 2 == 1
