"""Keeps tests/nufft_cases.py honest without a GPU: the geometry every case stands for, the host kernels and the numpy
restatement of the device arithmetic (float32 and float64, 1 - x x contracted or not, tile lists and chunked slabs) inside the
derived bounds at factor 1 on every case, crop_bits / pad_bits against the long-double product, and deliberate faults written
into copies of the restatement -- each caught by an exceeded bound or by changed bits on a named case (`FAULT name caught=
ratio=` lines, as tests/test_binmap_cases.py prints them)."""
import numpy as np
import pytest

from nifty_amd import nufft

from tests import nufft_cases as nc
from tests.test_nufft import spread_like_the_device

LD = nc.LD
NAMES = list(nc.CASES)
TYPES = {"fp64": np.float64, "fp32": np.float32}


def _parts(a):
    """[..., 2] or complex -> (re, im)"""
    a = np.asarray(a)
    return (a.real, a.imag) if np.iscomplexobj(a) else (a[..., 0], a[..., 1])


@pytest.mark.parametrize("name", NAMES)
def test_geometry_is_what_the_case_stands_for(name):
    plan = nc.plan_of(name)
    nmodes, eps, split, _ = nc.CASES[name]
    assert (plan.w, plan.n, plan.ntiles) == nc.GEOMETRY[name] and plan.tile == nufft.TILE[plan.ndim]
    assert plan.m == (nc.N_CLUSTER + nc.N_UNIFORM if split else nc.N_POINTS)
    assert split or plan.m % 16 != 0  # the last interpolation workgroup has dead groups
    assert np.all(plan.u_host >= 0) and np.all(plan.u_host < np.array(plan.n))
    lengths = plan.item[:, 2] - plan.item[:, 1]
    if split:
        assert plan.n_slabs == nc.SLABS[name] > 0 and plan.chunk < plan.max_list
        assert np.any(lengths % 64 != 0) and np.any(lengths[plan.item[:, 3] >= 0] % 64 != 0)
        assert nc.plan_of(name, chunk=1 << 40).n_slabs == 0
    else:
        assert plan.n_slabs == 0
    if name in nc.POWER_OF_TWO:
        assert nc.zero_r_taps(plan.u_host, plan.w, plan.beta, plan.n) >= 1  # z = -w / 2 exactly: r == 0
    for m in (1, 17):
        assert nc.plan_of(name, m).m == m


def test_what_the_named_cases_are_there_for():
    g = {k: nc.plan_of(k) for k in NAMES}
    assert g["tiny_1d"].n[0] < 256 and g["tiny_1d"].w == 2 and g["flat_3d"].w ** 2 < nc.NU_LANES
    assert g["one_mode"].nmodes[0] // 2 == 0
    for k in ("ring_1d_w15", "ring_1d_w16"):  # last tile ragged, the neighbour window shorter than the ring
        assert g[k].n[0] % 256 == 120 and 2 * g[k].reach[0] + 1 == 5 < g[k].ntiles[0] == 6
    assert g["ring_1d_w16"].w == g["wide_3d"].w == nufft.MAX_WIDTH == nc.NU_WMAX and g["wide_3d"].w ** 2 == 256
    assert g["ragged_2d"].w % 2 == 1 and all(n % t for n, t in zip(g["ragged_2d"].n, g["ragged_2d"].tile))
    p = g["window_2d"]
    assert 2 * p.reach[0] + 1 < p.ntiles[0] and 2 * p.reach[1] + 1 == p.ntiles[1]
    p = g["ragged_3d"]
    assert sum(1 for n, t in zip(p.n, p.tile) if n % t) == 2
    assert int(np.prod([min(2 * r + 1, t) for r, t in zip(p.reach, p.ntiles)])) == 45
    assert int(np.prod(g["split_3d"].ntiles)) == 512 and any(n % t for n, t in zip(g["split_3d_ragged"].n, g["split_3d_ragged"].tile))
    # the placed points: u = 0, integers, halves, a tile boundary and its two neighbours, a repeated point, a wrap on every axis
    p = g["wide_3d"]
    u = p.u_host
    for d, t in enumerate(p.tile):
        col = u[:, d]
        assert {0.0, float(t), float(np.nextafter(t, 0.0)), float(np.nextafter(t, 2.0 * t))} <= set(col.tolist())
        assert np.any(col % 1 == 0.5) and np.any((col % 1 == 0) & (col > 0)) and col.max() > p.n[d] - 1
    assert np.any(np.all(u < p.w / 2, axis=1) & np.all(u > 0, axis=1)) and np.any(np.all(u > np.array(p.n) - 1, axis=1))
    assert len(np.unique(u, axis=0)) <= p.m - 2
    for k in NAMES:  # the largest position below 1 is a point of its own
        if not nc.CASES[k][2]:
            assert np.all(nc.case_points(k)[1] == np.nextafter(1.0, 0.0))
    assert max(int(np.prod(g[k].n)) for k in NAMES) <= 131072 and max(g[k].m for k in NAMES) <= 700
    assert [nc.interp_steps(nd, w) for nd, w in ((1, 16), (2, 9), (3, 2), (3, 6), (3, 16))] == [5, 13, 6, 22, 260]


@pytest.mark.parametrize("name", NAMES)
def test_host_kernels_stay_inside_the_fp64_bound(name):
    plan = nc.plan_of(name)
    v = nc.case_values(name, False)[0]
    flat, prod, rho = nc.exact_taps(plan.u_host, plan.w, plan.beta, plan.n, nc.U64)
    hflat, hw = plan._host_weights(0, plan.m)
    assert np.array_equal(hflat, flat)
    ratio, where = nc.worst(hw, prod, (prod * rho).astype(np.float64))
    print(f"{name} _host_weights: worst error / bound = {ratio:.3f} at {where}")
    assert ratio <= 1
    ex = nc.spread_reference(name, False)
    size = int(np.prod(plan.n))
    host = (np.bincount(hflat.reshape(-1), (hw * v.real[:, None]).reshape(-1), size)
            + 1j * np.bincount(hflat.reshape(-1), (hw * v.imag[:, None]).reshape(-1), size)).reshape(plan.n)
    nc.check(host.real, host.imag, ex, f"{name} host spread grid")
    walked = spread_like_the_device(plan, v)
    nc.check(walked.real, walked.imag, ex, f"{name} spread_like_the_device")


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", NAMES)
def test_restated_device_arithmetic_stays_inside_the_bound(name, tname):
    T, single = TYPES[tname], tname == "fp32"
    plan = nc.plan_of(name)
    v, g, _ = nc.case_values(name, single)
    sx, ix = nc.spread_reference(name, single), nc.interp_reference(name, single)
    for fused in (False, True):
        tag = f"{name} {tname} {'fused' if fused else 'plain'}"
        grid = nc.device_spread(plan, v, T, fused)
        assert not np.any(np.isnan(grid))
        nc.check(*_parts(grid), sx, f"{tag} spread")
        pts = nc.device_interp(plan, g, T, fused)
        nc.check(*_parts(pts), ix, f"{tag} interp")
    if nc.CASES[name][2]:  # the same lists unsplit: another order of the same sums
        whole = nc.device_spread(nc.plan_of(name, chunk=1 << 40), v, T)
        nc.check(*_parts(whole), sx, f"{name} {tname} unsplit spread")
    for m in (1, 17):
        small = nc.plan_of(name, m)
        pts = nc.device_interp(small, g, T)
        nc.check(*_parts(pts), nc.interp_reference(name, single, m), f"{name} {tname} interp m={m}")
        full = nc.device_interp(plan, g, T)
        assert np.array_equal(nc.bits(pts.view(T)), nc.bits(full[:m].view(T)))  # a point's result does not depend on the others


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", NAMES)
def test_crop_and_pad_bits(name, tname):
    T, single = TYPES[tname], tname == "fp32"
    plan = nc.plan_of(name)
    v, g, x = nc.case_values(name, single)
    U = nc.unit(single)
    # roundings on the way: ndim - 1 of the correction's products and the product with the value in double, then the cast.
    # That is within 2 U everywhere except fp64 in 3-D, where ((1 c0) c1) c2 times the value is three roundings: 3 U there.
    k = (plan.ndim * nc.U64 + U) if single else max(2, plan.ndim) * nc.U64
    cex = corr = nc.corr_exact(plan.corr_axes)
    cells = nc._mode_cells(plan.nmodes, plan.n)
    got = nc.crop_bits(g, plan.corr_axes, plan.nmodes, plan.n)
    assert got.dtype == T and got.shape == plan.nmodes
    exact = g.real[cells].astype(LD) * cex
    assert nc.worst(got, exact, (k * np.abs(exact)).astype(np.float64))[0] <= 1
    assert np.array_equal(nc.bits(got), nc.bits(nc.device_crop(plan, g, T)))
    for xin in (x, (x * (1 - 2j)).astype(v.dtype), -0.0 * x):
        got = nc.pad_bits(xin, plan.corr_axes, plan.nmodes, plan.n)
        assert got.dtype == T and got.shape == plan.n + (2,)
        exact = np.zeros(plan.n + (2,), dtype=LD)
        exact[..., 0][cells] = xin.real.astype(LD) * corr
        exact[..., 1][cells] = np.asarray(xin.imag).astype(LD) * corr
        assert nc.worst(got, exact, (k * np.abs(exact)).astype(np.float64))[0] <= 1
        assert np.array_equal(nc.bits(got), nc.bits(nc.device_pad(plan, xin, T)))
        band = np.zeros(plan.n, dtype=bool)
        band[cells] = True
        assert not nc.bits(got)[~band].any() and int(band.sum()) == int(np.prod(plan.nmodes))  # +0 outside the band


# ---- deliberate faults ----------------------------------------------------------------------------------------------------------
def _spread_ratio(name, single, mut):
    T = np.float32 if single else np.float64
    grid = nc.device_spread(nc.plan_of(name), nc.case_values(name, single)[0], T, False, mut)
    return nc.worst_complex(*_parts(grid), nc.spread_reference(name, single))[0]


def _interp_ratio(name, single, mut):
    T = np.float32 if single else np.float64
    pts = nc.device_interp(nc.plan_of(name), nc.case_values(name, single)[1], T, False, mut)
    return nc.worst_complex(*_parts(pts), nc.interp_reference(name, single))[0]


def test_every_deliberate_fault_is_caught():
    lines, seen = [], set()

    def bound_fault(mut, name, single, kernel):
        ratio = (_spread_ratio if kernel == "spread" else _interp_ratio)(name, single, mut)
        assert ratio > 1, (mut, name, kernel, ratio)
        seen.add(mut)
        lines.append("FAULT %s caught=bound kernel=%s case=%s type=%s ratio=%.3e" % (mut, kernel, name, "fp32" if single else "fp64", ratio))

    def tail_fault(mut, name, single, kernel):
        # a tap of e^-36.8 .. 1e-10 of the peak is below the fp32 rounding of a point's sum (the final cast alone allows 6e-8
        # of it): at w = 16 the fp32 interpolation cannot show a fault of the last tap.  The fp32 spreading can, in the cells
        # that only tails reach, and so can both kernels in fp64.
        if single and kernel == "interp":
            ratio = _interp_ratio(name, single, mut)
            assert ratio <= 1
            lines.append("FAULT %s invisible (below fp32 roundoff) kernel=interp case=%s type=fp32 ratio=%.3e" % (mut, name, ratio))
        else:
            bound_fault(mut, name, single, kernel)

    for single in (False, True):
        for kernel in ("spread", "interp"):
            bound_fault("floor_l0", "ragged_2d", single, kernel)
            tail_fault("drop_last_tap", "ring_1d_w16", single, kernel)
            bound_fault("drop_last_tap", "tiny_1d", single, kernel)
            tail_fault("tap15_as_14", "wide_3d", single, kernel)
            bound_fault("sorted_index", "split_3d_ragged", single, kernel)
        bound_fault("no_wrap", "ragged_3d", single, "spread")
        bound_fault("no_wrap", "split_2d", single, "spread")
        bound_fault("tap15_as_14", "ring_1d_w16", single, "spread")
    for kernel in ("spread", "interp"):
        bound_fault("beta_fp32", "ring_1d_w16", False, kernel)
        bound_fault("beta_fp32", "split_3d", False, kernel)
    # tap 15 does not exist below w = 16: the fault is invisible there, which is why the w = 16 cases exist
    assert _spread_ratio("ring_1d_w15", False, "tap15_as_14") <= 1

    def bits_fault(mut, name, single, kernel):
        T = np.float32 if single else np.float64
        plan = nc.plan_of(name)
        v, g, x = nc.case_values(name, single)
        if kernel == "crop":
            want, got = nc.crop_bits(g, plan.corr_axes, plan.nmodes, plan.n), nc.device_crop(plan, g, T, mut)
        else:
            want, got = nc.pad_bits(x, plan.corr_axes, plan.nmodes, plan.n), nc.device_pad(plan, x, T, mut)
        changed = int(np.count_nonzero(nc.bits(want) != nc.bits(got)))
        assert changed > 0, (mut, name, kernel)
        seen.add(mut)
        lines.append("FAULT %s caught=bits kernel=%s case=%s type=%s entries_changed=%d of %d" %
                     (mut, kernel, name, "fp32" if single else "fp64", changed, want.size))

    for single in (False, True):
        for kernel in ("crop", "pad"):
            bits_fault("corr_offset_stuck", "ragged_2d", single, kernel)
            bits_fault("corr_offset_stuck", "split_3d_ragged", single, kernel)
        bits_fault("crop_half_up", "ragged_2d", single, "crop")
        bits_fault("crop_half_up", "ragged_3d", single, "crop")
        bits_fault("pad_band_short", "ragged_2d", single, "pad")
        bits_fault("pad_band_short", "tiny_1d", single, "pad")
    # an even length has (N + 1) // 2 == N // 2: only the odd lengths see that fault
    p = nc.plan_of("split_2d")
    g = nc.case_values("split_2d", False)[1]
    assert np.array_equal(nc.device_crop(p, g, np.float64, "crop_half_up"), nc.device_crop(p, g, np.float64))
    assert seen == set(nc.FAULTS)
    print("\n".join(lines))
