"""Cases, exact results and DERIVED error bounds for the kernels of nifty_amd/csrc/nk_nufft.hip: k_nufft_spread (with
k_nufft_slab_sum), k_nufft_interp, k_nufft_crop and k_nufft_pad (tests/test_nufft_cases.py on the host,
tests/test_nufft_kernels_gpu.py on the device through nk_nufft_*).

References.  They take what the kernels read -- the plan's u_host (doubles, grid units, the caller's order), w, beta, n, nmodes
and the correction tables -- as exact inputs and never look at perm, bin_start, item or the split tables, so an error of the
plan and an error of a kernel both show.  In np.longdouble:
    phi(z) = exp(beta (sqrt(max(1 - (2 z / w)^2, 0)) - 1)),   z = l0 - u + t,   l0 = ceil(u - w / 2),   t < w
    spread_exact   per oversampled cell  sum_j v_j prod_d phi_d          (re and im apart)
    interp_exact   per point             sum_taps prod_d phi_d g[cell]
crop and pad only multiply, which no contraction can change, so crop_bits / pad_bits reproduce the kernels' results bit for bit:
corr = ((1.0 c0) c1) c2 in double, one product with the grid value in double, then (fp32) one cast.

The bound of ONE weight.  The kernels evaluate, in the field's type T with unit roundoff U (2^-53 or 2^-24),
    x = (T)(z0 + t) (T)(2 / w);  r = 1 - x x (contracted or not);  s = sqrt(max(r, 0));  a = beta (s - 1);  exp(a).
Near the edge of the footprint r -> 0, where sqrt turns an absolute error dr into min(dr / (2 sqrt r), sqrt dr) and beta
multiplies it: a flat "few ulp" per weight is wrong by orders of magnitude there (restated in numpy, the worst single weight is
off by 2.5e-3 of itself in fp32 and 1.5e-10 in fp64, always on taps of size e^-beta).  Per tap, in long double:
    dx = 3 U |x| + 2^-53 |z0| 2 / w                 (z0 + t, the cast, the product with the rounded 2 / w; and z0 = l0 - u itself,
                                                     a double rounded relative to |z0| <= w / 2, which the first term misses at the
                                                     central taps where |z0 + t| << |z0|)
    dr = 2 |x| dx + dx^2 + U (x^2 + |1 - x^2|)      (x x and the subtraction; a fused 1 - x x has one rounding less)
    ds = min(sqrt dr, dr / (sqrt(r - dr) + sqrt r)) + SQRT_ULP U s        (only sqrt dr where r <= dr)
    da = beta ds + 3 U beta (1 - s + ds)            (beta in T, s - 1, the product)
    |weight - phi| <= phi (expm1(da) + EXP_ULP U e^da)
SQRT_ULP = EXP_ULP = 2 are the project's figures for the device library: "exp and sqrt of the device library are within
1 ulp = 2 u" (tests/amp_cases.py).  No other constant enters.
One term.  rho = prod_d (1 + rel_d) (1 + U)^(ND + 1) - 1: the axes' relative weight bounds and ND + 1 products in T (the weights
with each other and with the value), to first order with the cross terms added.
One cell / point.  sum |term| rho  +  gamma_L sum |term|  +  U |result|, gamma_L = L 2^-53 / (1 - L 2^-53) for the fp64 sum of L
terms and the last for the final cast.  Interpolation: L = the taps one lane adds plus the 4 steps of the lane tree.
Spreading: L = the number of points that cover the cell.  (A sum of L terms IN ANY ORDER stays within gamma_(L-1) sum |term|,
Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2 -- chunks and slabs are one such order, and the
zeros of points that miss the cell are never added -- so L does not have to be the longer list the tile walks.)
The bounds are applied with factor 1.

The restatement.  device_weights / device_spread / device_interp / device_crop / device_pad are the kernels' arithmetic and
index walks in numpy, in float32 or float64, with either form of 1 - x x, the tile lists in the kernel's order and the chunked
slabs.  A `mut` writes ONE deliberate fault (FAULTS) into them, which the bounds or the bits have to catch.
"""
import functools

import numpy as np
import pytest

from nifty_amd import nufft

LD = np.longdouble
U64 = 2.0 ** -53
U32 = 2.0 ** -24
SQRT_ULP = 2  # in units of U: "within 1 ulp = 2 u"
EXP_ULP = 2
NU_WMAX = 16
NU_LANES = 16
NU_CELLS = 256
N_POINTS = 300
N_CLUSTER, N_UNIFORM, SPLIT_CHUNK = 600, 40, 50

# name -> (nmodes, eps, split lists?, seed of the points)
CASES = {
    "tiny_1d": ((5,), 1.0, False, 1),
    "one_mode": ((1,), 1e-2, False, 2),
    "ring_1d_w15": ((700,), 2e-13, False, 3),
    "ring_1d_w16": ((700,), 1e-14, False, 3),
    "ragged_2d": ((13, 9), 1e-7, False, 4),
    "window_2d": ((40, 24), 1e-4, False, 5),
    "ragged_3d": ((9, 10, 11), 1e-4, False, 6),
    "wide_3d": ((8, 8, 8), 1e-14, False, 7),
    "flat_3d": ((1, 3, 2), 1.0, False, 8),
    "split_1d": ((1500,), 2e-13, True, 18),
    "split_2d": ((64, 64), 1e-4, True, 14),
    "split_3d": ((16, 32, 32), 1e-2, True, 17),
    "split_3d_ragged": ((24, 27, 20), 1e-2, True, 27),
}
# name -> (w, oversampled n, tiles per axis)
GEOMETRY = {
    "tiny_1d": (2, (10,), (1,)),
    "one_mode": (4, (8,), (1,)),
    "ring_1d_w15": (15, (1400,), (6,)),
    "ring_1d_w16": (16, (1400,), (6,)),
    "ragged_2d": (9, (27, 18), (2, 2)),
    "window_2d": (6, (80, 48), (5, 3)),
    "ragged_3d": (6, (18, 20, 24), (5, 3, 3)),
    "wide_3d": (16, (32, 32, 32), (8, 4, 4)),
    "flat_3d": (2, (4, 6, 4), (1, 1, 1)),
    "split_1d": (15, (3000,), (12,)),
    "split_2d": (6, (128, 128), (8, 8)),
    "split_3d": (4, (32, 64, 64), (8, 8, 8)),
    "split_3d_ragged": (4, (48, 54, 40), (12, 7, 5)),
}
SLABS = {"split_1d": 10, "split_2d": 121, "split_3d": 362, "split_3d_ragged": 598}  # of these seeds, at CHUNK = 50
POWER_OF_TWO = ("one_mode", "wide_3d", "split_2d", "split_3d")  # every n a power of two: the aligned points are exact
FAULTS = ("floor_l0", "no_wrap", "drop_last_tap", "tap15_as_14", "beta_fp32", "corr_offset_stuck", "crop_half_up",
          "pad_band_short", "sorted_index")


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def unit(single):
    return U32 if single else U64


# ---- points and plans ---------------------------------------------------------------------------------------------------------
def _pos_for(target, n):
    """a position in [0, 1) whose product with n is the double `target` if a neighbour of target / n gives it (always so for
    a power of two), else the closest there is"""
    p = best = target / n
    cands = [p]
    lo = hi = p
    for _ in range(4):
        lo, hi = np.nextafter(lo, -1.0), np.nextafter(hi, 2.0)
        cands += [lo, hi]
    for c in cands:
        if 0.0 <= c < 1.0 and abs(c * n - target) < abs(best * n - target):
            best = c
    return min(max(best, 0.0), np.nextafter(1.0, 0.0))


def _special_u(n, w, tile, ntiles):
    """the placed coordinates of one axis, in grid units"""
    last = (ntiles - 1) * tile
    b1 = float(tile if ntiles > 1 else n // 2)  # a tile boundary (the middle of a one-tile axis)
    b2 = float(last if ntiles > 2 else max(1, n // 2 - 1))
    out = [0.0, None,  # None: the largest position below 1
           float(n // 3), float(n - 1), n // 3 + 0.5, n - 0.5,
           b1, np.nextafter(b1, 0.0), np.nextafter(b1, 2.0 * b1), b2, np.nextafter(b2, 0.0), np.nextafter(b2, 2.0 * b2),
           last + 0.3 * (n - last),  # in the (ragged) last tile
           0.25, n - 0.25]  # the footprint wraps below 0 / past n
    return out


def case_points(name):
    """positions (m, ndim) in [0, 1) (distances 1), the placed ones first"""
    nmodes, eps, split, seed = CASES[name]
    w, n, ntiles = GEOMETRY[name]
    nd = len(nmodes)
    rng = np.random.default_rng(seed)
    if split:
        cluster = np.mod(0.998 + 0.004 * rng.random((N_CLUSTER, nd)), 1.0)
        cluster[0] = 0.0  # u = 0 on every axis: z = -w / 2 exactly for these even widths
        return np.concatenate([cluster, rng.random((N_UNIFORM, nd))])
    cols = []
    for d in range(nd):
        us = _special_u(n[d], w, nufft.TILE[nd][d], ntiles[d])
        cols.append([np.nextafter(1.0, 0.0) if u is None else _pos_for(u, n[d]) for u in us])
    placed = np.array(cols).T
    blocks = [placed]
    if nd > 1:  # the same coordinates, a different one on every axis
        blocks.append(np.stack([np.roll(placed[:, d], 4 * d + 1) for d in range(nd)], axis=1))
    rep = rng.random((1, nd))
    blocks.append(np.repeat(rep, 3, axis=0))
    fixed = np.concatenate(blocks)
    return np.concatenate([fixed, rng.random((N_POINTS - len(fixed), nd))])


def make_plan(name, m=None, chunk=None):
    """the case's NufftPlan (its first m points); split cases with nufft.CHUNK = SPLIT_CHUNK unless `chunk` is given"""
    nmodes, eps, split, _ = CASES[name]
    pos = case_points(name)
    if m is not None:
        pos = pos[:m]
    with pytest.MonkeyPatch.context() as mp:
        if chunk is not None or split:
            mp.setattr(nufft, "CHUNK", SPLIT_CHUNK if chunk is None else chunk)
        return nufft.NufftPlan(nmodes, [1.0] * len(nmodes), pos, eps)


@functools.lru_cache(maxsize=None)
def plan_of(name, m=None, chunk=None):
    return make_plan(name, m, chunk)


def case_values(name, single, m=None):
    """the points' values and a grid of the oversampled shape, complex, in the field's precision; never modified"""
    plan = plan_of(name, m)
    rng = np.random.default_rng(100 + CASES[name][3])
    ct = np.complex64 if single else np.complex128
    v = (rng.standard_normal(plan.m) + 1j * rng.standard_normal(plan.m)).astype(ct)
    g = (rng.standard_normal(plan.n) + 1j * rng.standard_normal(plan.n)).astype(ct)
    x = rng.standard_normal(plan.nmodes).astype(v.real.dtype)
    for a in (v, g, x):
        a.setflags(write=False)
    return v, g, x


# ---- exact weights and their bounds -------------------------------------------------------------------------------------------
def exact_axis(u, w, beta, n, U):
    """one axis: wrapped cell index [m, w], phi [m, w] and the relative bound of the weight evaluated in unit roundoff U"""
    uL = np.asarray(u, dtype=np.float64).astype(LD)
    h = LD(w) / 2
    l0 = np.ceil(uL - h)
    z = (l0 - uL)[:, None] + np.arange(w).astype(LD)[None, :]
    x = z / h
    r = np.maximum((h - z) * (h + z) / (h * h), LD(0))  # 1 - x^2 without the cancellation
    s = np.sqrt(r)
    bL = LD(beta)
    phi = np.exp(bL * (s - 1))
    U = LD(U)
    ax = np.abs(x)
    z0 = np.abs(l0 - uL)[:, None]
    dx = 3 * U * ax + LD(U64) * z0 / h  # z0 = l0 - u is rounded in double relative to |z0|, not to |z0 + t|
    dr = 2 * ax * dx + dx * dx + U * (x * x + r)
    wide = r > dr
    ds = np.sqrt(dr)
    ds = np.where(wide, np.minimum(ds, dr / (np.sqrt(np.where(wide, r - dr, LD(1))) + np.sqrt(np.where(wide, r, LD(1))))), ds)
    ds = ds + SQRT_ULP * U * s
    da = bL * ds + 3 * U * bL * (1 - s + ds)
    rel = np.expm1(da) + EXP_ULP * U * np.exp(da)
    idx = (l0.astype(np.int64)[:, None] + np.arange(w)[None, :]) % n
    return idx, phi, rel, r


def exact_taps(u_host, w, beta, n, U):
    """flat oversampled cell [m, w^nd], prod phi and rho of every (point, tap)"""
    u_host = np.asarray(u_host, dtype=np.float64)
    m, nd = u_host.shape
    flat = np.zeros((m, 1), dtype=np.int64)
    prod = np.ones((m, 1), dtype=LD)
    grow = np.ones((m, 1), dtype=LD)
    for d in range(nd):
        idx, phi, rel, _ = exact_axis(u_host[:, d], w, beta, n[d], U)
        flat = (flat[:, :, None] * n[d] + idx[:, None, :]).reshape(m, -1)
        prod = (prod[:, :, None] * phi[:, None, :]).reshape(m, -1)
        grow = (grow[:, :, None] * (1 + rel)[:, None, :]).reshape(m, -1)
    rho = grow * (1 + LD(U)) ** (nd + 1) - 1
    return flat, prod, rho


def zero_r_taps(u_host, w, beta, n):
    """taps with r == 0 exactly (z = -w / 2), over all axes"""
    return sum(int(np.count_nonzero(exact_axis(u_host[:, d], w, beta, n[d], U64)[3] == 0)) for d in range(u_host.shape[1]))


def _segment_sums(order, starts, cells, size, *arrays):
    out = []
    for a in arrays:
        full = np.zeros(size, dtype=LD)
        if len(order):
            full[cells] = np.add.reduceat(a.reshape(-1)[order], starts)
        out.append(full)
    return out


def spread_exact(u_host, w, beta, n, v, single):
    """{"re", "im"} exact sums per oversampled cell (longdouble, shape n), {"bound_re", "bound_im"} (float64), "count" = the
    points covering every cell"""
    U = unit(single)
    size = int(np.prod(n))
    flat, prod, rho = exact_taps(u_host, w, beta, n, U)
    v = np.asarray(v)
    vr, vi = v.real.astype(LD)[:, None], v.imag.astype(LD)[:, None]
    order = np.argsort(flat.reshape(-1), kind="stable")
    sorted_cells = flat.reshape(-1)[order]
    starts = np.nonzero(np.diff(sorted_cells, prepend=-1))[0] if len(order) else np.zeros(0, dtype=np.int64)
    cells = sorted_cells[starts] if len(order) else starts
    count = np.bincount(flat.reshape(-1), minlength=size)
    re, im, are, aim, cre, cim = _segment_sums(order, starts, cells, size, vr * prod, vi * prod, np.abs(vr) * prod,
                                               np.abs(vi) * prod, np.abs(vr) * prod * rho, np.abs(vi) * prod * rho)
    g = gamma(np.maximum(count, 1)).astype(LD)
    out = {"re": re.reshape(n), "im": im.reshape(n), "count": count.reshape(n),
           "bound_re": (cre + g * are + LD(U) * np.abs(re)).astype(np.float64).reshape(n),
           "bound_im": (cim + g * aim + LD(U) * np.abs(im)).astype(np.float64).reshape(n)}
    for a in out.values():
        a.setflags(write=False)
    return out


def interp_steps(nd, w):
    """L of the interpolation: the taps one lane adds plus the 4 steps of the lane tree"""
    rows = 1 if nd == 1 else (w if nd == 2 else w * w)
    taps = 1 if nd == 1 else -(-rows // NU_LANES) * w
    return taps + 4


def interp_exact(u_host, w, beta, n, g, single):
    """{"re", "im"} exact sums per point (longdouble), {"bound_re", "bound_im"} (float64)"""
    U = unit(single)
    flat, prod, rho = exact_taps(u_host, w, beta, n, U)
    gf = np.asarray(g).reshape(-1)
    gr, gi = gf.real.astype(LD)[flat], gf.imag.astype(LD)[flat]
    re, im = (prod * gr).sum(axis=1), (prod * gi).sum(axis=1)
    k = gamma(interp_steps(u_host.shape[1], w))
    out = {"re": re, "im": im,
           "bound_re": ((np.abs(gr) * prod * rho).sum(axis=1) + k * (np.abs(gr) * prod).sum(axis=1) + LD(U) * np.abs(re)).astype(np.float64),
           "bound_im": ((np.abs(gi) * prod * rho).sum(axis=1) + k * (np.abs(gi) * prod).sum(axis=1) + LD(U) * np.abs(im)).astype(np.float64)}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- crop and pad: the bits -----------------------------------------------------------------------------------------------------
def _corr_product(corr_axes):
    c = 1.0 * np.asarray(corr_axes[0], dtype=np.float64)
    for a in corr_axes[1:]:
        c = np.multiply.outer(c, np.asarray(a, dtype=np.float64))
    return c


def _mode_cells(nmodes, n):
    return np.ix_(*[(np.arange(N) - N // 2) % nn for N, nn in zip(nmodes, n)])


def crop_bits(grid, corr_axes, nmodes, n):
    """k_nufft_crop: the real part of the centred modes times the correction, in the grid's real type"""
    grid = np.asarray(grid)
    return (grid.real[_mode_cells(nmodes, n)].astype(np.float64) * _corr_product(corr_axes)).astype(grid.real.dtype)


def pad_bits(x, corr_axes, nmodes, n):
    """k_nufft_pad: [n..., 2] re / im of the oversampled grid, +0 outside the band (and in im for a real x)"""
    x = np.asarray(x)
    rt = x.real.dtype
    out = np.zeros(tuple(n) + (2,), dtype=rt)
    c = _corr_product(corr_axes)
    cells = _mode_cells(nmodes, n)
    out[..., 0][cells] = (x.real.astype(np.float64) * c).astype(rt)
    if np.iscomplexobj(x):
        out[..., 1][cells] = (x.imag.astype(np.float64) * c).astype(rt)
    return out


def corr_exact(corr_axes):
    c = np.asarray(corr_axes[0]).astype(LD)
    for a in corr_axes[1:]:
        c = np.multiply.outer(c, np.asarray(a).astype(LD))
    return c


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the kernels restated in numpy ----------------------------------------------------------------------------------------------
def device_weights(u, w, beta, T, fused=False, mut=None):
    """nu_first_cell and nu_es for every point and axis: first cell [m, nd] (unwrapped) and the NU_WMAX weights [m, nd, 16]"""
    u = np.asarray(u, dtype=np.float64)
    l = (np.floor if mut == "floor_l0" else np.ceil)(u - 0.5 * w)
    z0 = l - u
    zt = (z0[..., None] + np.arange(NU_WMAX, dtype=np.float64)).astype(T)
    x = zt * T(2.0 / w)
    if fused:
        # fp32: x x is exact in double and the one rounding to double before the cast matters only on ties.  fp64: the 64-bit
        # long double rounds x x once more before the result is rounded to double, so this is a double rounding and no true
        # fma: it can differ from the device's by one ulp of r near the footprint's edge.  An approximate contracted path --
        # the bound, which allows the subtraction's full rounding, does not depend on it.
        wide = LD if T is np.float64 else np.float64
        r = (wide(1) - x.astype(wide) * x.astype(wide)).astype(T)
    else:
        r = T(1) - x * x
    s = np.sqrt(np.maximum(r, T(0)))
    b = T(np.float32(beta)) if mut == "beta_fp32" else T(beta)
    ker = np.exp(b * (s - T(1))).astype(T)
    ker[..., (w - 1 if mut == "drop_last_tap" else w):] = 0
    return l.astype(np.int64), ker


def _tile_cells(plan, tc):
    """the 256 cells of tile tc in the order of the workgroup's threads"""
    return np.stack(np.meshgrid(*[tc[d] * plan.tile[d] + np.arange(plan.tile[d]) for d in range(plan.ndim)], indexing="ij"),
                    -1).reshape(-1, plan.ndim)


def device_spread(plan, v, T, fused=False, mut=None):
    """k_nufft_spread + k_nufft_slab_sum: [n..., 2] in T, NaN where no thread wrote"""
    nd, w = plan.ndim, plan.w
    n, tile, ntiles = np.array(plan.n), np.array(plan.tile), np.array(plan.ntiles)
    l0, ker = device_weights(plan.u, w, plan.beta, T, fused, mut)
    if mut != "no_wrap":
        l0 = np.where(l0 < 0, l0 + n[None, :], l0)
    v = np.asarray(v)
    vs = v if mut == "sorted_index" else v[plan.perm]
    vr, vi = vs.real.astype(T), vs.imag.astype(T)
    grid = np.full(tuple(plan.n) + (2,), np.nan, dtype=T)
    slabs = np.zeros((plan.n_slabs, NU_CELLS, 2))
    top = NU_WMAX - 2 if mut == "tap15_as_14" else NU_WMAX - 1
    for tl, lo, hi, sl in plan.item:
        tc = np.unravel_index(tl, plan.ntiles)
        axes = []
        for d in range(nd):
            span = 2 * plan.reach[d] + 1
            b0 = (tc[d] - plan.reach[d] + ntiles[d]) % ntiles[d] if span < ntiles[d] else 0
            axes.append([(b0 + o) % ntiles[d] for o in range(min(span, ntiles[d]))])
        bins = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, nd)
        bins = np.ravel_multi_index(tuple(bins.T), plan.ntiles)
        lst = np.concatenate([np.arange(plan.bin_start[b], plan.bin_start[b + 1]) for b in bins])[lo:hi]
        cells = _tile_cells(plan, tc)
        ts = np.array(tc) * tile
        a, b = ts[None, :] - l0[lst], l0[lst] - ts[None, :]
        hit = np.all((np.where(a < 0, a + n, a) < w) | (np.where(b < 0, b + n, b) < tile), axis=1)
        q = lst[hit]
        acc = np.zeros((NU_CELLS, 2))
        if len(q):
            dd = cells[None, :, :] - l0[q][:, None, :]
            dd = dd + np.where(dd < 0, n, 0)
            inn = np.all(dd < w, axis=2)
            tap = np.minimum(dd, top)
            k = np.ones(inn.shape, dtype=T)
            for d in range(nd):
                k = k * ker[q[:, None], d, tap[:, :, d]]
            tr = np.where(inn, (k * vr[q][:, None]).astype(np.float64), 0.0)
            ti = np.where(inn, (k * vi[q][:, None]).astype(np.float64), 0.0)
            acc = np.stack([np.cumsum(tr, axis=0)[-1], np.cumsum(ti, axis=0)[-1]], axis=1)  # point after point
        if sl >= 0:
            slabs[sl] = acc
        else:
            inside = np.all(cells < n[None, :], axis=1)
            grid[tuple(cells[inside].T)] = acc[inside].astype(T)
    for k, tl in enumerate(plan.split_tile):
        cells = _tile_cells(plan, np.unravel_index(tl, plan.ntiles))
        inside = np.all(cells < n[None, :], axis=1)
        tot = np.zeros((NU_CELLS, 2))
        for s in range(plan.split_slab[k], plan.split_slab[k + 1]):
            tot = tot + slabs[s]
        grid[tuple(cells[inside].T)] = tot[inside].astype(T)
    return grid


def device_interp(plan, g, T, fused=False, mut=None):
    """k_nufft_interp: complex [m] in T at the original indices (NaN where nothing was written)"""
    nd, w, m = plan.ndim, plan.w, plan.m
    n = np.array(plan.n)
    l0, ker = device_weights(plan.u, w, plan.beta, T, fused, mut)
    l0 = np.where(l0 < 0, l0 + n[None, :], l0)
    gf = np.asarray(g).reshape(-1)
    gr, gi = gf.real.astype(T), gf.imag.astype(T)
    acc = np.zeros((m, NU_LANES, 2))
    lane = np.arange(NU_LANES)
    top = NU_WMAX - 2 if mut == "tap15_as_14" else NU_WMAX - 1
    ker = ker[:, :, np.minimum(np.arange(NU_WMAX), top)]
    if nd == 1:
        i = (l0[:, 0:1] + lane[None, :]) % n[0]
        live = lane[None, :] < w
        acc[..., 0] = np.where(live, (ker[:, 0, :] * gr[i]).astype(np.float64), 0.0)
        acc[..., 1] = np.where(live, (ker[:, 0, :] * gi[i]).astype(np.float64), 0.0)
    else:
        nrows = w if nd == 2 else w * w
        for r0 in range(0, nrows, NU_LANES):
            r = r0 + lane
            on = r < nrows
            rc = np.where(on, r, 0)
            t0, t1 = (rc, np.zeros_like(rc)) if nd == 2 else (rc // w, rc % w)
            krow = ker[:, 0, :][:, t0]
            row = (l0[:, 0:1] + t0[None, :]) % n[0]
            if nd == 3:
                krow = krow * ker[:, 1, :][:, t1]
                row = row * n[1] + (l0[:, 1:2] + t1[None, :]) % n[1]
            for t in range(w):
                cell = row * n[nd - 1] + ((l0[:, nd - 1] + t) % n[nd - 1])[:, None]
                k = krow * ker[:, nd - 1, t][:, None]
                acc[..., 0] += np.where(on[None, :], (k * gr[cell]).astype(np.float64), 0.0)
                acc[..., 1] += np.where(on[None, :], (k * gi[cell]).astype(np.float64), 0.0)
    off = NU_LANES // 2
    while off:
        acc = acc + acc[:, lane ^ off, :]
        off >>= 1
    out = np.full(m, np.nan + 0j, dtype=np.complex64 if T is np.float32 else np.complex128)
    res = acc[:, 0, 0].astype(T) + 1j * acc[:, 0, 1].astype(T)
    out[np.arange(m) if mut == "sorted_index" else plan.perm] = res
    return out


def device_crop(plan, grid, T, mut=None):
    """k_nufft_crop, index by index"""
    nd = plan.ndim
    gre = np.asarray(grid).real.astype(T).reshape(-1)
    ids = np.unravel_index(np.arange(int(np.prod(plan.nmodes))), plan.nmodes)
    cell = np.zeros(len(ids[0]), dtype=np.int64)
    corr = np.ones(len(ids[0]))
    off = 0
    for d in range(nd):
        N = plan.nmodes[d]
        k = ids[d] - ((N + 1) // 2 if mut == "crop_half_up" else N // 2)
        k = k + np.where(k < 0, plan.n[d], 0)
        cell = cell * plan.n[d] + k
        corr = corr * plan.corr[off + ids[d]]
        off += 0 if mut == "corr_offset_stuck" else N
    return (gre[cell].astype(np.float64) * corr).astype(T).reshape(plan.nmodes)


def device_pad(plan, x, T, mut=None):
    """k_nufft_pad, cell by cell: [n..., 2] in T"""
    nd = plan.ndim
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    xr = x.real.astype(T).reshape(-1)
    xi = x.imag.astype(T).reshape(-1) if cplx else None
    ld = np.unravel_index(np.arange(int(np.prod(plan.n))), plan.n)
    inside = np.ones(len(ld[0]), dtype=bool)
    idx = np.zeros(len(ld[0]), dtype=np.int64)
    corr = np.ones(len(ld[0]))
    off = 0
    for d in range(nd):
        nm, nn = plan.nmodes[d], plan.n[d]
        half = nm // 2
        upper = ld[d] > nn - half if mut == "pad_band_short" else ld[d] >= nn - half
        k = np.where(ld[d] < nm - half, ld[d], np.where(upper, ld[d] - nn, nn))
        inside = inside & (k != nn)
        i = np.where(inside, k + half, 0)
        idx = idx * nm + i
        corr = corr * plan.corr[off + i]
        off += 0 if mut == "corr_offset_stuck" else nm
    out = np.zeros((len(idx), 2), dtype=T)
    out[:, 0] = np.where(inside, (xr[idx].astype(np.float64) * corr).astype(T), T(0))
    if cplx:
        out[:, 1] = np.where(inside, (xi[idx].astype(np.float64) * corr).astype(T), T(0))
    return out.reshape(tuple(plan.n) + (2,))


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def worst(got, exact, bound):
    """(largest |got - exact| / bound, its index); a NaN or an error where the bound is 0 counts as infinite"""
    diff = np.abs(np.asarray(got).astype(LD) - np.asarray(exact).astype(LD)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(diff), np.inf, ratio)
    if ratio.size == 0:
        return 0.0, ()
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), tuple(int(i) for i in np.unravel_index(k, ratio.shape))


def worst_complex(got_re, got_im, ex):
    """worst of the two parts against an exact-result record; returns (ratio, index, part)"""
    a, b = worst(got_re, ex["re"], ex["bound_re"]), worst(got_im, ex["im"], ex["bound_im"])
    return (a[0], a[1], "re") if a[0] >= b[0] else (b[0], b[1], "im")


def check(got_re, got_im, ex, what):
    """every entry within its bound, factor 1; the worst used fraction and its place are printed first"""
    ratio, where, part = worst_complex(got_re, got_im, ex)
    print(f"{what}: worst error / bound = {ratio:.3f} at {where} ({part})")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the bound at {where} ({part})"
    return ratio


# ---- shared references: computed once per case and type, read-only ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spread_reference(name, single):
    p = plan_of(name)
    return spread_exact(p.u_host, p.w, p.beta, p.n, case_values(name, single)[0], single)


@functools.lru_cache(maxsize=None)
def interp_reference(name, single, m=None):
    p = plan_of(name, m)
    return interp_exact(p.u_host, p.w, p.beta, p.n, case_values(name, single)[1], single)
