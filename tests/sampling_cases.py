"""Cases, exact results and derived error bounds for LinearInterpolator and RegriddingOperator (tests/test_sampling_ops.py,
tests/test_sampling_ops_gpu.py, tests/golden/make_golden_sampling.py).

The exact result of every map is formed in np.longdouble from the fp64 quantities of the definition (cell, e / bindex,
frac: docs/SAMPLING.md); an fp64 implementation is held to
    |got - exact| <= gamma_k (|A| |x|),   gamma_k = k u / (1 - k u),   u = 2^-53,
elementwise, where |A| has the absolute weights and k counts the rounding steps on the longest path from an input to an
output (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: a sum of products, in any order):
  interpolator TIMES    2^d + d + 2 : 2^d - 1 additions, and per term at most d roundings of 1 - e_a, d - 1 products of the
                                      weight and one product with x: 2^d + 2 d - 1 steps, within 2^d + d + 2 for d <= 3
  interpolator ADJOINT  L + d + 2   : L = most (point, corner) contributions into one grid cell: L - 1 additions in ANY order
                                      (per-corner partial sums, lane trees) and the same 2 d steps per term
  regridding TIMES      3 d         : per axis one rounding of 1 - f, one product, one addition
  regridding ADJOINT    sum_a (L_a + 2): per axis 1 - f, one product, L_a - 1 additions (L_a = most contributions into one
                                      old cell along axis a)
fp32 fields add u32 |exact| for the single final rounding (u32 = 2^-24; the inputs are fp32 numbers taken exactly).
A comparison of two rounded sides (host against golden, device against host) uses twice the bound.
"""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
LD = np.longdouble

# name -> list of (shape, distances or None) of the RGSpaces of the domain
INTERP_CASES = {
    "1d": [((7,), (0.3,))],
    "2d": [((5, 7), (0.2, 1.12))],
    "3d": [((5, 7, 6), (0.2, 1.12, 0.7))],
    "len123": [((1, 2, 3), None)],
    "two_1d": [((4,), None), ((6,), None)],
}
N_POINTS = 300  # per case, the fixed points included (the golden file holds every point)

# name -> (domain description, new_shape, space); a domain entry is ("rg", shape) or ("u", n)
REGRID_CASES = {
    "2d": ([("rg", (8, 6))], (5, 6), 0),
    "middle": ([("u", 3), ("rg", (7,)), ("u", 2)], (4,), 1),
    "clamped": ([("rg", (5,))], (5,), 0),
    "two_to_one": ([("rg", (2,))], (1,), 0),
    "length_one": ([("rg", (1, 5))], (1, 5), 0),
}


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def grid_of(spaces):
    """(shape, distances) of the combined grid of an INTERP_CASES entry (default distances 1 / N, as RGSpace's)"""
    shape = tuple(n for shp, _ in spaces for n in shp)
    dist = tuple(d for shp, dst in spaces for d in (dst if dst is not None else tuple(1.0 / n for n in shp)))
    return shape, dist


def interp_points(shape, dist, rng, n=N_POINTS):
    """n points: drawn over [-2, 3] box lengths, and on every axis at once: at 0, exactly at the box length, at -1e-17 L
    (e rounds to 1), on an interior node and in the last cell (its upper corners wrap to index 0)"""
    length = np.array(shape) * np.array(dist)
    fixed = np.stack([0.0 * length, length, -1e-17 * length, (np.array(shape) // 2) * np.array(dist),
                      (np.array(shape) - 0.5) * np.array(dist)], axis=1)
    drawn = (rng.random((len(shape), n - fixed.shape[1])) * 5.0 - 2.0) * length[:, None]
    return np.ascontiguousarray(np.concatenate([drawn, fixed], axis=1))


def interp_exact(shape, dist, points, x=None, y=None):
    """longdouble TIMES of x and ADJOINT_TIMES of y with their |A||.| companions, and L"""
    shape = tuple(shape)
    nd = len(shape)
    pos = np.asarray(points, dtype=np.float64) / np.asarray(dist, dtype=np.float64).reshape(-1, 1)
    low = np.floor(pos)
    e = (pos - low).astype(LD)
    cell = low.astype(np.int64)
    size = int(np.prod(shape))
    out = {"L": 0}
    count = np.zeros(size, dtype=np.int64)
    if x is not None:
        xf = np.asarray(x).reshape(-1).astype(LD)
        out["times"], out["times_abs"] = np.zeros(pos.shape[1], dtype=LD), np.zeros(pos.shape[1], dtype=LD)
    if y is not None:
        yl = np.asarray(y).astype(LD)
        out["adjoint"], out["adjoint_abs"] = np.zeros(size, dtype=LD), np.zeros(size, dtype=LD)
    for m in range(1 << nd):
        idx, w = np.zeros(pos.shape[1], dtype=np.int64), np.ones(pos.shape[1], dtype=LD)
        for a in range(nd):
            bit = (m >> (nd - 1 - a)) & 1
            idx = idx * shape[a] + (cell[a] + bit) % shape[a]
            w = w * (e[a] if bit else LD(1) - e[a])
        count += np.bincount(idx, minlength=size)
        if x is not None:
            out["times"] += w * xf[idx]
            out["times_abs"] += np.abs(w) * np.abs(xf[idx])
        if y is not None:
            np.add.at(out["adjoint"], idx, w * yl)
            np.add.at(out["adjoint_abs"], idx, np.abs(w) * np.abs(yl))
    out["L"] = int(count.max()) if pos.shape[1] else 0
    if y is not None:
        out["adjoint"], out["adjoint_abs"] = out["adjoint"].reshape(shape), out["adjoint_abs"].reshape(shape)
    return out


def interp_bounds(shape, ex, single=False):
    """elementwise bounds (fp64 arrays) of TIMES and ADJOINT_TIMES from interp_exact's output"""
    d = len(shape)
    out = {}
    if "times" in ex:
        out["times"] = gamma(2 ** d + d + 2) * ex["times_abs"] + (U32 * np.abs(ex["times"]) if single else 0)
    if "adjoint" in ex:
        out["adjoint"] = gamma(ex["L"] + d + 2) * ex["adjoint_abs"] + (U32 * np.abs(ex["adjoint"]) if single else 0)
    return {k: v.astype(np.float64) for k, v in out.items()}


def regrid_tables(n_old, n_new, dist=1.0):
    """bindex, frac of one axis, as the definition computes them in fp64"""
    newdist = dist * n_old / n_new
    tmp = np.arange(n_new) * (newdist / dist)
    b = np.minimum(n_old - 2, tmp.astype(np.int64))
    return b, tmp - b


def regrid_exact(full_shape, axes, old, new, dists, x=None, y=None):
    """longdouble TIMES of x (full_shape with the old lengths) and ADJOINT_TIMES of y (with the new lengths) along `axes` (field
    axes; old / new / dists per axis), with the |A||.| companions and the per-axis L_a; axes of old length 1 are the identity"""
    out = {"L": []}
    tabs = []
    for a, n_old, n_new, dist in zip(axes, old, new, dists):
        if n_old == 1:
            continue
        b, f = regrid_tables(n_old, n_new, dist)
        tabs.append((a, n_old, b, f.astype(LD)))
        out["L"].append(int((np.bincount(b, minlength=n_old) + np.bincount(b + 1, minlength=n_old)).max()))
    if x is not None:
        v, va = np.asarray(x).astype(LD), np.abs(np.asarray(x)).astype(LD)
        for a, n_old, b, f in tabs:
            fs = f.reshape((1,) * a + (-1,) + (1,) * (v.ndim - a - 1))
            v = np.take(v, b, axis=a) * (LD(1) - fs) + np.take(v, b + 1, axis=a) * fs
            va = np.take(va, b, axis=a) * np.abs(LD(1) - fs) + np.take(va, b + 1, axis=a) * np.abs(fs)
        out["times"], out["times_abs"] = v, va
    if y is not None:
        v, va = np.asarray(y).astype(LD), np.abs(np.asarray(y)).astype(LD)
        for a, n_old, b, f in tabs:
            fs = f.reshape((1,) * a + (-1,) + (1,) * (v.ndim - a - 1))
            shp = list(v.shape)
            shp[a] = n_old
            nv, nva = np.zeros(shp, dtype=LD), np.zeros(shp, dtype=LD)
            idx = (slice(None),) * a
            np.add.at(nv, idx + (b,), v * (LD(1) - fs))
            np.add.at(nv, idx + (b + 1,), v * fs)
            np.add.at(nva, idx + (b,), va * np.abs(LD(1) - fs))
            np.add.at(nva, idx + (b + 1,), va * np.abs(fs))
            v, va = nv, nva
        out["adjoint"], out["adjoint_abs"] = v, va
    return out


def regrid_bounds(ex, single=False):
    d = len(ex["L"])
    out = {}
    if "times" in ex:
        out["times"] = gamma(max(1, 3 * d)) * ex["times_abs"] + (U32 * np.abs(ex["times"]) if single else 0)
    if "adjoint" in ex:
        out["adjoint"] = gamma(max(1, sum(la + 2 for la in ex["L"]))) * ex["adjoint_abs"] + (U32 * np.abs(ex["adjoint"]) if single else 0)
    return {k: v.astype(np.float64) for k, v in out.items()}


def regrid_layout(case):
    """(field shape, axes of the regridded space, old lengths, new lengths, distances, target field shape)"""
    desc, new_shape, space = case
    shape, axes, old, dists = [], [], [], []
    for k, (kind, val) in enumerate(desc):
        if kind == "rg":
            if k == space:
                axes = list(range(len(shape), len(shape) + len(val)))
                old = list(val)
                dists = [1.0 / n for n in val]
            shape += list(val)
        else:
            shape.append(val)
    tshape = list(shape)
    for a, n in zip(axes, new_shape):
        tshape[a] = n
    return tuple(shape), axes, old, list(new_shape), dists, tuple(tshape)


def err_ok(got, exact, bound):
    """elementwise |got - exact| <= bound, the difference taken in longdouble; returns (ok, worst ratio)"""
    diff = np.abs(np.asarray(got).astype(LD) - np.asarray(exact).astype(LD)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    ok = bool(np.all(diff <= bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    return ok, float(ratio.max()) if ratio.size else 0.0


def check(got, exact, bound, what, factor=1.0):
    """assert |got - exact| <= factor * bound elementwise; the worst fraction of the allowed bound is printed first"""
    ok, worst = err_ok(got, exact, factor * np.asarray(bound, dtype=np.float64))
    print(f"{what}: worst |got - exact| = {worst:.3f} of the allowed {factor:g} x bound")
    assert ok, f"{what}: {worst:.3f} of the allowed {factor:g} x bound"
