"""The bin-map kernels of nk_vec.hip (nk_octant_expand, nk_octant_expand_k2, nk_octant_scatter, nk_octant_scatter_k2,
nk_fold_copies, nk_segment_sum, nk_pindex_from_k2, nk_scatter_add) and the product-spectrum kernels of nk_prod.hip called directly
through the C ABI, against the exact restatements, long-double references and DERIVED bounds of tests/binmap_cases.py
(tests/test_binmap_cases.py keeps those honest on the host).

Every operand, output and scratch sits between guard bands of all-ones bytes; outputs and scratch are prefilled with NaN (the
scratch of nk_octant_scatter_k2 is a slice of exactly the documented 64 * (nb + 32) doubles); after every call the bands must
be intact, the read-only operands bit-identical and no NaN in an output that should be finite.  Gathers, the fixed-point
scatter, nk_fold_copies and nk_segment_sum are held to BITS; the floating-point sums to their per-bin bounds.  Every case prints
`ERR kernel shape dtype variant err bound ratio` (the largest ratio of the case); profiles/r11_binmap_errors.txt keeps one run."""
import ctypes

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from tests import binmap_cases as bc
from tests.test_fused_transforms_gpu import Guarded, stream

pytestmark = pytest.mark.gpu

LD = bc.LD
NAN = float("nan")
DTYPES = [np.float64, np.float32]
CODE = {np.dtype(np.float64): L.NK_F64, np.dtype(np.float32): L.NK_F32}


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def shp(shape):
    return (ctypes.c_int64 * len(shape))(*shape)


def nan_out(n, dtype=np.float64):
    return Guarded(np.full(n, NAN, dtype=dtype))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def settle(outputs, inputs):
    """after a call: bands intact, operands untouched; returns the outputs' contents"""
    torch.cuda.synchronize()
    for g in list(outputs) + list(inputs):
        assert g.guards_intact()
    for g in inputs:
        assert g.unchanged()
    return [g.get() if g.arr is not None else None for g in outputs]


def finite(a):
    assert not np.isnan(a).any(), f"{int(np.isnan(a).sum())} entries unwritten or NaN"
    return a


# ---- nk_octant_scatter_k2 -----------------------------------------------------------------------------------------------------
class ShellDevice:
    def __init__(self, geo):
        self.geo, self.lib = geo, L.load()
        self.pidx, self.k2 = Guarded(geo.pidx), Guarded(geo.bin_k2)

    def run(self, w8, wmax, launches=1):
        geo = self.geo
        w8d = Guarded(w8)
        ins = [self.pidx, self.k2, w8d]
        wm = None
        if wmax is not None:
            wm = Guarded(np.array([wmax], dtype=np.float64))
            ins.append(wm)
        got = []
        for _ in range(launches):
            scratch, abar = Guarded(nbytes=8 * geo.scratch_doubles()), nan_out(geo.nb)
            L.check(self.lib.nk_octant_scatter_k2(geo.ndim, shp(geo.shape), w8d.ptr, self.pidx.ptr, self.k2.ptr, geo.nb, scratch.ptr,
                                                  abar.ptr, wm.ptr if wm else None, stream()), "nk_octant_scatter_k2")
            got.append(settle([abar, scratch], ins)[0])
        return got


@pytest.mark.parametrize("shape", list(bc.SHELL_SHAPES), ids=ids(bc.SHELL_SHAPES))
def test_shell_scatter_fixed_point_is_the_exact_restatement(shape):
    geo = bc.geometry(shape)
    assert (geo.nb, geo.shells) == bc.SHELL_SHAPES[shape]
    dev = ShellDevice(geo)
    failures = []
    for name, w8, wmax, _ in bc.scatter_datasets(geo):
        want, partial, e = bc.fixed_point_scatter(geo, w8, wmax)
        got = dev.run(w8, wmax, launches=3)
        finite(got[0])
        ref, _ = bc.shell_reference(geo, w8)
        w = bc.worst(got[0], ref, bc.fixed_bound(geo, partial, e))
        bc.record("nk_octant_scatter_k2", shape, "f64", "fixed:" + name, w)
        differ = int(np.count_nonzero(bits(got[0]) != bits(want)))
        print(f"BITS nk_octant_scatter_k2 {'x'.join(map(str, shape))} fixed:{name} e={e} bins_differing={differ}")
        if differ or w[0] > 1 or not all(np.array_equal(bits(g), bits(got[0])) for g in got[1:]):
            failures.append((name, differ, w))
    assert not failures, failures


@pytest.mark.parametrize("shape", list(bc.SHELL_SHAPES), ids=ids(bc.SHELL_SHAPES))
def test_shell_scatter_floating_point_within_the_per_bin_bound(shape):
    geo = bc.geometry(shape)
    assert (geo.nb, geo.shells) == bc.SHELL_SHAPES[shape]
    dev = ShellDevice(geo)
    failures = []
    for name, w8, _, fixed_only in bc.scatter_datasets(geo):
        if fixed_only:  # the same data as an earlier set
            continue
        got = finite(dev.run(w8, None)[0])
        ref, mag = bc.shell_reference(geo, w8)
        w = bc.worst(got, ref, bc.float_shell_bound(geo, mag))
        bc.record("nk_octant_scatter_k2", shape, "f64", "float:" + name, w)
        if w[0] > 1:
            failures.append((name, w))
    assert not failures, failures


def test_shell_scatter_answers_zero_and_non_finite_maxima():
    geo = bc.geometry((16, 16, 256))
    dev = ShellDevice(geo)
    w8 = bc.scatter_datasets(geo)[0][1]
    assert not dev.run(np.zeros(geo.oshape), 0.0)[0].any()
    for wmax in (np.inf, np.nan):
        assert np.isnan(dev.run(w8, wmax)[0]).all()


# ---- nk_octant_scatter --------------------------------------------------------------------------------------------------------
def run_atomic_scatter(geo, pidx, w8, abar0, flag):
    p, w, abar = Guarded(pidx), Guarded(w8), Guarded(abar0)
    L.check(L.load().nk_octant_scatter(geo.ndim, shp(geo.shape), w.ptr, p.ptr, abar.ptr, flag, stream()), "nk_octant_scatter")
    return finite(settle([abar], [p, w])[0])


ATOMIC_CASES = [(s, 0, "index") for s in bc.SCATTER_SHAPES] + [((8, 8, 12), 1, "index"), ((64, 64, 64), 1, "index"),
                                                               ((4, 6, 10), 1, "index"), ((8, 8, 12), 0, "asymmetric")]


@pytest.mark.parametrize("shape,flag,index", ATOMIC_CASES, ids=[f"{'x'.join(map(str, s))}-merge{f}-{i}" for s, f, i in ATOMIC_CASES])
def test_octant_scatter_accumulates_into_abar(shape, flag, index):
    geo = bc.geometry(shape)
    rng = np.random.default_rng([31, flag, *shape])
    if index == "asymmetric":  # any index is legal without the merge: nothing may assume the swap symmetry
        nb = 37
        pidx = rng.integers(0, nb, size=shape).astype(np.int32)
        assert not np.array_equal(pidx[:5, :5], pidx[:5, :5].transpose(1, 0, 2))
    else:
        nb, pidx = geo.nb, geo.pidx
        if flag and shape[0] == shape[1]:
            assert np.array_equal(geo.pidx8, geo.pidx8.transpose(1, 0, 2))
    w8 = rng.normal(size=geo.oshape) * 10.0 ** rng.uniform(-4, 4, size=geo.oshape)
    abar0 = rng.normal(size=nb) * 100.0
    honoured = bool(flag) and geo.ndim == 3 and shape[0] == shape[1]  # the launcher ignores the flag otherwise
    assert honoured == (flag == 1 and shape != (4, 6, 10))
    got = run_atomic_scatter(geo, pidx, w8, abar0, flag)
    ref, bound = bc.atomic_scatter_reference(geo, pidx, w8, abar0, honoured, nb)
    w = bc.worst(got, ref, bound)
    bc.record("nk_octant_scatter", shape, "f64", f"merge={flag}:{index}", w)
    assert w[0] <= 1, w
    if flag and not honoured:  # equal to the unmerged scatter: the same reference, the same bound
        assert bc.worst(run_atomic_scatter(geo, pidx, w8, abar0, 0), ref, bound)[0] <= 1


# ---- expansions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", bc.SCATTER_SHAPES, ids=ids(bc.SCATTER_SHAPES))
def test_octant_expand_is_the_gather(shape, dtype):
    geo = bc.geometry(shape)
    table = np.random.default_rng([37, *shape]).normal(size=geo.nb).astype(dtype)
    t, p = Guarded(table), Guarded(geo.pidx)
    for compact, want in ((0, table[geo.pidx]), (1, table[geo.pidx8])):
        out = nan_out(want.shape, dtype)
        L.check(L.load().nk_octant_expand(geo.ndim, shp(shape), t.ptr, p.ptr, out.ptr, CODE[np.dtype(dtype)], compact, stream()),
                "nk_octant_expand")
        got = finite(settle([out], [t, p])[0])  # no NaN left: every element was written
        differ = int(np.count_nonzero(bits(got) != bits(want)))
        print(f"BITS nk_octant_expand {'x'.join(map(str, shape))} {np.dtype(dtype).name} compact={compact} threads="
              f"{256 if geo.Ch >= 256 else 64} differing={differ}")
        assert differ == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "line_order"])
@pytest.mark.parametrize("shape", bc.EXPAND_K2_SHAPES, ids=ids(bc.EXPAND_K2_SHAPES))
def test_octant_expand_k2_is_the_gather(shape, ordered, dtype):
    geo = bc.geometry(shape)
    table = np.random.default_rng([41, *shape]).normal(size=geo.nb)  # fp64, as the amplitude kernels produce it
    t, k2 = Guarded(table), Guarded(geo.bin_k2)
    order = Guarded(geo.line_order()) if ordered else None
    ins = [t, k2] + ([order] if ordered else [])
    dense = nan_out(int(geo.bin_k2[-1]) + 1, dtype)  # exactly max k^2 + 1 elements
    out = nan_out(geo.oshape, dtype)
    L.check(L.load().nk_octant_expand_k2(geo.ndim, shp(shape), t.ptr, k2.ptr, geo.nb, dense.ptr, out.ptr, CODE[np.dtype(dtype)],
                                         order.ptr if ordered else None, stream()), "nk_octant_expand_k2")
    got, spread = settle([out, dense], ins)
    want = table.astype(dtype)[geo.pidx8]
    differ = int(np.count_nonzero(bits(finite(got)) != bits(want)))
    print(f"BITS nk_octant_expand_k2 {'x'.join(map(str, shape))} {np.dtype(dtype).name} ordered={ordered} differing={differ}")
    assert differ == 0
    assert np.array_equal(bits(spread[geo.bin_k2]), bits(table.astype(dtype)))


# ---- exact orders -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, 16])
@pytest.mark.parametrize("n", [1, 31, 4097])
def test_fold_copies_adds_in_copy_order(n, copies):
    src, n, copies, stride = bc.fold_data(n, copies)
    assert stride > n
    s, out = Guarded(src), nan_out(n)
    L.check(L.load().nk_fold_copies(n, copies, stride, s.ptr, out.ptr, stream()), "nk_fold_copies")
    got = finite(settle([out], [s])[0])
    assert np.array_equal(bits(got), bits(bc.fold_copies_host(src, n, copies, stride)))


@pytest.mark.parametrize("accumulate", [0, 1])
def test_segment_sum_adds_in_perm_order(accumulate):
    rowptr, perm, src = bc.segment_data()
    nseg = len(rowptr) - 1
    assert 5000 in np.diff(rowptr) and 0 in np.diff(rowptr) and nseg > 256
    dst0 = np.random.default_rng(43).normal(size=nseg) if accumulate else np.full(nseg, NAN)
    r, p, s, dst = Guarded(rowptr), Guarded(perm), Guarded(src), Guarded(dst0)
    L.check(L.load().nk_segment_sum(nseg, r.ptr, p.ptr, s.ptr, dst.ptr, accumulate, stream()), "nk_segment_sum")
    got = finite(settle([dst], [r, p, s])[0])
    want = bc.segment_sum_host(rowptr, perm, src, dst0, accumulate)
    assert np.array_equal(bits(got), bits(want))
    assert not want[np.diff(rowptr) == 0].any() or accumulate  # an empty segment is 0.0, or dst + 0.0


@pytest.mark.parametrize("shape", bc.PINDEX_SHAPES, ids=ids(bc.PINDEX_SHAPES))
def test_pindex_from_k2_with_rho(shape):
    geo = bc.geometry(shape)
    table = Guarded(geo.k2table)
    pidx = Guarded(np.full(shape, -7, dtype=np.int32))
    rho = Guarded(np.zeros(geo.nb, dtype=np.int64))
    L.check(L.load().nk_pindex_from_k2(geo.ndim, shp(shape), table.ptr, pidx.ptr, rho.ptr, stream()), "nk_pindex_from_k2")
    got_p, got_r = settle([pidx, rho], [table])
    assert np.array_equal(got_p, geo.pidx) and np.array_equal(got_r, geo.rho) and got_r.sum() == int(np.prod(shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (4099, 0), (4099, 1)], ids=["1", "3", "4099", "4099-unaligned"])
def test_scatter_add_within_the_atomic_bound(n, offset, dtype):
    rng = np.random.default_rng([47, n])
    nb = 1 if n == 1 else 13
    values = (rng.normal(size=n + offset) * 10.0 ** rng.uniform(-3, 3, size=n + offset)).astype(dtype)
    pidx = rng.integers(0, nb, size=n).astype(np.int32)
    v, p, out = Guarded(values), Guarded(pidx), Guarded(np.zeros(nb))
    vptr = v.ptr + offset * np.dtype(dtype).itemsize  # a view one element in: not 16-byte aligned
    assert (vptr % 16 != 0) == bool(offset)
    L.check(L.load().nk_scatter_add(n, vptr, p.ptr, nb, out.ptr, CODE[np.dtype(dtype)], stream()), "nk_scatter_add")
    got = finite(settle([out], [v, p])[0])
    ref, bound = bc.scatter_add_reference(pidx, values[offset:], nb)
    w = bc.worst(got, ref, bound)
    bc.record("nk_scatter_add", (n,), np.dtype(dtype).name, f"offset={offset}", w)
    assert w[0] <= 1, w


# ---- nk_prod.hip ----------------------------------------------------------------------------------------------------------------
PRODUCT_CASES = [(s, None, False) for s in bc.PRODUCT_SIZES] + [((5, 255, 63), 1, False), ((128, 255), 0, True), ((600,), 0, True)]


@pytest.mark.parametrize("sizes,null_dtab,null_dscale", PRODUCT_CASES,
                         ids=[f"{'x'.join(map(str, s))}-dtab{d}-dscale{int(not n)}" for s, d, n in PRODUCT_CASES])
def test_product_field_tangent_and_marginals(sizes, null_dtab, null_dscale):
    lib = L.load()
    pc = bc.ProductCase(sizes, null_dtab, null_dscale)
    held = {"pidx": [Guarded(p) for p in pc.pidx], "tab": [Guarded(t) for t in pc.tab],
            "dtab": [None if t is None else Guarded(t) for t in pc.dtab], "scale": Guarded(np.array([pc.scale])),
            "dscale": None if pc.dscale is None else Guarded(np.array([pc.dscale])), "w": Guarded(pc.w)}
    ins = held["pidx"] + held["tab"] + [g for g in held["dtab"] if g] + [held["scale"], held["w"]] + ([held["dscale"]] if held["dscale"] else [])
    q = L.Product()
    q.nsub = pc.nsub
    for i in range(pc.nsub):
        q.size[i], q.pidx[i], q.tab[i] = sizes[i], held["pidx"][i].ptr, held["tab"][i].ptr
        q.dtab[i] = held["dtab"][i].ptr if held["dtab"][i] else None
    q.scale, q.dscale = held["scale"].ptr, held["dscale"].ptr if held["dscale"] else None
    failures = []
    for tangent in (0, 1):
        ref, b64 = pc.field(tangent)
        for dtype in DTYPES:
            out = nan_out(pc.n, dtype)
            L.check(lib.nk_product_field(ctypes.byref(q), tangent, out.ptr, CODE[np.dtype(dtype)], stream()), "nk_product_field")
            got = finite(settle([out], ins)[0])
            w = bc.worst(got, ref, b64 + bc.store_rounding(ref, dtype))
            bc.record("nk_product_field", sizes, np.dtype(dtype).name, f"tangent={tangent}:dtab{null_dtab}:dscale{int(not null_dscale)}", w)
            if w[0] > 1:
                failures.append(("field", tangent, dtype, w))
    for which in range(pc.nsub):
        A, Bn, C = pc.abc(which)
        nbytes = int(lib.nk_product_marginal_scratch(ctypes.byref(q), which))
        assert nbytes == 8 * (A * Bn + -(-A // bc.MARG_ROWS) * Bn)
        got = []
        for _ in range(2):
            scratch, marg = Guarded(nbytes=nbytes), nan_out(Bn)
            L.check(lib.nk_product_marginal(ctypes.byref(q), which, held["w"].ptr, scratch.ptr, marg.ptr, stream()), "nk_product_marginal")
            got.append(finite(settle([marg, scratch], ins)[0]))
        ref, bound = pc.marginal(which)
        w = bc.worst(got[0], ref, bound)
        bc.record("nk_product_marginal", sizes, "f64", f"which={which}:A={A}:Bn={Bn}:C={C}", w)
        if w[0] > 1 or not np.array_equal(bits(got[0]), bits(got[1])):
            failures.append(("marginal", which, w))
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", bc.MIRROR_SHAPES, ids=ids(bc.MIRROR_SHAPES))
def test_mirror_combine_against_the_direct_sum(shape, dtype):
    rng = np.random.default_rng([53, *shape])
    x = rng.normal(size=shape).astype(dtype)
    xin = Guarded(x)
    scale, offset = -1.75, 0.3125
    best = (-1.0,)
    for nsub, group in bc.mirror_groupings(len(shape)):
        coef = rng.normal(size=1 << nsub)
        out = nan_out(shape, dtype)
        L.check(L.load().nk_mirror_combine(len(shape), shp(shape), (ctypes.c_int * len(shape))(*group), nsub,
                                           (ctypes.c_double * len(coef))(*coef), xin.ptr, out.ptr, scale, offset,
                                           CODE[np.dtype(dtype)], stream()), "nk_mirror_combine")
        got = finite(settle([out], [xin])[0])
        w = bc.worst(got, *bc.mirror_reference(x, group, nsub, coef, scale, offset, dtype))
        assert w[0] <= 1, (nsub, group, w)
        best = max(best, w, key=lambda t: t[0])
    bc.record("nk_mirror_combine", shape, np.dtype(dtype).name, f"groupings={len(bc.mirror_groupings(len(shape)))}", best)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib = L.load()
    assert (L.NK_ERR_INVALID, L.NK_ERR_UNSUPPORTED) == (-1, -2)
    header = open(bc.os.path.join(bc.ROOT, "include", "niftyk.h")).read()
    assert "NK_ERR_INVALID = -1," in header and "NK_ERR_UNSUPPORTED = -2," in header
    d = Guarded(np.zeros(64))           # stands in for every array: a refused call touches none of them
    i = Guarded(np.zeros(64, dtype=np.int32))
    s1, s3 = shp((4,)), shp((4, 4, 4))
    four = shp((2, 2, 2, 2))
    st = stream()
    invalid = {
        "expand ndim 0": lambda: lib.nk_octant_expand(0, s1, d.ptr, i.ptr, d.ptr, L.NK_F64, 0, st),
        "expand ndim 4": lambda: lib.nk_octant_expand(4, four, d.ptr, i.ptr, d.ptr, L.NK_F64, 0, st),
        "expand null table": lambda: lib.nk_octant_expand(1, s1, None, i.ptr, d.ptr, L.NK_F64, 0, st),
        "expand null field": lambda: lib.nk_octant_expand(1, s1, d.ptr, i.ptr, None, L.NK_F64, 0, st),
        "expand null shape": lambda: lib.nk_octant_expand(1, None, d.ptr, i.ptr, d.ptr, L.NK_F64, 0, st),
        "scatter ndim 0": lambda: lib.nk_octant_scatter(0, s1, d.ptr, i.ptr, d.ptr, 0, st),
        "scatter ndim 4": lambda: lib.nk_octant_scatter(4, four, d.ptr, i.ptr, d.ptr, 0, st),
        "scatter null pidx": lambda: lib.nk_octant_scatter(1, s1, d.ptr, None, d.ptr, 0, st),
        "scatter null abar": lambda: lib.nk_octant_scatter(1, s1, d.ptr, i.ptr, None, 0, st),
        "expand_k2 ndim 4": lambda: lib.nk_octant_expand_k2(4, four, d.ptr, i.ptr, 3, d.ptr, d.ptr, L.NK_F64, None, st),
        "expand_k2 nb 0": lambda: lib.nk_octant_expand_k2(1, s1, d.ptr, i.ptr, 0, d.ptr, d.ptr, L.NK_F64, None, st),
        "expand_k2 null dense": lambda: lib.nk_octant_expand_k2(1, s1, d.ptr, i.ptr, 3, None, d.ptr, L.NK_F64, None, st),
        "scatter_k2 ndim 0": lambda: lib.nk_octant_scatter_k2(0, s1, d.ptr, i.ptr, i.ptr, 3, d.ptr, d.ptr, None, st),
        "scatter_k2 ndim 4": lambda: lib.nk_octant_scatter_k2(4, four, d.ptr, i.ptr, i.ptr, 3, d.ptr, d.ptr, None, st),
        "scatter_k2 nb 0": lambda: lib.nk_octant_scatter_k2(1, s1, d.ptr, i.ptr, i.ptr, 0, d.ptr, d.ptr, None, st),
        "scatter_k2 null scratch": lambda: lib.nk_octant_scatter_k2(1, s1, d.ptr, i.ptr, i.ptr, 3, None, d.ptr, None, st),
        "scatter_k2 null bin_k2": lambda: lib.nk_octant_scatter_k2(1, s1, d.ptr, i.ptr, None, 3, d.ptr, d.ptr, None, st),
        "pindex ndim 0": lambda: lib.nk_pindex_from_k2(0, s1, i.ptr, i.ptr, None, st),
        "pindex ndim 4": lambda: lib.nk_pindex_from_k2(4, four, i.ptr, i.ptr, None, st),
        "pindex null table": lambda: lib.nk_pindex_from_k2(1, s1, None, i.ptr, None, st),
        "fold copies 0": lambda: lib.nk_fold_copies(4, 0, 8, d.ptr, d.ptr, st),
        "fold null src": lambda: lib.nk_fold_copies(4, 1, 8, None, d.ptr, st),
        "segment null perm": lambda: lib.nk_segment_sum(2, i.ptr, None, d.ptr, d.ptr, 0, st),
        "scatter_add nbins 0": lambda: lib.nk_scatter_add(4, d.ptr, i.ptr, 0, d.ptr, L.NK_F64, st),
        "scatter_add null bins": lambda: lib.nk_scatter_add(4, d.ptr, i.ptr, 3, None, L.NK_F64, st),
    }
    grp = (ctypes.c_int * 3)(0, 0, 0)
    coef = (ctypes.c_double * 8)(*[1.0] * 8)
    out = Guarded(np.zeros(64))
    invalid.update({
        "mirror in place": lambda: lib.nk_mirror_combine(3, s3, grp, 1, coef, d.ptr, d.ptr, 1.0, 0.0, L.NK_F64, st),
        "mirror nsub 0": lambda: lib.nk_mirror_combine(3, s3, grp, 0, coef, d.ptr, out.ptr, 1.0, 0.0, L.NK_F64, st),
        "mirror nsub 4": lambda: lib.nk_mirror_combine(3, s3, grp, 4, coef, d.ptr, out.ptr, 1.0, 0.0, L.NK_F64, st),
        "mirror ndim 0": lambda: lib.nk_mirror_combine(0, s3, grp, 1, coef, d.ptr, out.ptr, 1.0, 0.0, L.NK_F64, st),
        "mirror ndim 4": lambda: lib.nk_mirror_combine(4, four, grp, 1, coef, d.ptr, out.ptr, 1.0, 0.0, L.NK_F64, st),
        "mirror null coef": lambda: lib.nk_mirror_combine(3, s3, grp, 1, None, d.ptr, out.ptr, 1.0, 0.0, L.NK_F64, st),
    })

    def product(nsub, scale=True, pidx=True):
        q = L.Product()
        q.nsub = nsub
        for k in range(3):
            q.size[k], q.pidx[k], q.tab[k] = 4, i.ptr if pidx else None, d.ptr
        q.scale = d.ptr if scale else None
        return q

    for nsub in (0, 4):
        invalid[f"product field nsub {nsub}"] = lambda n=nsub: lib.nk_product_field(ctypes.byref(product(n)), 0, out.ptr, L.NK_F64, st)
        invalid[f"product marginal nsub {nsub}"] = lambda n=nsub: lib.nk_product_marginal(ctypes.byref(product(n)), 0, d.ptr, out.ptr, out.ptr, st)
    invalid["product null scale"] = lambda: lib.nk_product_field(ctypes.byref(product(2, scale=False)), 0, out.ptr, L.NK_F64, st)
    invalid["product null pidx"] = lambda: lib.nk_product_field(ctypes.byref(product(2, pidx=False)), 0, out.ptr, L.NK_F64, st)
    invalid["product null out"] = lambda: lib.nk_product_field(ctypes.byref(product(2)), 0, None, L.NK_F64, st)
    invalid["marginal which 2 of 2"] = lambda: lib.nk_product_marginal(ctypes.byref(product(2)), 2, d.ptr, out.ptr, out.ptr, st)
    invalid["marginal null w"] = lambda: lib.nk_product_marginal(ctypes.byref(product(2)), 0, None, out.ptr, out.ptr, st)
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            L.check(call(), name)
    assert lib.nk_product_marginal_scratch(ctypes.byref(product(0)), 0) == 0
    # (Ch - 1)^2 = 2^24 at (8192,): the integer square roots are exact below that only
    big = shp((8192,))
    unsupported = {
        "scatter_k2 k^2 range": lambda: lib.nk_octant_scatter_k2(1, big, d.ptr, i.ptr, i.ptr, 3, d.ptr, out.ptr, None, st),
        "expand_k2 k^2 range": lambda: lib.nk_octant_expand_k2(1, big, d.ptr, i.ptr, 3, d.ptr, out.ptr, L.NK_F64, None, st),
    }
    for name, call in unsupported.items():
        with pytest.raises(NotImplementedError):
            L.check(call(), name)
    torch.cuda.synchronize()
    assert all(g.guards_intact() and g.unchanged() for g in (d, i, out))
