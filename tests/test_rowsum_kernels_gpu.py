"""The sparse and index-movement kernels at the end of nk_vec.hip -- nk_csr_rowsum, nk_spmv, nk_csr_rowsum_batch (one thread group
per row and the staged short-row kernel), nk_spmv_t, nk_tiled_rowsum, nk_roll, nk_cumsum -- called directly through the C ABI
against the exact sums, the documented order, the long-double references and the DERIVED bounds of tests/rowsum_cases.py
(tests/test_rowsum_cases.py keeps those honest on the host).

Every operand, output and scratch sits between guard bands of all-ones bytes; outputs are prefilled with NaN; after every call the
bands must be intact, the read-only operands bit-identical and no NaN left in an output that should be finite.  Exact data is held to
BITS (any order gives the same sum), ordered data to the bits of the documented order, normal data to the per-row / per-column /
per-element bound.  Every case prints `ERR kernel case dtype lanes variant err bound ratio` (the largest ratio of the case);
profiles/rowsum_kernel_errors.txt keeps one run."""
import ctypes
import os

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from tests import rowsum_cases as rc
from tests.test_fused_transforms_gpu import Guarded, stream

pytestmark = pytest.mark.gpu

LD = rc.LD
NAN = float("nan")
CODE = {np.dtype(np.float64): L.NK_F64, np.dtype(np.float32): L.NK_F32}
DT_IDS = ["f64", "f32"]
W_IDS = ["w", "u"]


def nan_out(shape, dtype=np.float64):
    return Guarded(np.full(shape, NAN, dtype=dtype))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


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


def ptrs(gs):
    return (ctypes.c_void_p * len(gs))(*[None if g is None else g.ptr for g in gs])


def i64s(v):
    return (ctypes.c_int64 * len(v))(*v)


class DeviceCsr:
    """a Csr of rowsum_cases with the weights of one data kind, on the device"""

    def __init__(self, m, kind):
        self.m, self.kind, self.wgt = m, kind, m.weights(kind)
        self.rowptr, self.col = Guarded(m.rowptr), Guarded(m.col)
        self.w = None if self.wgt is None else Guarded(self.wgt)
        self.ins = [self.rowptr, self.col] + ([self.w] if self.w else [])
        self.wptr = self.w.ptr if self.w else None

    def rowsum(self, x, lanes, entry="nk_csr_rowsum"):
        lib, m = L.load(), self.m
        xd, y = x if isinstance(x, Guarded) else Guarded(x), nan_out(m.nrows, (x.arr if isinstance(x, Guarded) else x).dtype)
        code = CODE[xd.arr.dtype]
        if entry == "nk_spmv":
            rcode = lib.nk_spmv(m.nrows, self.rowptr.ptr, self.col.ptr, self.wptr, xd.ptr, y.ptr, code, stream())
        else:
            rcode = lib.nk_csr_rowsum(m.nrows, self.rowptr.ptr, self.col.ptr, self.wptr, xd.ptr, y.ptr, code, lanes, stream())
        L.check(rcode, entry)
        return finite(settle([y], self.ins + [xd])[0])

    def batch(self, xds, lanes):
        lib, m = L.load(), self.m
        ys = [nan_out(m.nrows, xds[0].arr.dtype) for _ in xds]
        L.check(lib.nk_csr_rowsum_batch(m.nrows, self.rowptr.ptr, self.col.ptr, self.wptr, len(xds), ptrs(xds), ptrs(ys),
                                        CODE[xds[0].arr.dtype], lanes, stream()), "nk_csr_rowsum_batch")
        return [finite(a) for a in settle(ys, self.ins + list(xds))]


def check_single(m, lanes, dtype, failures, kernel="nk_csr_rowsum"):
    """the three data kinds on one matrix at one lane count: exact bits, the bits of the documented order, the per-row bound; the
    same bits on a second launch.  Returns {kind: (DeviceCsr, result)}"""
    out = {}
    for kind in rc.KINDS:
        d = DeviceCsr(m, kind)
        x = rc.operand(kind, m.ncols, dtype)
        got = d.rowsum(x, lanes)
        ref, mag = rc.rowsum_ld(m, d.wgt, x)
        w = rc.worst(got, ref, rc.rowsum_bound(m, mag, ref, lanes, dtype))
        rc.record(kernel, m.name, dtype, lanes, f"{'weighted' if m.weighted else 'unweighted'}:{kind}", w)
        if kind == "exact":
            ok = same_bits(got, ref.astype(dtype))
        elif kind == "ordered":
            ok = same_bits(got, rc.rowsum_in_order(m.rowptr, m.col, d.wgt, x, lanes).astype(dtype))
        else:
            ok = w[0] <= 1
        if not ok or w[0] > 1 or not same_bits(got, d.rowsum(x, lanes)):
            failures.append((m.name, lanes, kind, w))
        out[kind] = (d, got)
    return out


# ---- nk_csr_rowsum, nk_spmv ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("weighted", [True, False], ids=W_IDS)
@pytest.mark.parametrize("lanes", rc.LANES)
def test_rowsum_on_the_edge_matrix(lanes, weighted, dtype):
    m = rc.edge_matrix(lanes, weighted)
    failures = []
    res = check_single(m, lanes, dtype, failures)
    if lanes == 64 and weighted:  # nk_spmv is lanes = 64
        for kind, (d, got) in res.items():
            if not same_bits(d.rowsum(rc.operand(kind, m.ncols, dtype), 64, entry="nk_spmv"), got):
                failures.append(("nk_spmv", kind))
    assert not failures, failures


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("weighted", [True, False], ids=W_IDS)
@pytest.mark.parametrize("name", rc.STAGED_NAMES)
def test_rowsum_staged_on_its_window_edges(name, weighted, dtype):
    assert "NK_ROWSUM_STAGED" not in os.environ  # the default: short rows run staged
    failures = []
    check_single(rc.staged_matrix(name, 1, weighted), 1, dtype, failures, kernel="nk_csr_rowsum:staged")
    assert not failures, failures


# ---- nk_csr_rowsum_batch ------------------------------------------------------------------------------------------------------------
def check_batch(m, lanes, dtype, counts, failures):
    for kind in rc.KINDS:
        d = DeviceCsr(m, kind)
        xs = [rc.operand(kind, m.ncols, dtype, seed=k) for k in range(max(counts))]
        assert not any(np.array_equal(xs[0], x) for x in xs[1:])
        xds = [Guarded(x) for x in xs]
        singles = [d.rowsum(xd, lanes) for xd in xds]
        worst = (-1.0,)
        for x, single in zip(xs, singles):
            ref, mag = rc.rowsum_ld(m, d.wgt, x)
            w = rc.worst(single, ref, rc.rowsum_bound(m, mag, ref, lanes, dtype))
            worst = max(worst, w, key=lambda t: t[0])
            if kind == "exact" and not same_bits(single, ref.astype(dtype)):
                failures.append((m.name, lanes, kind, "single not exact"))
        rc.record("nk_csr_rowsum_batch", m.name, dtype, lanes,
                  f"{'weighted' if m.weighted else 'unweighted'}:{kind}:counts={','.join(map(str, counts))}", worst)
        if worst[0] > 1:
            failures.append((m.name, lanes, kind, worst))
        for count in counts:
            got = d.batch(xds[:count], lanes)
            differ = [k for k in range(count) if not same_bits(got[k], singles[k])]
            if differ:
                failures.append((m.name, lanes, kind, count, differ))


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("weighted", [True, False], ids=W_IDS)
@pytest.mark.parametrize("lanes", rc.LANES[1:])
def test_rowsum_batch_members_are_their_single_calls(lanes, weighted, dtype):
    assert rc.BATCH_COUNTS == tuple(range(1, L.MAX_BATCH + 1)) and L.MAX_BATCH == rc.NK_MAX_BATCH
    failures = []
    check_batch(rc.edge_matrix(lanes, weighted), lanes, dtype, rc.BATCH_COUNTS, failures)
    assert not failures, failures


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("weighted", [True, False], ids=W_IDS)
@pytest.mark.parametrize("name", rc.STAGED_NAMES)
def test_rowsum_batch_staged_on_its_window_edges(name, weighted, dtype):
    assert "NK_ROWSUM_STAGED" not in os.environ
    failures = []
    check_batch(rc.staged_matrix(name, 4, weighted), 1, dtype, rc.STAGED_BATCH_COUNTS, failures)
    assert not failures, failures


# ---- nk_spmv_t ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nrows", rc.SPMV_T_ROWS)
def test_spmv_t_adds_onto_its_prefill(nrows, dtype):
    m = rc.spmv_t_matrix(nrows)
    x0 = rc.spmv_t_prefill(nrows)
    untouched = list(rc.SPMV_T_UNTOUCHED)
    failures = []
    for kind in ("exact", "normal"):
        d = DeviceCsr(m, kind)
        y = Guarded(rc.operand(kind, nrows, dtype))
        x64 = Guarded(x0)
        L.check(L.load().nk_spmv_t(nrows, d.rowptr.ptr, d.col.ptr, d.wptr, y.ptr, x64.ptr, CODE[np.dtype(dtype)], stream()), "nk_spmv_t")
        got = finite(settle([x64], d.ins + [y])[0])
        ref, bound, _ = rc.spmv_t_reference(m, d.wgt, y.arr, x0)
        w = rc.worst(got, ref, bound)
        rc.record("nk_spmv_t", m.name, dtype, 64, kind, w)
        if w[0] > 1 or not same_bits(got[untouched], x0[untouched]) or (kind == "exact" and not same_bits(got, ref.astype(np.float64))):
            failures.append((kind, w))
    assert not failures, failures


def test_sparse_refusals_launch_nothing():
    lib, st = L.load(), stream()
    # (the guard of this very test: without the check, a NULL wgt or col below is a device-side null read)
    src = rc.VEC_SRC[rc.VEC_SRC.index('extern "C" int nk_spmv_t'):]
    assert "!col || !wgt" in src[:src.index("hipLaunchKernelGGL")]
    m = rc.spmv_t_matrix(5)
    d = DeviceCsr(m, "normal")
    y, x = Guarded(rc.operand("normal", m.ncols, np.float64)), Guarded(rc.operand("normal", m.ncols, np.float64, seed=1))
    out = nan_out(64)
    f64 = L.NK_F64
    for what, wptr, cptr in (("wgt", None, d.col.ptr), ("col", d.wptr, None)):
        assert lib.nk_spmv_t(m.nrows, d.rowptr.ptr, cptr, wptr, y.ptr, out.ptr, f64, st) == L.NK_ERR_INVALID, what
        assert b"nk_spmv_t" in lib.nk_last_error()
    two = [x, y]
    invalid = {
        "rowsum lanes 0": lambda: lib.nk_csr_rowsum(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, x.ptr, out.ptr, f64, 0, st),
        "rowsum lanes 3": lambda: lib.nk_csr_rowsum(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, x.ptr, out.ptr, f64, 3, st),
        "rowsum lanes 32": lambda: lib.nk_csr_rowsum(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, x.ptr, out.ptr, f64, 32, st),
        "rowsum lanes 128": lambda: lib.nk_csr_rowsum(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, x.ptr, out.ptr, f64, 128, st),
        "rowsum null col": lambda: lib.nk_csr_rowsum(m.nrows, d.rowptr.ptr, None, d.wptr, x.ptr, out.ptr, f64, 4, st),
        "rowsum negative rows": lambda: lib.nk_csr_rowsum(-1, d.rowptr.ptr, d.col.ptr, d.wptr, x.ptr, out.ptr, f64, 4, st),
        "spmv without weights": lambda: lib.nk_spmv(m.nrows, d.rowptr.ptr, d.col.ptr, None, x.ptr, out.ptr, f64, st),
        "spmv_t null x64": lambda: lib.nk_spmv_t(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, y.ptr, None, f64, st),
        "batch lanes 2": lambda: lib.nk_csr_rowsum_batch(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, 2, ptrs(two), ptrs([out, out]), f64, 2, st),
        "batch count 0": lambda: lib.nk_csr_rowsum_batch(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, 0, ptrs(two), ptrs([out, out]), f64, 4, st),
        "batch count 9": lambda: lib.nk_csr_rowsum_batch(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, rc.NK_MAX_BATCH + 1,
                                                         ptrs([x] * 9), ptrs([out] * 9), f64, 4, st),
        "batch null x member": lambda: lib.nk_csr_rowsum_batch(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, 2, ptrs([x, None]),
                                                               ptrs([out, out]), f64, 4, st),
        "batch null y member": lambda: lib.nk_csr_rowsum_batch(m.nrows, d.rowptr.ptr, d.col.ptr, d.wptr, 2, ptrs(two),
                                                               ptrs([out, None]), f64, 4, st),
    }
    assert rc.NK_MAX_BATCH + 1 == 9
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            L.check(call(), name)
    # no rows: NK_OK, nothing read or written (NULL operands are fine then)
    assert lib.nk_csr_rowsum(0, d.rowptr.ptr, None, None, None, out.ptr, f64, 4, st) == L.NK_OK
    assert lib.nk_spmv(0, d.rowptr.ptr, None, None, None, out.ptr, f64, st) == L.NK_OK
    assert lib.nk_spmv_t(0, d.rowptr.ptr, None, None, None, out.ptr, f64, st) == L.NK_OK
    assert lib.nk_csr_rowsum_batch(0, d.rowptr.ptr, None, None, 1, ptrs([None]), ptrs([out]), f64, 1, st) == L.NK_OK
    got = settle([out], d.ins + [x, y])[0]
    assert np.isnan(got).all()


# ---- nk_tiled_rowsum ----------------------------------------------------------------------------------------------------------------
class DeviceTiled:
    _keys = ("item_tile", "item_blk", "blk_slot", "row_slot", "loc", "wgt")

    def __init__(self, plan):
        self.plan = plan
        self.arrays = {k: Guarded(plan[k]) for k in self._keys}
        assert (plan["item_tile"].dtype, plan["item_blk"].dtype, plan["blk_slot"].dtype, plan["row_slot"].dtype, plan["loc"].dtype,
                plan["wgt"].dtype) == (np.int32, np.int64, np.int32, np.int64, np.uint16, np.float32)
        self.c = L.TiledCsr(n_rows=int(plan["n_rows"]), n_slots=int(plan["n_slots"]), n_items=int(plan["n_items"]), ny=int(plan["ny"]),
                            nx=int(plan["nx"]), th=int(plan["th"]), tw=int(plan["tw"]), **{k: self.arrays[k].ptr for k in self._keys})
        self.ins = list(self.arrays.values())

    def call(self, count, xds, ys, scratch, dtype):
        return L.load().nk_tiled_rowsum(ctypes.byref(self.c), count, ptrs(xds), ptrs(ys), scratch.ptr, CODE[np.dtype(dtype)], stream())

    def run(self, xds, dtype):
        """exactly count * n_slots doubles of scratch, between guards"""
        n = int(self.plan["n_rows"])
        ys = [nan_out(n, dtype) for _ in xds]
        scratch = Guarded(nbytes=8 * len(xds) * int(self.plan["n_slots"]))
        L.check(self.call(len(xds), xds, ys, scratch, dtype), "nk_tiled_rowsum")
        return [finite(a) for a in settle(ys + [scratch], self.ins + list(xds))[:len(xds)]]


@pytest.mark.parametrize("shape,tile", [((37,), (None, None)), ((150, 200), (32, 64))], ids=["37", "150x200"])
def test_tiled_rowsum_float32_and_full_batches(shape, tile):
    from nifty_amd import los_response as lr
    from tests.test_los_response import _random_csr

    rng = np.random.default_rng(4)  # the matrix of test_tiled_rowsum_device_equals_its_host_emulation_bit_for_bit
    n = int(np.prod(shape))
    lengths = rng.integers(0, min(n, 2500), size=57)
    lengths[5] = 0
    lengths[11] = min(n, 9000)
    rowptr, col, wgt = _random_csr(rng, len(lengths), n, lengths)
    plan = lr.tiled_plan(rowptr, col, wgt, shape, *tile)
    t = DeviceTiled(plan)
    count = rc.NK_MAX_BATCH
    xs = [rng.normal(size=shape) for _ in range(count)]
    for dtype in rc.DTYPES:
        xds = [Guarded(x.astype(dtype)) for x in xs]
        singles = [t.run([xd], dtype)[0] for xd in xds]
        for k in (0, count - 1):  # the emulation adds in the kernel's order: bits, also after the one rounding of a float32 store
            want = lr.tiled_rowsum_host(plan, xds[k].arr.astype(np.float64)).astype(dtype)
            assert same_bits(singles[k], want), (np.dtype(dtype).name, k)
        full = t.run(xds, dtype)
        assert all(same_bits(a, b) for a, b in zip(full, singles))
    ys = [nan_out(len(lengths)) for _ in range(count + 1)]
    scratch = Guarded(nbytes=8 * (count + 1) * int(plan["n_slots"]))
    x9 = [Guarded(xs[0])] * (count + 1)
    for bad in (0, count + 1):
        with pytest.raises(ValueError):
            L.check(t.call(bad, x9, ys, scratch, np.float64), f"count {bad}")
    assert all(np.isnan(a).all() for a in settle(ys, t.ins + x9[:1]))


# ---- nk_roll ----------------------------------------------------------------------------------------------------------------------
def run_roll(a, shift, ind=None):
    ind = Guarded(a) if ind is None else ind
    out = nan_out(a.shape, a.dtype)
    L.check(L.load().nk_roll(a.ndim, i64s(a.shape), i64s(shift), a.dtype.itemsize, ind.ptr, out.ptr, stream()), "nk_roll")
    return finite(settle([out], [ind])[0])


@pytest.mark.parametrize("shape", rc.ROLL_SHAPES, ids=["x".join(map(str, s)) for s in rc.ROLL_SHAPES])
def test_roll_is_numpy_roll_bit_for_bit(shape):
    failures = []
    for dtype in rc.ROLL_DTYPES:
        a = rc.roll_payload(shape, dtype)
        ind = Guarded(a)
        for shift in rc.roll_shifts(shape):
            got = run_roll(a, shift, ind)
            if not same_bits(got, np.roll(a, shift, axis=tuple(range(a.ndim)))) or not same_bits(got, rc.roll_reference(a, shift)):
                failures.append((np.dtype(dtype).name, shift))
    assert not failures, failures


def test_roll_second_trip_of_the_grid_stride_loop():
    n = rc.ROLL_LONG[0]
    assert n > rc.ROLL_MAX_BLOCKS * rc.ROLL_THREADS and n - rc.ROLL_MAX_BLOCKS * rc.ROLL_THREADS == 777
    a = rc.roll_payload(rc.ROLL_LONG, np.float32)
    ind = Guarded(a)
    for shift in (12345, -(n // 2)):
        assert same_bits(run_roll(a, (shift,), ind), np.roll(a, shift))


def test_roll_refusals_write_nothing():
    lib, st = L.load(), stream()
    a = Guarded(rc.roll_payload((4, 6), np.float64))
    out = nan_out((4, 6))
    s2, z2 = i64s((4, 6)), i64s((1, 2))
    seven = i64s((1,) * 7)
    invalid = {
        "ndim 0": lambda: lib.nk_roll(0, s2, z2, 8, a.ptr, out.ptr, st),
        "ndim 7": lambda: lib.nk_roll(7, seven, seven, 8, a.ptr, out.ptr, st),
        "elem_bytes 2": lambda: lib.nk_roll(2, s2, z2, 2, a.ptr, out.ptr, st),
        "elem_bytes 12": lambda: lib.nk_roll(2, s2, z2, 12, a.ptr, out.ptr, st),
        "negative length": lambda: lib.nk_roll(2, i64s((4, -6)), z2, 8, a.ptr, out.ptr, st),
        "in == out": lambda: lib.nk_roll(2, s2, z2, 8, out.ptr, out.ptr, st),
        "null in": lambda: lib.nk_roll(2, s2, z2, 8, None, out.ptr, st),
        "null out": lambda: lib.nk_roll(2, s2, z2, 8, a.ptr, None, st),
        "null shape": lambda: lib.nk_roll(2, None, z2, 8, a.ptr, out.ptr, st),
        "null shift": lambda: lib.nk_roll(2, s2, None, 8, a.ptr, out.ptr, st),
    }
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            L.check(call(), name)
    assert lib.nk_roll(3, i64s((3, 0, 2)), i64s((1, 1, 1)), 8, a.ptr, out.ptr, st) == L.NK_OK  # a zero-length axis: nothing to move
    assert lib.nk_roll(3, i64s((3, 0, 2)), i64s((1, 1, 1)), 8, None, None, st) == L.NK_OK
    assert np.isnan(settle([out], [a])[0]).all()


# ---- nk_cumsum ------------------------------------------------------------------------------------------------------------------
def run_cumsum(x, reverse, inplace):
    n = len(x)
    if inplace:
        io = Guarded(x)
        L.check(L.load().nk_cumsum(n, io.ptr, io.ptr, reverse, CODE[x.dtype], stream()), "nk_cumsum")
        return settle([io], [])[0]
    ind, out = Guarded(x), nan_out(n, x.dtype)
    L.check(L.load().nk_cumsum(n, ind.ptr, out.ptr, reverse, CODE[x.dtype], stream()), "nk_cumsum")
    return settle([out], [ind])[0]


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", rc.CUMSUM_N)
def test_cumsum_forward_reverse_in_and_out_of_place(n, dtype):
    failures = []
    for reverse in (0, 1):
        xe, xn = rc.cumsum_data("exact", n, dtype), rc.cumsum_data("normal", n, dtype)
        ref, bound = rc.cumsum_reference(xn, reverse, dtype)
        for inplace in (False, True):
            variant = f"{'reverse' if reverse else 'forward'}:{'in_place' if inplace else 'out_of_place'}"
            got = finite(run_cumsum(xe, reverse, inplace))
            if not same_bits(got, rc.cumsum_exact(xe, reverse)):
                failures.append((variant, "exact"))
            w = rc.worst(finite(run_cumsum(xn, reverse, inplace)), ref, bound)
            rc.record("nk_cumsum", f"n={n}", dtype, 64, variant, w)
            if w[0] > 1:
                failures.append((variant, w))
    assert not failures, failures


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [2049, 5000])
def test_cumsum_nan_reaches_only_what_follows_it(n, dtype):
    p = rc.CUMSUM_TILE + 300  # inside the second tile, in the order the kernel walks
    for reverse in (0, 1):
        x = rc.cumsum_data("exact", n, dtype)
        q = n - 1 - p if reverse else p
        clean = rc.cumsum_exact(x, reverse)
        x[q] = NAN
        for inplace in (False, True):
            got = run_cumsum(x, reverse, inplace)
            before, after = (slice(q + 1, n), slice(0, q + 1)) if reverse else (slice(0, q), slice(q, n))
            assert same_bits(got[before], clean[before]) and np.isfinite(got[before]).all() and before.stop > before.start
            assert np.isnan(got[after]).all()


def test_cumsum_refusals_and_the_empty_vector():
    lib, st = L.load(), stream()
    x, out = Guarded(rc.cumsum_data("normal", 64, np.float64)), nan_out(64)
    assert lib.nk_cumsum(0, x.ptr, out.ptr, 0, L.NK_F64, st) == L.NK_OK
    assert lib.nk_cumsum(0, None, None, 1, L.NK_F32, st) == L.NK_OK
    for name, call in {"null in": lambda: lib.nk_cumsum(64, None, out.ptr, 0, L.NK_F64, st),
                       "null out": lambda: lib.nk_cumsum(64, x.ptr, None, 0, L.NK_F64, st),
                       "negative n": lambda: lib.nk_cumsum(-1, x.ptr, out.ptr, 0, L.NK_F64, st)}.items():
        with pytest.raises(ValueError):
            L.check(call(), name)
    assert np.isnan(settle([out], [x])[0]).all()
