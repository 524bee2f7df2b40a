"""Element-wise, reduction and complex kernels of nk_vec.hip against exact or high-precision references, at every code path
the launcher picks (nk_launch_map): the flat one-vector-per-thread maps, the block-cyclic chunks with their unrolled and
partial chunks, the unaligned scalar map, the scalar tail after the vectors, the 64-unit reduction layout, both sides of the
512-workgroup switch of nk_grid_red and the batched launches that fall back to single launches.

Every device output is written into the middle of a larger buffer filled with a NaN sentinel; the guard elements around it
must survive.  The reference helpers (exact sums, TwoProduct, the launch-length table) have host tests of their own at the
end of the file, so that a wrong reference cannot make a GPU test pass."""
import ctypes
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nifty_amd", "csrc")

# ---- launch geometry of nk_vec.hip (checked against the source by test_launch_constants_match_the_source) ---------------
THREADS = 256        # NK_VEC_THREADS
MAX_BLOCKS = 2048    # NK_MAX_BLOCKS
RED_UNITS = 64       # NK_RED_UNITS (nk_util.h)
UNIT_GRID = 64       # default NK_RED_UNIT_GRID
VW = {np.float32: 4, np.float64: 2}  # 16-byte vector width in elements (VecOf<T>::N)
NPT = {np.float32: torch.float32, np.float64: torch.float64}
CODE = {np.float32: 0, np.float64: 1}  # NK_F32 / NK_F64
INT = {np.float32: np.int32, np.float64: np.int64}
DTYPES = [np.float32, np.float64]


def last_chunked(v):
    """largest aligned length whose map still runs as block-cyclic chunks: pieces = ceil(nvec / 256) <= NK_MAX_BLOCKS"""
    return MAX_BLOCKS * THREADS * v


def first_flat(v):
    """smallest aligned length that goes to k_map_flat (one more whole vector than last_chunked)"""
    return last_chunked(v) + v


def map_lengths(v):
    """the lengths of the launch-path matrix: tiny, one vector plus tail, around one and many 256-vector rows, and the
    chunked / flat boundary (last chunked, first flat, flat with the longest scalar tail)"""
    return [1, 2, 3, v + 1, 255, 257, 256 * v - 1, 256 * v + 1, 4096 * v + 1,
            last_chunked(v), first_flat(v), first_flat(v) + v - 1]


def grid_red(nvec):
    """nk_grid_red: >= 32 vectors per thread up to 512 workgroups, >= 64 beyond"""
    b = -(-nvec // (32 * THREADS))
    if b > 512:
        b = max(512, -(-nvec // (64 * THREADS)))
    return min(max(b, 1), MAX_BLOCKS)


def red_unit(n, v):
    """nk_red_unit_of: the unit length of the 64-unit layout, 0 when the array is one unit"""
    row = v * THREADS
    if n <= 0 or n % (RED_UNITS * row) != 0 or n // (RED_UNITS * row) < 2:
        return 0
    return n // RED_UNITS


def red_grid(n, v, aligned):
    """the grid nk_launch_map gives a reduction of n elements"""
    if not aligned:
        return grid_red(n)
    unit = red_unit(n, v)
    if unit:
        return RED_UNITS * min(grid_red(unit // v), UNIT_GRID)
    return grid_red(n // v)


def red_depth(n, v, aligned):
    """Longest chain of fp64 additions from one term to the result in nk_map_body, for the error bound of the sums.

    A thread adds its terms in order: the block-cyclic chunks give it at most 2 * ceil(n / (grid * 256)) elements (the chunk
    length rounds the share down, the chunk count up), plus one vector of slack and the scalar tail.  Then: the wave shuffle
    tree (6 levels), the sum of the 4 wave partials in LDS (4 additions, it starts from 0), the lanes that stride the
    workgroup partials of a unit (ceil(G / 64)) and their shuffle tree (6), the sequential sum over the units (<= 64) and
    the update of the result (accumulate).  Every addition rounds once, so with h such additions
        |computed - exact| <= gamma_h * sum |term|,   gamma_h = h u / (1 - h u),  u = 2^-53,
    (Higham, Accuracy and Stability, 4.2), and the products of an fp64 dot add one rounding (u |x y|) each."""
    grid = red_grid(n, v, aligned)
    per_thread = 2 * -(-n // (grid * THREADS)) + 2 * v
    return per_thread + 6 + 4 + -(-grid // 64) + 6 + RED_UNITS + 2


def sum_bound(n, v, aligned, abs_terms_sum, product=False):
    u = 2.0 ** -53
    h = red_depth(n, v, aligned) + (1 if product else 0)
    return h * u / (1 - h * u) * abs_terms_sum * 1.0001


# ---- exact references -----------------------------------------------------------------------------------------------------
def split(a):
    """Veltkamp split of fp64 values: hi + lo == a, both with at most 26 significant bits"""
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """Dekker's TwoProduct: p + e == a * b exactly (fp64 arrays, no overflow / underflow of the partial products)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_dot(x, y):
    """sum(x * y) correctly rounded to fp64: fp32 products are exact in fp64, fp64 products are split exactly"""
    if x.dtype == np.float32:
        return math.fsum((x.astype(np.float64) * y.astype(np.float64)).tolist())
    p, e = two_product(x, y)
    return math.fsum(p.tolist() + e.tolist())


def ulps(got, ref, dt):
    """|got - ref| in ulps of dt at |ref| (ref in fp64 or better; ulp of a zero reference = the smallest subnormal)"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    sp = np.spacing(np.abs(ref).astype(dt)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(got - ref) / sp


def same_bits(got, exp):
    """bitwise equal, except that a NaN may come with any payload"""
    it = INT[exp.dtype.type]
    nan = np.isnan(exp)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(it), exp[~nan].view(it)))


# ---- guarded device buffers -------------------------------------------------------------------------------------------------
GUARD = 64  # elements on either side (a multiple of 16 bytes: offset 0 is 16-byte aligned)
SENTINEL = {np.float32: 0x7FC5A5A5, np.float64: 0x7FF8A5A5A5A5A5A5, np.int32: -0x5A5A5A5B}


class Guarded:
    """n elements at element offset `off` inside a larger device buffer whose other elements hold a NaN sentinel"""

    def __init__(self, dt, n, off, host=None):
        self.dt, self.n, self.lo = dt, n, GUARD + off
        idt = {np.float32: torch.int32, np.float64: torch.int64, np.int32: torch.int32}[dt]
        raw = torch.full((GUARD + off + n + GUARD,), SENTINEL[dt], dtype=idt, device="cuda")
        self.buf = raw if dt == np.int32 else raw.view(NPT[dt])
        if host is not None:
            self.buf[self.lo:self.lo + n].copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=dt)))

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def get(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def guards_intact(self):
        bits = self.buf.view(torch.int32 if self.buf.element_size() == 4 else torch.int64).cpu().numpy()
        s = np.array(SENTINEL[self.dt]).astype(bits.dtype)
        return bool(np.all(bits[:self.lo] == s) and np.all(bits[self.lo + self.n:] == s))


def lib():
    from nifty_amd import _lib

    return _lib.load()


def stream():
    from nifty_amd import backend as B

    return B._stream()


def check(rc, what):
    from nifty_amd import _lib

    _lib.check(rc, what)


def offset_patterns(k, dt):
    """element offsets of k operands: all aligned, all shifted alike, and each operand alone at offset 1"""
    pats = [(0,) * k, (1,) * k] + ([(2,) * k, (3,) * k] if dt == np.float32 else [])
    pats += [tuple(1 if j == i else 0 for j in range(k)) for i in range(k)]
    return list(dict.fromkeys(pats))


def patterns_for(n, k, dt):
    """the full pattern set up to 64K elements, all-aligned and all-shifted beyond (the longest lengths cost host time)"""
    return offset_patterns(k, dt) if n <= 1 << 16 else [(0,) * k, (1,) * k]


def rand(rng, dt, n, kind="normal"):
    if kind == "int":
        return rng.integers(-8, 9, size=n).astype(dt)
    return rng.standard_normal(n).astype(dt)


def with_subnormals(x, dt):
    """a few subnormal operands (and their negatives) spread over x"""
    x = x.copy()
    tiny = np.finfo(dt).tiny
    sub = np.array([tiny / 2, tiny / 3, -tiny / 7, tiny * 2.0 ** -10, np.finfo(dt).smallest_subnormal], dtype=dt)
    idx = np.arange(0, len(x), 7)[:len(sub) * 4]
    x[idx] = np.resize(sub, len(idx))
    return x


# ============================================ A. maps without reductions ====================================================
def _binary_cases(dt):
    s1, s2 = dt(0.1), dt(-3.0)
    for op in range(4):
        yield op, "tt", None
        yield op, "ts", float(s1)
        yield op, "st", float(s2)


NP_OP = [np.add, np.subtract, np.multiply, np.divide]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_binary_all_paths_bit_exact(dt):
    """+ - * / in T are one IEEE operation: bit for bit equal to numpy in T, at every length, offset and path -- with
    subnormal operands, which the device neither flushes on input nor on output (asserted, not assumed)"""
    rng = np.random.default_rng(1)
    v = VW[dt]
    for n in map_lengths(v):
        a = with_subnormals(rand(rng, dt, n), dt)
        b = with_subnormals(rand(rng, dt, n), dt) + dt(0.5)
        b[b == 0] = dt(1)
        for op, mode, s in _binary_cases(dt):
            for oa, ob, oo in patterns_for(n, 3, dt):
                A = Guarded(dt, n, oa, a) if mode != "st" else None
                Bb = Guarded(dt, n, ob, b) if mode != "ts" else None
                O = Guarded(dt, n, oo)
                check(lib().nk_binary(op, n, A.ptr if A else None, s if mode == "st" else 0.0, Bb.ptr if Bb else None,
                                      s if mode == "ts" else 0.0, O.ptr, CODE[dt], stream()), "nk_binary")
                with np.errstate(all="ignore"):
                    exp = NP_OP[op](a if A else dt(s), b if Bb else dt(s)).astype(dt)
                assert same_bits(O.get(), exp), (n, op, mode, oa, ob, oo)
                assert O.guards_intact() and (A is None or A.guards_intact()), (n, op, mode, oa, ob, oo)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_subnormal_results_are_kept(dt):
    """the device keeps subnormal results of T arithmetic (no flush to zero): tiny * 0.5 and tiny / 4 stay nonzero"""
    n = 1000
    tiny = np.finfo(dt).tiny
    a = np.full(n, tiny, dtype=dt)
    out = Guarded(dt, n, 0)
    for op, s, expect in ((2, 0.5, tiny / 2), (3, 4.0, tiny / 4)):
        check(lib().nk_binary(op, n, Guarded(dt, n, 0, a).ptr, 0.0, None, s, out.ptr, CODE[dt], stream()), "nk_binary")
        got = out.get()
        assert np.all(got == dt(expect)) and np.all(got != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_axpby_and_clip_all_paths(dt):
    """axpby rounds alpha x + beta y once from fp64: with power-of-two scalars the products are exact, so the result is the
    correctly rounded sum -- numpy in T bit for bit (fp64), within 1 ulp of T of the fp64 value for general scalars (fp32).
    clip only selects: bit exact."""
    rng = np.random.default_rng(2)
    v = VW[dt]
    for n in map_lengths(v):
        x = with_subnormals(rand(rng, dt, n), dt)
        y = rand(rng, dt, n)
        for ox, oy, oo in patterns_for(n, 3, dt):
            X, Y, O = Guarded(dt, n, ox, x), Guarded(dt, n, oy, y), Guarded(dt, n, oo)
            check(lib().nk_axpby(n, 0.5, X.ptr, -4.0, Y.ptr, O.ptr, CODE[dt], stream()), "nk_axpby")
            exp = (dt(0.5) * x + dt(-4.0) * y).astype(dt)
            assert same_bits(O.get(), exp) and O.guards_intact(), (n, ox, oy, oo)
            check(lib().nk_axpby(n, 0.25, X.ptr, 0.0, None, O.ptr, CODE[dt], stream()), "nk_axpby")
            assert same_bits(O.get(), (dt(0.25) * x).astype(dt)) and O.guards_intact(), (n, ox, oo)
            if dt == np.float32:
                check(lib().nk_axpby(n, 0.3, X.ptr, 1.7, Y.ptr, O.ptr, CODE[dt], stream()), "nk_axpby")
                ref = 0.3 * x.astype(np.float64) + 1.7 * y.astype(np.float64)
                assert np.max(ulps(O.get(), ref, dt)) <= 1.0 and O.guards_intact(), (n, ox, oy, oo)
            F, D = Guarded(dt, n, oo), Guarded(dt, n, oy)
            check(lib().nk_clip(-0.5, 0.75, n, X.ptr, F.ptr, D.ptr, CODE[dt], stream()), "nk_clip")
            fx = np.clip(x, dt(-0.5), dt(0.75))
            assert same_bits(F.get(), fx) and F.guards_intact(), (n, ox, oo)
            assert same_bits(D.get(), np.where((fx == dt(-0.5)) | (fx == dt(0.75)), 0, 1).astype(dt)) and D.guards_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_pointwise_and_gather_all_paths(dt):
    """nk_pointwise at every path: fp64 sqrt / reciprocal / abs are correctly rounded (bit exact); fp32 computes in fp64
    and rounds once (<= 1 ulp of the fp64 value).  nk_gather copies: bit exact, table and indices at any offset."""
    rng = np.random.default_rng(3)
    v = VW[dt]
    fns = [("sqrt", 2, np.sqrt), ("reciprocal", 5, np.reciprocal), ("abs", 7, np.abs)]
    if dt == np.float32:
        fns += [("exp", 0, np.exp), ("tanh", 3, np.tanh), ("log1p", 8, np.log1p)]
    table = rand(rng, dt, 1000)
    for n in map_lengths(v):
        x = np.abs(rand(rng, dt, n)) + dt(0.01)
        idx = rng.integers(0, 1000, size=n).astype(np.int32)
        for ox, oo in patterns_for(n, 2, dt):
            X = Guarded(dt, n, ox, x)
            for name, fn, ref in fns:
                O = Guarded(dt, n, oo)
                check(lib().nk_pointwise(fn, 0.0, n, X.ptr, O.ptr, None, CODE[dt], stream()), "nk_pointwise")
                if dt == np.float64:
                    assert same_bits(O.get(), ref(x)), (name, n, ox, oo)
                else:
                    assert np.max(ulps(O.get(), ref(x.astype(np.float64)), dt)) <= 1.0, (name, n, ox, oo)
                assert O.guards_intact() and X.guards_intact(), (name, n, ox, oo)
            P, T = Guarded(np.int32, n, ox, idx), Guarded(dt, 1000, oo, table)
            O = Guarded(dt, n, oo)
            check(lib().nk_gather(n, T.ptr, ctypes.c_void_p(P.ptr), O.ptr, CODE[dt], stream()), "nk_gather")
            assert same_bits(O.get(), table[idx]) and O.guards_intact() and P.guards_intact(), (n, ox, oo)


def _cplx(x):
    z = np.empty(len(x) // 2, dtype=np.complex128)
    z.real, z.imag = x[0::2], x[1::2]  # (not re + 1j * im: 1j * inf would put a NaN into the real part)
    return z


def _close_normwise(got, ref, dt, k=4.0):
    """per element |got - ref| <= k eps_T |ref| (both components), plus the smallest subnormal of T"""
    eps, sub = float(np.finfo(dt).eps), float(np.finfo(dt).smallest_subnormal)
    err = np.abs(got - ref)
    return bool(np.all(err <= k * eps * np.abs(ref) + sub))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_complex_kernels_all_paths(dt):
    """nk_cplx_muldiv (kinds 0/1/2, conj_b, multiply / divide) and nk_cplx_pointwise over the same lengths and offsets;
    operands are interleaved (re, im) arrays at REAL-element offsets, so that fp64 offset 1 puts the output at 8 bytes"""
    rng = np.random.default_rng(4)
    v = VW[dt]
    ns = sorted({max(1, L // 2) for L in map_lengths(v)} | {(L + 1) // 2 for L in map_lengths(v)})
    for n in ns:
        a = rng.integers(-8, 9, size=2 * n).astype(dt)
        a[0::2] = np.where((a[0::2] == 0) & (a[1::2] == 0), dt(5), a[0::2])  # (no zero to take the reciprocal of)
        b = rng.integers(-8, 9, size=2 * n).astype(dt)
        b[0::2] = np.where(b[0::2] == 0, dt(3), b[0::2])
        br = b[0::2].copy()
        za, zb = _cplx(a), _cplx(b)
        for oa, ob, oo in patterns_for(n, 3, dt):
            A, Bc, Br = Guarded(dt, 2 * n, oa, a), Guarded(dt, 2 * n, ob, b), Guarded(dt, n, ob, br)
            Ar = Guarded(dt, n, oa, a[0::2].copy())
            cases = [(0, 0, 0, 0, za * zb), (0, 0, 1, 0, za * np.conj(zb)), (0, 0, 0, 1, za / zb), (0, 0, 1, 1, za / np.conj(zb)),
                     (0, 1, 0, 0, za * br.astype(np.float64)), (1, 0, 0, 1, a[0::2].astype(np.float64) / zb),
                     (0, 2, 0, 1, za / (0.5 - 2j)), (2, 0, 1, 0, (1.5 + 0.25j) * np.conj(zb))]
            for ka, kb, conj, div, ref in cases:
                O = Guarded(dt, 2 * n, oo)
                pa = A.ptr if ka == 0 else (Ar.ptr if ka == 1 else None)
                pb = Bc.ptr if kb == 0 else (Br.ptr if kb == 1 else None)
                check(lib().nk_cplx_muldiv(n, pa, ka, 1.5, 0.25, pb, kb, 0.5, -2.0, conj, div, O.ptr, CODE[dt], stream()),
                      "nk_cplx_muldiv")
                got = _cplx(O.get())
                if div:
                    assert _close_normwise(got, ref, dt), (n, ka, kb, conj, div, oa, ob, oo)
                else:  # small integers: every product and sum is exact
                    assert np.array_equal(got, ref), (n, ka, kb, conj, oa, ob, oo)
                assert O.guards_intact(), (n, ka, kb, conj, div, oa, ob, oo)
            for fn, ref in ((2, np.sqrt(za)), (3, 1 / za), (4, np.conj(za))):
                O = Guarded(dt, 2 * n, oo)
                check(lib().nk_cplx_pointwise(fn, n, A.ptr, O.ptr, CODE[dt], stream()), "nk_cplx_pointwise")
                got = _cplx(O.get())
                assert (np.array_equal(got, ref) if fn == 4 else _close_normwise(got, ref, dt)), (n, fn, oa, oo)
                assert O.guards_intact(), (n, fn, oa, oo)
            O = Guarded(dt, n, oo)
            check(lib().nk_cplx_pointwise(5, n, A.ptr, O.ptr, CODE[dt], stream()), "nk_cplx_pointwise")
            assert np.max(ulps(O.get(), np.abs(za), dt)) <= (1.0 if dt == np.float32 else 2.0) and O.guards_intact(), (n, oa, oo)


# ================================================== B. reductions ==========================================================
def red_lengths(dt):
    v = VW[dt]
    units = RED_UNITS * 2 * THREADS * v  # the shortest 64-unit layout (two 256-vector rows per unit)
    return map_lengths(v)[:-3] + [units, units + v]  # (the flat path is for maps only; long lengths: switch_lengths)


def switch_lengths(dt):
    """lengths on both sides of the 512-workgroup switch of nk_grid_red, aligned (vectors) and unaligned (scalars)"""
    v = VW[dt]
    edge = 512 * 32 * THREADS  # vectors (aligned) or elements (unaligned) with exactly 512 workgroups of 32 per thread
    return [(edge * v - v, True), (edge * v + v, True), (edge, False), (edge + 2, False)]


def _cg_operands(rng, dt, n, kind):
    return [rand(rng, dt, n, kind) for _ in range(5)]  # x, r, d, q, b


def _run_reductions(dt, n, offs, data, accumulate, with_b=True):
    """every reduction kernel on the same operands; checks the vectors they store and returns {name: (sum, [(p, w)])}: each
    device sum with the operand pair whose dot product it must equal"""
    x, r, d, q, b = data
    S = torch.zeros(8, dtype=torch.float64, device="cuda")
    pre = 1000.0 if accumulate else 0.0
    out = {}
    X, R, Dd, Q, Bb = (Guarded(dt, n, o, h) for o, h in zip(offs, data))
    assert all(G.guards_intact() for G in (X, R, Dd, Q, Bb))

    def fresh(vals):
        S.copy_(torch.tensor(vals + [0.0] * (8 - len(vals)), dtype=torch.float64))

    fresh([pre])
    check(lib().nk_vdot(n, X.ptr, Dd.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), accumulate, stream()), "nk_vdot")
    out["vdot"] = (S[0].item() - pre, [(x, d)])
    fresh([pre])
    check(lib().nk_sum(n, X.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), accumulate, stream()), "nk_sum")
    out["sum"] = (S[0].item() - pre, [(x, np.ones_like(x))])
    fresh([pre, pre])
    check(lib().nk_cg_curv(n, Dd.ptr, Q.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), accumulate, stream()), "nk_cg_curv")
    out["curv"] = (S[1].item() - pre, [(d, q)])
    O = Guarded(dt, n, offs[2])
    fresh([pre])
    check(lib().nk_axpby_sqnorm(n, 0.5, X.ptr, -2.0, R.ptr, O.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), accumulate,
                                stream()), "nk_axpby_sqnorm")
    z = (dt(0.5) * x + dt(-2.0) * r).astype(dt)
    assert same_bits(O.get(), z) and O.guards_intact()
    out["axpby_sqnorm"] = (S[0].item() - pre, [(z, z)])
    # CG: alpha = scal[0] / scal[1] = 0.25, beta = scal[2] / scal[0] = 2 (powers of two: the updates are exact roundings)
    fresh([0.5, 2.0, pre, pre, pre])
    check(lib().nk_cg_update(n, X.ptr, R.ptr, Dd.ptr, Q.ptr, Bb.ptr if with_b else None, CODE[dt],
                             ctypes.c_void_p(S.data_ptr()), accumulate, stream()), "nk_cg_update")
    xn, rn = (x - dt(0.25) * d).astype(dt), (r - dt(0.25) * q).astype(dt)
    assert same_bits(X.get(), xn) and same_bits(R.get(), rn) and X.guards_intact() and R.guards_intact()
    s = S.cpu().numpy()
    out["cg_rr"] = (s[2] - pre, [(rn, rn)])
    out["cg_xr"] = (s[3] - pre, [(xn, rn)])
    if with_b:
        out["cg_xb"] = (s[4] - pre, [(xn, b)])
    else:
        assert s[4] == pre, "the x.b slot of nk_cg_update without b must keep its value"
    X, R = Guarded(dt, n, offs[0], x), Guarded(dt, n, offs[1], r)
    fresh([0.5, 2.0, pre, pre])
    check(lib().nk_cg_update_dr(n, X.ptr, R.ptr, Dd.ptr, Q.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), accumulate, stream()),
          "nk_cg_update_dr")
    assert same_bits(X.get(), xn) and same_bits(R.get(), rn) and X.guards_intact() and R.guards_intact()
    s = S.cpu().numpy()
    out["dr_rr"] = (s[2] - pre, [(rn, rn)])
    out["dr_dr"] = (s[3] - pre, [(d, r)])
    Dd = Guarded(dt, n, offs[2], d)
    fresh([1.0, 4.0, 2.0, 7.0, 7.0, 0.0, 0.0])
    check(lib().nk_cg_direction(n, Dd.ptr, R.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), 1, stream()), "nk_cg_direction")
    assert same_bits(Dd.get(), (dt(2.0) * d + rn).astype(dt)) and Dd.guards_intact()
    assert S.cpu().tolist() == [2.0, 4.0, 0.0, 0.0, 0.0, 0.25, 2.0, 0.0]  # roll 1: gamma_prev, alpha, beta; slots cleared
    return out


def _check_exact(out, dt, n, offs):
    """the operands are multiples of 1/4 (integers, halved or quartered by the power-of-two scalars): 16 x the sum in int64"""
    for name, (got, pairs) in out.items():
        (p, w), = pairs
        p4, w4 = (4 * p.astype(np.float64)).astype(np.int64), (4 * w.astype(np.float64)).astype(np.int64)
        assert np.array_equal(p4, 4 * p.astype(np.float64)) and np.array_equal(w4, 4 * w.astype(np.float64))
        exp = Fraction(int(np.dot(p4, w4)), 16)
        assert Fraction(got) == exp, (name, n, offs, got, float(exp))


def _check_rounded(out, dt, n, offs):
    aligned = all(o == 0 for o in offs)
    for name, (got, pairs) in out.items():
        (p, w), = pairs
        exact = exact_dot(p, w)
        terms = np.abs(p.astype(np.float64) * w.astype(np.float64))
        bound = sum_bound(n, VW[dt], aligned, float(np.sum(terms)), product=dt == np.float64)
        if n >= 1000:  # the bound is tight: a single missing term of typical size breaks it
            assert bound < np.median(terms[terms > 0]), (name, n, bound)
        assert abs(got - exact) <= bound, (name, n, offs, got, exact, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_reductions_exact_on_integer_data(dt):
    """integer operands and power-of-two scalars: every sum is exactly representable, so every length, offset, layout and
    accumulate mode must give it exactly -- a dropped, doubled or misplaced element fails deterministically"""
    rng = np.random.default_rng(5)
    v = VW[dt]
    assert red_unit(red_lengths(dt)[-2], v) > 0 and red_unit(red_lengths(dt)[-1], v) == 0  # one 64-unit layout, one not
    for n in red_lengths(dt):
        data = _cg_operands(rng, dt, n, "int")
        for offs in patterns_for(n, 5, dt):
            for acc in (0, 1):  # (nk_cg_update without b at both accumulate modes, on every other length)
                _check_exact(_run_reductions(dt, n, offs, data, acc, with_b=acc == 0 or n % 2 == 0), dt, n, offs)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_reductions_exact_across_the_grid_switch(dt):
    rng = np.random.default_rng(6)
    for n, aligned in switch_lengths(dt):
        data = _cg_operands(rng, dt, n, "int")
        offs = (0,) * 5 if aligned else (1,) * 5
        _check_exact(_run_reductions(dt, n, offs, data, 0), dt, n, offs)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_reductions_on_normal_data_within_the_derived_bound(dt):
    rng = np.random.default_rng(7)
    for n in red_lengths(dt):
        data = _cg_operands(rng, dt, n, "normal")
        for offs in [(0,) * 5, (1,) * 5]:
            _check_rounded(_run_reductions(dt, n, offs, data, 0), dt, n, offs)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_stats_skips_nan_and_zero_and_keeps_inf(dt):
    rng = np.random.default_rng(8)
    for n in red_lengths(dt):
        x = rand(rng, dt, n, "int")
        x[rng.integers(0, n, size=max(1, n // 50))] = np.nan
        for offs in patterns_for(n, 1, dt):
            X = Guarded(dt, n, offs[0], x)
            S = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
            check(lib().nk_stats(n, X.ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), stream()), "nk_stats")
            keep = ~np.isnan(x) & (x != 0)
            xi = x[keep].astype(np.int64)
            assert S.cpu().tolist() == [float(xi.sum()), float((xi * xi).sum()), float(n - keep.sum())], (n, offs)
    x = np.array([1.0, np.inf, 0.0, np.nan, -2.0] * 300, dtype=dt)
    for y, exp in ((x, [np.inf, np.inf, 600.0]), (np.where(x == -2.0, -np.inf, x).astype(dt), [np.nan, np.inf, 600.0])):
        for off in (0, 1):
            S = torch.zeros(3, dtype=torch.float64, device="cuda")
            check(lib().nk_stats(len(y), Guarded(dt, len(y), off, y).ptr, CODE[dt], ctypes.c_void_p(S.data_ptr()), stream()),
                  "nk_stats")
            got = S.cpu().numpy()
            assert np.array_equal(got, np.array(exp), equal_nan=True), (off, got)


# ================================================ C. batched launches =======================================================
def _pa(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [4099, 65538])
def test_batches_with_one_unaligned_member_equal_single_calls(dt, n):
    from nifty_amd import _lib as L

    rng = np.random.default_rng(9)
    for count in range(1, 9):
        odd = count // 2
        offs = [1 if m == odd else 0 for m in range(count)]
        xs = [rand(rng, dt, n, "int") for _ in range(count)]
        ys = [rand(rng, dt, n, "int") for _ in range(count)]
        X = [Guarded(dt, n, o, h) for o, h in zip(offs, xs)]
        Y = [Guarded(dt, n, o, h) for o, h in zip(offs, ys)]
        # vdot
        res = [torch.full((1,), 3.0, dtype=torch.float64, device="cuda") for _ in range(count)]
        check(lib().nk_vdot_batch(n, count, _pa([g.ptr for g in X]), _pa([g.ptr for g in Y]), CODE[dt],
                                  _pa([t.data_ptr() for t in res]), 1, stream()), "nk_vdot_batch")
        for m in range(count):
            single = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
            check(lib().nk_vdot(n, X[m].ptr, Y[m].ptr, CODE[dt], ctypes.c_void_p(single.data_ptr()), 1, stream()), "nk_vdot")
            exp = 3.0 + float(np.dot(xs[m].astype(np.int64), ys[m].astype(np.int64)))
            assert res[m].item() == single.item() == exp, (count, m)
        # axpby, axpby_sqnorm and binary
        outs = [Guarded(dt, n, o) for o in offs]
        alpha, beta = [0.5 * (m + 1) for m in range(count)], [-2.0] * count
        check(lib().nk_axpby_batch(n, count, L.double_array(alpha), _pa([g.ptr for g in X]), L.double_array(beta),
                                   _pa([g.ptr for g in Y]), _pa([g.ptr for g in outs]), CODE[dt], stream()), "nk_axpby_batch")
        sq = [torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(count)]
        outs2 = [Guarded(dt, n, o) for o in offs]
        check(lib().nk_axpby_sqnorm_batch(n, count, L.double_array(alpha), _pa([g.ptr for g in X]), L.double_array(beta),
                                          _pa([g.ptr for g in Y]), _pa([g.ptr for g in outs2]), CODE[dt],
                                          _pa([t.data_ptr() for t in sq]), 0, stream()), "nk_axpby_sqnorm_batch")
        outs3 = [Guarded(dt, n, o) for o in offs]
        check(lib().nk_binary_batch(2, n, count, _pa([g.ptr for g in X]), L.double_array([0.0] * count),
                                    _pa([g.ptr for g in Y]), L.double_array([0.0] * count), _pa([g.ptr for g in outs3]),
                                    CODE[dt], stream()), "nk_binary_batch")
        for m in range(count):
            single = Guarded(dt, n, offs[m])
            check(lib().nk_axpby(n, alpha[m], X[m].ptr, beta[m], Y[m].ptr, single.ptr, CODE[dt], stream()), "nk_axpby")
            exp = (dt(alpha[m]) * xs[m] + dt(beta[m]) * ys[m]).astype(dt)
            assert same_bits(outs[m].get(), single.get()) and same_bits(single.get(), exp) and outs[m].guards_intact()
            assert same_bits(outs2[m].get(), exp) and outs2[m].guards_intact()
            assert sq[m].item() == math.fsum((exp.astype(np.float64) ** 2).tolist()), (count, m)  # (exact: quarters)
            assert same_bits(outs3[m].get(), xs[m] * ys[m]) and outs3[m].guards_intact()


# ============================================ D. pointwise edge arguments ==================================================
@pytest.fixture(autouse=True)
def _mp40():
    with mpmath.workdps(40):
        yield


LIB_FNS = {  # name: (nk fn code, mpmath function, param)
    "exp": (0, mpmath.exp, 0.0), "log": (1, mpmath.log, 0.0), "sqrt": (2, mpmath.sqrt, 0.0), "tanh": (3, mpmath.tanh, 0.0),
    "log1p": (8, mpmath.log1p, 0.0), "expm1": (9, mpmath.expm1, 0.0), "arctan": (10, mpmath.atan, 0.0),
    "sin": (11, mpmath.sin, 0.0), "cos": (12, mpmath.cos, 0.0), "tan": (13, mpmath.tan, 0.0),
    "log10": (15, mpmath.log10, 0.0), "sinh": (16, mpmath.sinh, 0.0), "cosh": (17, mpmath.cosh, 0.0),
    "power": (6, lambda v: mpmath.power(v, mpmath.mpf(2.5)), 2.5),
    "power_neg": (6, lambda v: mpmath.power(v, mpmath.mpf(-1.5)), -1.5),
    "exponentiate": (20, lambda v: mpmath.power(mpmath.mpf(10.0), v), 10.0),
}


def edge_args(name, dt):
    f32 = dt == np.float32
    sub = [1e-45, -1e-45, 1e-40, -1e-40] if f32 else [5e-324, -5e-324, 1e-310, -1e-310]
    small = [1e-38, -1e-38] if f32 else [1e-300, -1e-300]
    common = [0.0, -0.0] + sub + small + [1e-8, -1e-8, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 10.0, -20.0]
    big = 1e38 if f32 else 1e300
    extra = {
        "exp": [88.72, -87.0, -103.0] if f32 else [709.7, -708.5, -745.0],
        "expm1": [88.72, -40.0] if f32 else [709.7, -40.0],
        "sinh": [89.41, -89.41] if f32 else [710.4, -710.4],
        "cosh": [89.41, -89.41] if f32 else [710.4, -710.4],
        "tanh": [20.0, -40.0, big],
        "log1p": [-1 + 2.0 ** -24, -0.999999, -1 + 1e-7] if f32 else [-1 + 2.0 ** -53, -0.999999, -1 + 1e-10],
        "log": [big, 1 + 2.0 ** -23 if f32 else 1 + 2.0 ** -52, 0.99999],
        "log10": [big, 1000.0, 0.99999],
        "sqrt": [big, 2.0],
        "sin": [1e5, 1e15, big, -big], "cos": [1e5, 1e15, big, -big, 1.5707963267948966], "tan": [1e5, 1e15, big, -big],
        "arctan": [big, -big, 1e8],
        "power": [1e-8, 1e10, 7.0], "power_neg": [1e-8, 1e10, 7.0], "exponentiate": [30.0, -30.0, 37.5] if f32 else [300.0, -300.0, 307.5],
    }[name]
    return np.array(common + extra, dtype=dt)


def _domain_ok(name, v):
    if name in ("log", "log10", "sqrt", "power", "power_neg"):
        return v > 0
    if name == "log1p":
        return v > -1
    return True


def _pointwise(dt, fn, param, x):
    n = len(x)
    X, F = Guarded(dt, n, 1, x), Guarded(dt, n, 0)
    check(lib().nk_pointwise(fn, param, n, X.ptr, F.ptr, None, CODE[dt], stream()), "nk_pointwise")
    assert F.guards_intact()
    return F.get()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(LIB_FNS))
def test_library_functions_at_edge_arguments(dt, name):
    """relative error against mpmath at 40 digits, with no floor: <= 4 ulp in fp64; in fp32 (computed in fp64 and rounded
    once) <= 1 ulp.  Arguments outside the real domain, ±inf and NaN give what IEEE / C99 prescribe (numpy in fp64)."""
    fn, mf, param = LIB_FNS[name]
    x = edge_args(name, dt)
    got = _pointwise(dt, fn, param, x)
    fmax, lim = float(np.finfo(dt).max), 1.0 if dt == np.float32 else 4.0
    checked = 0
    for xv, gv in zip(x.tolist(), got.tolist()):
        if not _domain_ok(name, xv) or (name in ("power_neg", "log", "log10") and xv == 0):
            continue
        ref = mf(mpmath.mpf(xv))
        if abs(ref) >= fmax * (1 - 2.0 ** -30):
            continue  # the result overflows T
        spacing = float(np.spacing(dt(abs(float(ref)))))
        err = abs(mpmath.mpf(gv) - ref) / spacing
        assert err <= lim, (name, xv, gv, float(ref), float(err))
        if ref == 0:
            assert math.copysign(1, gv) == math.copysign(1, xv) or name in ("power", "exponentiate"), (name, xv, gv)
        checked += 1
    assert checked >= 6
    # special values: numpy fp64 (C99 Annex F), cast to T
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, -1.0, -2.0], dtype=dt)
    got = _pointwise(dt, fn, param, sp)
    ref_np = {"exp": np.exp, "log": np.log, "sqrt": np.sqrt, "tanh": np.tanh, "log1p": np.log1p, "expm1": np.expm1,
              "arctan": np.arctan, "sin": np.sin, "cos": np.cos, "tan": np.tan, "log10": np.log10, "sinh": np.sinh,
              "cosh": np.cosh, "power": lambda v: np.power(v, 2.5), "power_neg": lambda v: np.power(v, -1.5),
              "exponentiate": lambda v: np.power(10.0, v)}[name]
    with np.errstate(all="ignore"):
        exp = ref_np(sp.astype(np.float64)).astype(dt)
    for xv, gv, ev in zip(sp.tolist(), got.tolist(), exp.tolist()):
        if np.isnan(ev) or np.isinf(ev) or ev == 0:
            assert (np.isnan(gv) and np.isnan(ev)) or gv == ev, (name, xv, gv, ev)


FORMULA_FNS = {  # name: (code, want the derivative, numpy fp64 formula of the kernel, arguments)
    "softplus": (19, False, lambda v: np.where(v > 33, v, np.where(v < -33, 0.0, np.log(1 + np.exp(v)))),
                 [-40.0, -33.5, -32.9, -5.0, -1e-8, 0.0, 1e-8, 2.0, 20.0, 32.9, 33.1]),
    "sigmoid": (4, False, lambda v: 0.5 + 0.5 * np.tanh(v), [-0.5, -1e-8, 0.0, 1e-8, 0.3, 3.0, 20.0]),
    "tanh_derivative": (3, True, lambda v: 1 - np.tanh(v) ** 2, [-1.0, -0.5, -1e-8, 0.0, 1e-8, 0.25, 0.75, 1.0]),
    "sinc_derivative": (14, True, lambda v: np.where(v == 0, 0.0, (np.cos(np.pi * v) - np.sin(np.pi * v) / (np.pi * v)) / v),
                        [-2.75, -1.5, -0.75, 0.0, 0.5, 0.75, 1.5, 2.75]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(FORMULA_FNS))
def test_formula_functions_match_their_formula(dt, name):
    """functions that pointwise.py defines by a formula: compared in ulps with that formula in numpy fp64 (8 ulp in fp64 --
    two library calls and a subtraction on each side, at arguments where the subtraction amplifies a library ulp at most
    about 2x; fp32 rounds once from fp64: 1 ulp)"""
    fn, deriv, formula, args = FORMULA_FNS[name]
    x = np.array(args, dtype=dt)
    n = len(x)
    X, F, D = Guarded(dt, n, 1, x), Guarded(dt, n, 0), Guarded(dt, n, 3 if dt == np.float32 else 1)
    check(lib().nk_pointwise(fn, 0.0, n, X.ptr, F.ptr, D.ptr, CODE[dt], stream()), "nk_pointwise")
    assert F.guards_intact() and D.guards_intact()
    got = (D if deriv else F).get()
    ref = formula(x.astype(np.float64))
    assert np.max(ulps(got, ref, dt)) <= (1.0 if dt == np.float32 else 8.0), (name, got, ref)


# ============================================ E. complex kernels, component-wise ===========================================
def _mags(dt):
    return [-140, -126, -60, 0, 60, 126] if dt == np.float32 else [-1000, -600, -520, -160, 0, 160, 520, 1000]


def _cplx_inputs(dt, rng):
    """components m 2^k (m in [1, 2), random signs) for every pair of magnitudes: alike and mixed"""
    ks = _mags(dt)
    out = []
    for kr in ks:
        for ki in ks:
            for sr in (1, -1):
                for si in (1, -1):
                    out.append(complex(sr * math.ldexp(1 + rng.random(), kr), si * math.ldexp(1 + rng.random(), ki)))
    return _as_t(out, dt)


def _as_t(z, dt, keep_zero=False):
    """the values exactly as complex T holds them (fp64 components); drops what T cannot hold (inf, and 0 unless kept)"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.complex128).astype(np.complex64 if dt == np.float32 else np.complex128).astype(np.complex128)
    return z if keep_zero else z[np.isfinite(z) & (z != 0)]


def _to_dev(z, dt, off=0):
    buf = np.empty(2 * len(z), dtype=dt)
    buf[0::2], buf[1::2] = z.real, z.imag
    return Guarded(dt, 2 * len(z), off, buf)


def _cplx_pw(dt, fn, z):
    X = _to_dev(z, dt, 1)
    O = Guarded(dt, len(z) if fn == 5 else 2 * len(z), 0)
    check(lib().nk_cplx_pointwise(fn, len(z), X.ptr, O.ptr, CODE[dt], stream()), "nk_cplx_pointwise")
    assert O.guards_intact()
    return O.get().astype(np.float64) if fn == 5 else _cplx(O.get())


def _cplx_div(dt, a, b):
    A, Bc, O = _to_dev(a, dt, 1), _to_dev(b, dt, 0), Guarded(dt, 2 * len(a), 0)
    check(lib().nk_cplx_muldiv(len(a), A.ptr, 0, 0.0, 0.0, Bc.ptr, 0, 0.0, 0.0, 0, 1, O.ptr, CODE[dt], stream()), "nk_cplx_muldiv")
    assert O.guards_intact()
    return _cplx(O.get())


def _comp_ulps(got, ref, dt):
    """per component: |got - ref| in ulps of that component of the (mpmath) reference; a component beyond the range of T
    must be the infinity of its sign"""
    def one(g, r):
        with np.errstate(over="ignore"):
            rt = dt(float(r))
        if np.isinf(rt):
            return 0.0 if g == float(rt) else math.inf
        return float(ulps(g, float(r), dt))
    return max(one(got.real, ref.real), one(got.imag, ref.imag))


def _norm_err(got, ref, dt):
    """max component error in units of eps_T |ref| (+ the smallest subnormal of T)"""
    eps, sub = float(np.finfo(dt).eps), float(np.finfo(dt).smallest_subnormal)
    scale = eps * float(abs(ref)) + sub
    return max(float(abs(mpmath.mpf(got.real) - ref.real)), float(abs(mpmath.mpf(got.imag) - ref.imag))) / scale


def _fits(w, dt):
    return float(abs(w)) < float(np.finfo(dt).max) / 4


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["c64", "c128"])
def test_complex_sqrt_componentwise(dt):
    rng = np.random.default_rng(10)
    z = np.concatenate([_cplx_inputs(dt, rng), np.array([4 + 1e-9j, 4 + 1e-6j, -1 + 1e-20j, -4 - 1e-9j, 1e-30j], dtype=np.complex128)])
    z = _as_t(z, dt)
    got = _cplx_pw(dt, 2, z)
    for zi, gi in zip(z, got):
        ref = mpmath.sqrt(mpmath.mpc(zi.real, zi.imag))
        assert _comp_ulps(gi, ref, dt) <= 4, (zi, gi, complex(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["c64", "c128"])
def test_complex_reciprocal_componentwise(dt):
    rng = np.random.default_rng(11)
    z = np.concatenate([_cplx_inputs(dt, rng), np.array([3e-160, 1e-170 + 2e-170j, 1e300 - 1e300j], dtype=np.complex128)])
    z = _as_t(z, dt)
    got = _cplx_pw(dt, 3, z)
    for zi, gi in zip(z, got):
        ref = 1 / mpmath.mpc(zi.real, zi.imag)
        assert _comp_ulps(gi, ref, dt) <= 4, (zi, gi, complex(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["c64", "c128"])
def test_complex_division_normwise(dt):
    rng = np.random.default_rng(12)
    z = _cplx_inputs(dt, rng)
    a = np.concatenate([z, rng.permutation(z), [3 + 4j, 1e-200 + 1e-200j, 1e300 + 1e300j]])
    b = np.concatenate([rng.permutation(z), z, [1e-170, 1e-170 + 2e-170j, 1e300 - 1e300j]])
    a, b = _as_t(a, dt, keep_zero=True), _as_t(b, dt, keep_zero=True)
    ok = np.isfinite(a) & np.isfinite(b) & (b != 0)
    a, b = a[ok], b[ok]
    refs = [mpmath.mpc(x.real, x.imag) / mpmath.mpc(y.real, y.imag) for x, y in zip(a, b)]
    keep = np.array([_fits(r, dt) for r in refs])
    assert keep.sum() > len(keep) // 2
    got = _cplx_div(dt, a[keep], b[keep])
    for x, y, gi, ref in zip(a[keep], b[keep], got, [r for r, k in zip(refs, keep) if k]):
        assert _norm_err(gi, ref, dt) <= 4, (x, y, gi, complex(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["c64", "c128"])
def test_complex_log_exp_abs(dt):
    rng = np.random.default_rng(13)
    z = np.concatenate([_cplx_inputs(dt, rng), np.array([1e200 + 1e200j, 1 + 1e-8j, 0.6 + 0.8j], dtype=np.complex128)])
    z = _as_t(z, dt)
    eps = float(np.finfo(dt).eps)
    got = _cplx_pw(dt, 1, z)
    for zi, gi in zip(z, got):
        ref = mpmath.log(mpmath.mpc(zi.real, zi.imag))
        # real part relative, except near |z| = 1 where log|z| cancels: there normwise (a few eps of |log z| >= |arg z|)
        err_re = abs(mpmath.mpf(gi.real) - ref.real)
        assert err_re <= 4 * float(np.spacing(dt(abs(float(ref.real))))) + 4 * eps * float(abs(ref)), (zi, gi, complex(ref))
        assert float(ulps(gi.imag, float(ref.imag), dt)) <= 4, (zi, gi, complex(ref))
    got = _cplx_pw(dt, 5, z)
    for zi, gi in zip(z, got):
        assert float(ulps(gi, float(abs(mpmath.mpc(zi.real, zi.imag))), dt)) <= (1 if dt == np.float32 else 2), (zi, gi)
    # exp: the real part stays where the result is finite
    zr = np.array([complex(np.clip(w.real, -600 if dt == np.float64 else -80, 2), w.imag) for w in z], dtype=np.complex128)
    zr = zr.astype(np.complex64 if dt == np.float32 else np.complex128).astype(np.complex128)
    got = _cplx_pw(dt, 0, zr)
    for zi, gi in zip(zr, got):
        ref = mpmath.exp(mpmath.mpc(zi.real, zi.imag))
        assert _norm_err(gi, ref, dt) <= 4, (zi, gi, complex(ref))


# ========================================== F. offsets into unchecked kernels ==============================================
def _view_at(t, off):
    """a contiguous copy of t that starts `off` elements into a fresh buffer"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_unaligned_views_into_transforms_give_the_aligned_bits(tdt):
    from nifty_amd import backend as B

    g = torch.Generator(device="cuda").manual_seed(14)
    offs = (1, 2, 3) if tdt == torch.float32 else (1,)
    for shape in ((64, 48), (4096,), (32, 16, 24)):
        x = torch.randn(shape, dtype=tdt, device="cuda", generator=g)
        xc = torch.complex(x, torch.randn(shape, dtype=tdt, device="cuda", generator=g))
        flat = x.reshape(-1)
        tab = torch.randn(777, dtype=tdt, device="cuda", generator=g)
        pidx = torch.randint(0, 777, (flat.numel(),), dtype=torch.int32, device="cuda", generator=g)
        ref = {"hartley": B.hartley(x), "fftn": B.fftn(xc), "cumsum": B.cumsum(flat), "roll": B.roll(x, [3] * x.dim()),
               "gather": B.gather(tab, pidx, (flat.numel(),))}
        for off in offs:
            xv, fv, tv = _view_at(x, off), _view_at(flat, off), _view_at(tab, off)
            got = {"hartley": B.hartley(xv), "fftn": B.fftn(_view_at(xc, off)), "cumsum": B.cumsum(fv),
                   "roll": B.roll(xv, [3] * x.dim()), "gather": B.gather(tv, _view_at(pidx, off), (flat.numel(),))}
            for k in ref:
                assert torch.equal(got[k].cpu(), ref[k].cpu()), (k, shape, off)


@pytest.mark.gpu
@pytest.mark.parametrize("npdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_packed_multifield_feeds_transforms_the_same_bits(npdt):
    """a device MultiField with scalar keys before `xi` is packed into one buffer by `+`: `xi` of the sum is a view at an
    odd element offset, and a HarmonicTransformOperator on it must give the bits of the same call on an aligned copy"""
    import nifty_amd as ift

    h = ift.RGSpace((32, 48), harmonic=True)
    dom = ift.MultiDomain.make({"a": ift.UnstructuredDomain(1), "b": ift.UnstructuredDomain(2), "xi": h})
    rng = np.random.default_rng(15)
    f1 = ift.MultiField.from_dict({k: ift.makeField(dom[k], rng.standard_normal(dom[k].shape).astype(npdt)) for k in dom.keys()})
    f2 = ift.MultiField.from_dict({k: ift.makeField(dom[k], rng.standard_normal(dom[k].shape).astype(npdt)) for k in dom.keys()})
    s = f1.at(0) + f2.at(0)
    xi = s["xi"]
    assert s._flat is not None and (xi.val.data_ptr() % 16) != 0, "the packed sum should leave xi unaligned"
    ht = ift.HarmonicTransformOperator(h)
    aligned = ift.makeField(h, xi.val.clone())
    assert aligned.val.data_ptr() % 16 == 0
    assert torch.equal(ht(xi).val.cpu(), ht(aligned).val.cpu())


# ============================================= host tests of the references ================================================
def test_launch_constants_match_the_source():
    src = open(os.path.join(CSRC, "nk_vec.hip")).read()
    util = open(os.path.join(CSRC, "nk_util.h")).read()

    def const(text, name):
        factors = re.search(r"constexpr int %s = ([\d *]+);" % name, text).group(1).split("*")
        return math.prod(int(f) for f in factors)

    assert const(src, "NK_VEC_THREADS") == THREADS
    assert const(src, "NK_MAX_BLOCKS") == 256 * 8 == MAX_BLOCKS
    assert const(util, "NK_RED_UNITS") == RED_UNITS
    assert 'nk_vec_env_int("NK_RED_UNIT_GRID", %d)' % UNIT_GRID in src
    # the flat-path rule and the reduction grid rule these helpers mirror
    assert "pieces > NK_MAX_BLOCKS" in src and "(nvec + NK_VEC_THREADS - 1) / NK_VEC_THREADS" in src
    assert "if (b > 512) b = std::max<int64_t>(512, (nvec + 64 * NK_VEC_THREADS - 1) / (64 * NK_VEC_THREADS));" in src
    assert "n % (NK_RED_UNITS * row) != 0 || n / (NK_RED_UNITS * row) < 2" in src


def test_launch_length_table():
    assert map_lengths(2)[-3:] == [1048576, 1048578, 1048579]
    assert map_lengths(4)[-3:] == [2097152, 2097156, 2097159]
    for v in (2, 4):
        def pieces(n):
            return -(-(n // v) // THREADS)
        assert pieces(last_chunked(v)) == MAX_BLOCKS and pieces(last_chunked(v) + v - 1) == MAX_BLOCKS
        assert pieces(first_flat(v)) == MAX_BLOCKS + 1 and (first_flat(v) + v - 1) % v == v - 1
    # 64-unit layouts: fp64 65536, fp32 131072; the same length plus V is one unit
    assert red_lengths(np.float64)[-2:] == [65536, 65538] and red_lengths(np.float32)[-2:] == [131072, 131076]
    assert red_unit(65536, 2) == 1024 and red_unit(65538, 2) == 0 and red_unit(131072, 4) == 2048
    # both sides of the 512-workgroup switch
    for dt in DTYPES:
        (lo, _), (hi, _), (ulo, _), (uhi, _) = switch_lengths(dt)
        v = VW[dt]
        assert -(-(lo // v) // (32 * THREADS)) == 512 and -(-(hi // v) // (32 * THREADS)) == 513
        assert -(-ulo // (32 * THREADS)) == 512 and -(-uhi // (32 * THREADS)) == 513
        assert red_unit(lo, v) == 0 and red_unit(hi, v) == 0 and max(lo, hi, ulo, uhi) <= 1 << 26
    assert switch_lengths(np.float64)[1][0] == 8388610


def test_two_product_and_exact_sums_against_fractions():
    rng = np.random.default_rng(16)
    a = rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, size=200)
    b = rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, size=200)
    p, e = two_product(a, b)
    for ai, bi, pi, ei in zip(a.tolist(), b.tolist(), p.tolist(), e.tolist()):
        assert Fraction(pi) + Fraction(ei) == Fraction(ai) * Fraction(bi)
        hi, lo = split(np.array([ai]))
        assert Fraction(float(hi[0])) + Fraction(float(lo[0])) == Fraction(ai)
    for dt in DTYPES:
        x = rng.standard_normal(300).astype(dt) * dt(1e3)
        y = rng.standard_normal(300).astype(dt)
        exact = sum(Fraction(float(u)) * Fraction(float(w)) for u, w in zip(x, y))
        got = exact_dot(x, y)
        assert got == float(exact)  # correctly rounded (Fraction -> float rounds to nearest)
        assert abs(Fraction(got) - exact) <= abs(Fraction(float(np.nextafter(got, np.inf))) - Fraction(got))


def test_error_bound_helpers():
    # the bound is tight enough to see one typical missing term at every reduction length of the suite
    for dt in DTYPES:
        for n in red_lengths(dt) + [L for L, _ in switch_lengths(dt)]:
            if n < 1000:
                continue
            for aligned in (True, False):
                assert sum_bound(n, VW[dt], aligned, 0.8 * n, product=True) < 0.05, (dt, n, aligned)
    assert red_grid(65536, 2, True) == 64 and red_grid(8388610, 2, True) == 512 and red_grid(100, 2, False) == 1
    # ulps / same_bits
    assert ulps(np.float32(1) + np.float32(2.0 ** -23), 1.0, np.float32) == 1.0
    assert same_bits(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0]))
    assert not same_bits(np.array([0.0]), np.array([-0.0]))
