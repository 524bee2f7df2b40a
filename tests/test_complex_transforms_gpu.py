"""nk_fftn, nk_bluestein_rows and nk_cplx_rows called directly through the C ABI, and the array seam backend.fftn /
backend.hartley on lengths the planner rejects, against long-double transforms with DERIVED bounds
(tests/transform_cases.py: references, derivations, comparators, the tables of shapes and lengths).

Input, output and workspace sit between guard bands of NaN, the bands are checked bit-wise afterwards, no NaN may reach an
output, and an input the call may only read is bit-unchanged.  Every case prints one line
`ERR kind= shape= n= m= dtype= mode= err= bound= err_u= host=` (err_u: the error in unit roundoffs; host: the error of a
restatement in T on the same input); profiles/r09_complex_transform_errors.txt keeps one run's lines."""
import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from nifty_amd import backend as B
from nifty_amd import config
from tests import transform_cases as tc
from tests.test_fused_transforms_gpu import Guarded, PlanH, stream

pytestmark = pytest.mark.gpu

LD, CLD = np.longdouble, np.clongdouble
DTYPES = [np.float64, np.float32]
OK, INVALID, UNSUPPORTED = L.NK_OK, L.NK_ERR_INVALID, L.NK_ERR_UNSUPPORTED


def code(dtype):
    return L.NK_F32 if np.dtype(dtype) == np.float32 else L.NK_F64


def sid(shape):
    return "x".join(map(str, shape))


def record(kind, dtype, mode, err, bound, host, shape=None, n=0, m=0):
    u = tc.unit_roundoff(dtype)
    print(f"ERR kind={kind} shape={sid(shape) if shape else '-'} n={n} m={m} dtype={np.dtype(dtype).name} mode={mode} err={err:.3e} "
          f"bound={bound:.3e} err_u={err / u:.2f} host={host:.3e}")


# ---- nk_fftn -------------------------------------------------------------------------------------------------------------
def run_fftn(plan, x, inverse, scale, inplace):
    """one guarded nk_fftn call on the first plan.batch members of x; returns the output"""
    gin, ws = Guarded(x), plan.workspace()
    gout = gin if inplace else Guarded(np.full_like(x, np.nan))
    L.check(plan.lib.nk_fftn(plan.p, gin.ptr, gout.ptr, int(inverse), float(scale), ws.ptr, stream()), "nk_fftn")
    torch.cuda.synchronize()
    got = gout.get()
    assert gin.guards_intact() and gout.guards_intact() and ws.guards_intact()
    assert inplace or gin.unchanged()
    assert not np.isnan(got.view(got.real.dtype)).any()
    return got


def c2c_params():
    return [pytest.param(s, d, id=f"{sid(s)}-{np.dtype(d).name}") for d in DTYPES for s in tc.c2c_shapes(d)]


def plan_lds(plan):
    """(contiguous, middle, first) bytes of dynamic LDS of the plan's c2c launches, from the LIBRARY (nk_plan_c2c_lds)"""
    import ctypes

    lds = (ctypes.c_int64 * 3)()
    L.check(plan.lib.nk_plan_c2c_lds(plan.p, lds), "nk_plan_c2c_lds")
    return tuple(lds)


def assert_c2c_set_up(plan, shape, dtype):
    """The plan is in the branch of the c2c set-up its shape is in the table for -- asked of the library, so that a change
    of the tile rules fails here; the restatement tc.c2c_lds_bytes must agree on every shape."""
    got = plan_lds(plan)
    assert got == tc.c2c_lds_bytes(shape, dtype, plan.batch), (shape, plan.batch, got)
    big, lds = tc.C2C_BIG_LDS[np.dtype(dtype)]
    if shape == big:
        assert got[2] == lds > 64 * 1024
    if shape == (1000, 8) and np.dtype(dtype) == np.float64:
        assert got[2] == 64000  # the listed shape stays just below the opt-in
    if shape == (tc.c2c_longest(dtype),):  # the rule of nk_plan_create: one padded line in 144 KiB
        nl, lim = shape[0], tc.c2c_line_limit(dtype)
        assert nl + nl // 16 + 1 <= lim == (9216 if np.dtype(dtype) == np.float64 else 18432)
        assert got == ((nl + nl // 16 + 1) * (144 * 1024 // lim), 0, 0) and got[0] > 64 * 1024


@pytest.mark.parametrize("shape,dtype", c2c_params())
def test_fftn_normal_data(shape, dtype):
    """forward and inverse, scale 1 and 0.75, out of place and in place, batch 1 and 3, against fft_ld inside c2c_rel_bound"""
    nd = len(shape)
    x3 = tc.normal_complex((3,) + shape, dtype, 51)
    rel = tc.c2c_rel_bound(shape, dtype)
    refs = {inv: tc.fft_ld(x3, nd, inv) for inv in (False, True)}
    hosts = {inv: tc.err_l2c(tc.fft_same_precision(x3, nd, inv), refs[inv]) / tc.l2c(refs[inv]) for inv in (False, True)}
    assert max(hosts.values()) <= rel
    for batch in (1, 3):
        with PlanH(shape, dtype, batch) as plan:
            assert plan.lib.nk_plan_c2c_ok(plan.p) == 1
            assert_c2c_set_up(plan, shape, dtype)
            x = x3[:batch]
            for inv in (False, True):
                for scale in (1.0, 0.75):
                    ref = LD(scale) * refs[inv][:batch]
                    nrm = tc.l2c(ref)
                    for inplace in (False, True):
                        got = run_fftn(plan, x, inv, scale, inplace)
                        ok, e = tc.within_l2c(got, ref, rel * nrm)
                        record("c2c", dtype, f"normal/b{batch}/inv{int(inv)}/s{scale}/{'in' if inplace else 'out'}place", e / nrm, rel,
                               hosts[inv], shape=shape)
                        assert ok, (batch, inv, scale, inplace, e / nrm, rel)


@pytest.mark.parametrize("shape,dtype", c2c_params())
def test_fftn_structured_inputs(shape, dtype):
    """Impulses element by element (the impulse in the second member of a batch of two, whose first member must come out as
    exact zeros), the constant and one complex exponential: exact answers, in the 2-norm and in every element."""
    nd, cdt = len(shape), tc.complex_dtype(dtype)
    rel, ebound = tc.c2c_rel_bound(shape, dtype), tc.c2c_impulse_elem_bound(shape, dtype)
    with PlanH(shape, dtype, 2) as plan:
        worst_all = 0.0
        for i, p in enumerate(tc.impulse_positions(shape)):
            inv, scale = bool(i % 2), (1.5 if i % 3 == 0 else 1.0)
            x = np.zeros((2,) + shape, dtype=cdt)
            x[(1,) + p] = 1.0
            got = run_fftn(plan, x, inv, scale, False)
            assert not got[0].any(), p
            ref = LD(scale) * tc.impulse_reference_c2c(shape, p, inv)
            ok, worst = tc.within_elem_c(got[1], ref, scale * ebound)
            worst_all = max(worst_all, worst)
            assert ok, (p, inv, worst)
            assert tc.within_l2c(got[1], ref, rel * tc.l2c(ref))[0], p
        p = tc.impulse_positions(shape)[-1]
        x1 = np.zeros(shape, dtype=cdt)
        x1[p] = 1.0
        host = float(np.max(np.abs(tc.fft_same_precision(x1, nd).astype(CLD) - tc.impulse_reference_c2c(shape, p))))
        record("c2c", dtype, "impulse/elementwise", worst_all * ebound, ebound, host, shape=shape)
        # the constant and exp(2 pi i q.j / n), rounded to T: the transform of what was handed over, N at one coefficient
        q = [min(3, n - 1) for n in shape]
        th = sum((np.arange(n, dtype=np.int64) * k % n).reshape([-1 if e == d else 1 for e in range(nd)]) / n
                 for d, (n, k) in enumerate(zip(shape, q)))
        x = np.stack([np.full(shape, 1.0 - 0.5j), np.exp(2j * np.pi * th)]).astype(cdt)
        for inv in (False, True):
            ref = tc.fft_ld(x, nd, inv)
            peak = tuple(k if not inv else (-k) % n for k, n in zip(q, shape))
            assert abs(ref[1][peak]) > 0.999 * x[1].size and abs(ref[0][(0,) * nd]) > 1.1 * x[0].size
            got = run_fftn(plan, x, inv, 1.0, False)
            for k, name in enumerate(("constant", "exponential")):
                nrm = tc.l2c(ref[k])
                ok, e = tc.within_l2c(got[k], ref[k], rel * nrm)
                okm, _ = tc.within_elem_c(got[k], ref[k], rel * nrm)
                hk = tc.err_l2c(tc.fft_same_precision(x[k], nd, inv), ref[k]) / nrm
                record("c2c", dtype, f"{name}/inv{int(inv)}", e / nrm, rel, hk, shape=shape)
                assert ok and okm, (name, inv, e / nrm, rel)


@pytest.mark.parametrize("shape,dtype", c2c_params())
def test_fftn_inverse_is_the_forward_transform_of_the_swapped_input(shape, dtype):
    """With scale = 1, nk_fftn(inverse = 1)(z) equals swap(nk_fftn(inverse = 0)(swap z)) bit for bit (swap exchanges re and
    im): that is how every pass implements the inverse, and a pass that forgets one of its two swaps fails this."""
    x = tc.normal_complex((3,) + shape, dtype, 53)

    def swap(z):
        out = np.empty_like(z)
        out.real, out.imag = z.imag, z.real
        return out

    with PlanH(shape, dtype, 3) as plan:
        inv = run_fftn(plan, x, True, 1.0, False)
        fwd = run_fftn(plan, swap(x), False, 1.0, False)
    r = inv.real.dtype
    assert np.array_equal(inv.view(r), swap(fwd).view(r))


def test_two_live_plans_with_different_dynamic_lds_needs():
    """Plan A needs 128 KiB of dynamic LDS in k_c2c_strided<double>, plan B -- created AFTER it -- 80 KiB: A, B, A must all
    run and meet their bound (nk_allow_lds sets the kernel's attribute at every plan creation)."""
    dtype = np.float64
    (sa, la), (sb, lb) = tc.C2C_TWO_PLANS
    data = {}
    for s in (sa, sb):
        x = tc.normal_complex((1,) + s, dtype, 54)
        ref = tc.fft_ld(x, 2)
        data[s] = (x, ref, tc.err_l2c(tc.fft_same_precision(x, 2), ref) / tc.l2c(ref))
    with PlanH(sa, dtype) as pa, PlanH(sb, dtype) as pb:
        assert plan_lds(pa)[2] == la > plan_lds(pb)[2] == lb > 64 * 1024  # the library's figures: both opt in, A needs more
        for i, (plan, s) in enumerate(((pa, sa), (pb, sb), (pa, sa))):
            x, ref, host = data[s]
            rel = tc.c2c_rel_bound(s, dtype)
            got = run_fftn(plan, x, False, 1.0, False)
            ok, e = tc.within_l2c(got, ref, rel * tc.l2c(ref))
            record("c2c", dtype, f"two-plans/run{i}", e / tc.l2c(ref), rel, host, shape=s)
            assert ok, (i, s, e)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_next_even_smooth_length_is_refused_by_the_c2c_kernel(dtype):
    """The longest line is the longest: the next even 7-smooth length (fp64: 8748) still has a plan -- the real transforms
    hold half a line -- whose nk_plan_c2c_ok is 0, whose LDS figures are 0 and whose nk_fftn is NK_ERR_UNSUPPORTED."""
    nl = tc.c2c_longest(dtype) + 2
    while not tc.is_smooth(nl):
        nl += 2
    assert nl + nl // 16 + 1 > tc.c2c_line_limit(dtype) and (nl != 8748) == (np.dtype(dtype) == np.float32)
    x = tc.normal_complex((1, nl), dtype, 64)
    with PlanH((nl,), dtype) as plan:
        assert plan.lib.nk_plan_c2c_ok(plan.p) == 0 and plan_lds(plan) == (0, 0, 0)
        gin, gout = Guarded(x), Guarded(np.full_like(x, np.nan))
        assert plan.lib.nk_fftn(plan.p, gin.ptr, gout.ptr, 0, 1.0, None, stream()) == UNSUPPORTED
        torch.cuda.synchronize()
        assert gout.unchanged() and gout.guards_intact() and gin.unchanged()
    assert not B.c2c_line_fits(nl, tdt(dtype)) and B.c2c_line_fits(tc.c2c_longest(dtype), tdt(dtype))


# ---- nk_bluestein_rows -----------------------------------------------------------------------------------------------------
def device_tables(n, m, dtype, inverse):
    """the tables of backend._bluestein_tables on the device, the filter spectrum in natural order on the host, its error"""
    cdt = torch.complex64 if np.dtype(dtype) == np.float32 else torch.complex128
    w, bbr, tw = B._bluestein_tables(n, m, cdt, inverse, torch.device("cuda", torch.cuda.current_device()))
    bhat = bbr.cpu().numpy()[tc.bit_reverse(m)]
    terr = tc.bluestein_table_error(bhat, n, m, inverse)
    assert terr <= tc.host_table_error_ceiling(n, m, dtype, inverse), (n, m, terr)  # the table may not widen its own bound
    return (w, bbr, tw), w.cpu().numpy(), bhat, terr


def run_bluestein(tabs, x, n, m, dtype, scale, in_real, hartley, inplace=False, expect=OK):
    rows = x.size // n if n else 0
    gin = Guarded(x)
    if inplace:
        gout = gin
    else:
        gout = Guarded(np.full(x.shape, np.nan, dtype=dtype if hartley else tc.complex_dtype(dtype)))
    w, bbr, tw = tabs
    rc = L.load().nk_bluestein_rows(rows, n, m, gin.ptr, w.data_ptr(), bbr.data_ptr(), tw.data_ptr(), gout.ptr, float(scale),
                                    int(in_real), int(hartley), code(dtype), stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.load().nk_last_error())
    assert gin.guards_intact() and gout.guards_intact()
    assert inplace or gin.unchanged()
    return gout.get()


def check_bluestein(n, m, dtype, x, inverse, in_real, hartley, scale, inplace=False, mode=""):
    tabs, w, bhat, terr = device_tables(n, m, dtype, inverse)
    xin = np.ascontiguousarray(x.real) if in_real else x
    ref = LD(scale) * tc.fft_ld(xin, 1, inverse)
    if hartley:
        ref = ref.real + hartley * ref.imag
    got = run_bluestein(tabs, xin, n, m, dtype, scale, in_real, hartley, inplace)
    assert not np.isnan(got.view(got.real.dtype)).any()
    bound = tc.bluestein_rel_bound(n, m, dtype, bool(in_real), bool(hartley), inverse, terr)
    e = float(np.max(tc.row_errors(got, ref, xin, n, scale)))
    host = float(np.max(tc.row_errors(tc.bluestein_same_precision(xin, n, m, w, bhat, scale, hartley), ref, xin, n, scale)))
    record("bluestein", dtype, f"{mode}rows{x.shape[0]}/inv{int(inverse)}/real{int(in_real)}/h{hartley}/s{scale}" + ("/inplace" if inplace else ""),
           e, bound, host, n=n, m=m)
    assert host <= bound, (n, m, host, bound)  # the restatement in T on this very input
    assert e <= bound, (n, m, inverse, in_real, hartley, scale, inplace, e, bound)


def bluestein_params():
    return [pytest.param(n, m, d, id=f"{n}-{m}-{np.dtype(d).name}") for d in DTYPES for n, m, only in tc.BLUESTEIN_LENGTHS
            if only is None or np.dtype(only) == np.dtype(d)]


@pytest.mark.parametrize("n,m,dtype", bluestein_params())
def test_bluestein_rows_every_mode(n, m, dtype):
    """forward and inverse tables, complex and real input rows, complex output and both Hartley ends (with scale 0.75), in
    place for complex ends: three normal rows, and the structured rows with exact answers"""
    x = tc.normal_complex((3, n), dtype, 52)
    for inverse in (False, True):
        for in_real in (0, 1):
            for hartley in (0, 1, -1):
                check_bluestein(n, m, dtype, x, inverse, in_real, hartley, 0.75 if hartley else 1.0)
        check_bluestein(n, m, dtype, x, inverse, 0, 0, 1.0, inplace=True)
    # impulses at 0, n / 2, n - 1, the constant, one exponential: the row bound is a bound on every element as well
    check_bluestein(n, m, dtype, tc.structured_rows(n, dtype), False, 0, 0, 1.0, mode="structured/")
    check_bluestein(n, m, dtype, tc.structured_rows(n, dtype), True, 0, -1, 0.75, mode="structured/")
    check_bluestein(n, m, dtype, tc.structured_rows(n, dtype, real=True).astype(tc.complex_dtype(dtype)), False, 1, 1, 0.75, mode="structured/")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", tc.BLUESTEIN_ROW_SWEEPS)
def test_bluestein_rows_partial_row_groups(n, m, dtype):
    """R = 4096 / m rows share a workgroup: fewer rows than R, exactly R, a last group of one row, of three rows"""
    R = 4096 // m
    for rows in (1, R - 1, R, R + 1, 2 * R + 3):
        x = tc.normal_complex((rows, n), dtype, 55)
        check_bluestein(n, m, dtype, x, False, 0, 0, 1.0)
        check_bluestein(n, m, dtype, x, True, 1, -1, 0.75)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bluestein_rows_grid_stride_loop(dtype):
    """more row groups than the 2048 workgroups of the launch"""
    n, m, rows = tc.BLUESTEIN_GRID_STRIDE
    assert 4096 // m == 1 and rows > 256 * 8
    check_bluestein(n, m, dtype, tc.normal_complex((rows, n), dtype, 56), False, 0, 0, 1.0)


def test_bluestein_rows_argument_checks():
    dtype = np.float64
    n, m = 11, 32
    tabs = device_tables(n, m, dtype, False)[0]
    x = tc.normal_complex((2, n), dtype, 57)
    run_bluestein(tabs, x, n, 48, dtype, 1.0, 0, 0, expect=INVALID)        # m not a power of two
    run_bluestein(tabs, x, n, 16, dtype, 1.0, 0, 0, expect=INVALID)        # m < 2 n - 1
    run_bluestein(tabs, x, n, m, dtype, 1.0, 0, 2, expect=INVALID)         # out_hartley outside -1 .. 1
    xr = np.ascontiguousarray(x.real)
    for in_real, hartley in ((1, 0), (0, 1), (1, -1)):                     # real ends in place
        g = Guarded(np.concatenate([xr, xr]))  # room for either end
        w, bbr, tw = tabs
        rc = L.load().nk_bluestein_rows(2, n, m, g.ptr, w.data_ptr(), bbr.data_ptr(), tw.data_ptr(), g.ptr, 1.0, in_real, hartley,
                                        code(dtype), stream())
        torch.cuda.synchronize()
        assert rc == INVALID and g.unchanged() and g.guards_intact()
    for d, big in ((np.float64, 8192), (np.float32, 16384)):               # a row that does not fit 64 KiB
        g, out = Guarded(tc.normal_complex((1, 11), d, 57)), Guarded(np.full((1, 11), np.nan, dtype=tc.complex_dtype(d)))
        w, bbr, tw = tabs  # never read: the size check comes first
        rc = L.load().nk_bluestein_rows(1, 11, big, g.ptr, w.data_ptr(), bbr.data_ptr(), tw.data_ptr(), out.ptr, 1.0, 0, 0, code(d), stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and out.unchanged() and out.guards_intact()
    got = run_bluestein(tabs, x[:0], n, m, dtype, 1.0, 0, 0)               # rows = 0: NK_OK, nothing touched
    assert got.size == 0
    out = Guarded(np.full((2, n), np.nan, dtype=np.complex128))
    w, bbr, tw = tabs
    assert L.load().nk_bluestein_rows(0, n, m, None, w.data_ptr(), bbr.data_ptr(), tw.data_ptr(), out.ptr, 1.0, 0, 0, code(dtype), stream()) == OK
    torch.cuda.synchronize()
    assert out.unchanged() and out.guards_intact()


# ---- nk_cplx_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_cplx_rows_every_mode(dtype):
    """modes 0 / 1 / 2, padding and cropping, w given and NULL, sgn +-1, scale != 1, element by element against long double
    with gamma_3 times the sum of the absolute terms; the padded columns exactly zero."""
    u, cdt, lib = tc.unit_roundoff(dtype), tc.complex_dtype(dtype), L.load()
    rows, scale = 5, 0.75
    worst_all = 0.0
    for mode, in_cols, out_cols, with_w, sgn in [(0, 7, 7, True, 1), (0, 7, 16, True, 1), (0, 16, 7, True, 1), (0, 7, 16, False, 1),
                                                 (0, 300, 300, False, 1), (1, 7, 7, False, 1), (1, 7, 16, True, 1), (1, 16, 7, False, 1),
                                                 (2, 7, 7, False, 1), (2, 7, 7, False, -1), (2, 16, 7, False, -1), (0, 1, 1, True, 1)]:
        a = tc.normal_complex((rows, in_cols), dtype, 58)
        if mode == 1:
            a = np.ascontiguousarray(a.real)
        w = tc.normal_complex((max(in_cols, out_cols),), dtype, 59)
        ga, gw = Guarded(a), Guarded(w)
        out0 = np.full((rows, out_cols), np.nan, dtype=dtype if mode == 2 else cdt)
        gout = Guarded(out0)
        rc = lib.nk_cplx_rows(rows, in_cols, out_cols, ga.ptr, gw.ptr if with_w else None, gout.ptr, mode, scale, sgn, code(dtype), stream())
        torch.cuda.synchronize()
        assert rc == OK, (mode, in_cols, out_cols, lib.nk_last_error())
        assert ga.guards_intact() and gw.guards_intact() and gout.guards_intact() and ga.unchanged() and gw.unchanged()
        got = gout.get()
        k = min(in_cols, out_cols)
        al = a[:, :k].astype(CLD)
        g3, tiny = tc.gamma(3, u), np.finfo(np.float64).tiny
        assert not np.isnan(got.view(got.real.dtype)).any()
        if mode == 2:  # scale (re + sgn im): one addition, one product
            ref = LD(scale) * (al.real + sgn * al.imag)
            parts = [(got[:, :k], ref, tc.gamma(2, u) * abs(scale) * (np.abs(al.real) + np.abs(al.imag)))]
        else:  # each component on its own: scale (re wr - im wi) and scale (re wi + im wr)
            wl = w[:k].astype(CLD) if with_w else np.ones(k, dtype=CLD)
            ref = LD(scale) * al * wl
            tre = abs(scale) * (np.abs(al.real * wl.real) + np.abs(al.imag * wl.imag))
            tim = abs(scale) * (np.abs(al.real * wl.imag) + np.abs(al.imag * wl.real))
            parts = [(got[:, :k].real, ref.real, g3 * tre), (got[:, :k].imag, ref.imag, g3 * tim)]
        for g, r, bnd in parts:
            ok, worst = tc.within_elem(g, r, bnd + tiny)
            worst_all = max(worst_all, worst * (tc.gamma(2, u) / g3 if mode == 2 else 1.0))
            assert ok, (mode, in_cols, out_cols, with_w, sgn, worst)
        assert not got[:, k:].any(), (mode, in_cols, out_cols)
    record("rows", dtype, "every-mode/worst-of-gamma3-terms", worst_all * tc.gamma(3, u), tc.gamma(3, u), 0.0)
    # rows = 0 touches nothing; mode 2 cannot pad; a mode outside 0 .. 2
    gout = Guarded(np.full((2, 4), np.nan, dtype=cdt))
    assert lib.nk_cplx_rows(0, 4, 4, None, None, gout.ptr, 0, 1.0, 1, code(dtype), stream()) == OK
    assert lib.nk_cplx_rows(2, 4, 8, gout.ptr, None, gout.ptr, 2, 1.0, 1, code(dtype), stream()) == INVALID
    assert lib.nk_cplx_rows(2, 4, 4, gout.ptr, None, gout.ptr, 3, 1.0, 1, code(dtype), stream()) == INVALID
    torch.cuda.synchronize()
    assert gout.unchanged() and gout.guards_intact()


# ---- the array seam ------------------------------------------------------------------------------------------------------------
def tdt(dtype, complex_=False):
    if complex_:
        return torch.complex64 if np.dtype(dtype) == np.float32 else torch.complex128
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def chirp_table_error(n, dtype, inverse):
    """table_err of the filter spectrum the composition multiplies with (nk_fftn of the filter, in T, on the device) -- after
    the cached spectrum itself is held to its derived 2-norm bound, so that a wrong table cannot widen its own bound"""
    key = (n, tdt(dtype, True), bool(inverse), torch.cuda.current_device())
    m, w, fb = B._chirps[key]
    fb = fb.cpu().numpy()
    wl, bhat, bmax = tc.bluestein_filter_ld(n, m, inverse)
    assert tc.err_l2c(fb, bhat) <= tc.device_filter_l2_bound(n, m, dtype, inverse), (n, m)
    assert np.max(np.abs(w.cpu().numpy().astype(CLD) - wl)) <= tc._table_mu(dtype, tc.MU_W64)
    terr = tc.bluestein_table_error(fb, n, m, inverse)
    assert terr <= tc.device_filter_l2_bound(n, m, dtype, inverse) / bmax  # (implied: the maximum is below the 2-norm)
    return m, terr


def axis_path(n, dtype, batch, one_launch_allowed):
    if n == 1 or B.plan_supported((n,), tdt(dtype), batch, None, complex=True):
        return "native"
    csize = 8 if np.dtype(dtype) == np.float32 else 16
    return "one-launch" if one_launch_allowed and tc.smallest_m(n) * csize <= B.BLUESTEIN_LDS_BYTES else "composition"


def seam_bound(shape, dtype, inverse, one_launch_allowed, hartley, scale=1.0):
    """the bound of one seam call AFTER it ran (the composition's table is read back from the seam's cache)"""
    u = tc.unit_roundoff(dtype)
    if B.plan_supported(shape, tdt(dtype), 1, None, complex=not hartley):
        if hartley:
            return tc.transform_rel_bound(shape, dtype) + u + 8 * tc.U64, ["native"]
        return tc.c2c_rel_bound(shape, dtype), ["native"]
    total = int(np.prod(shape))
    bounds, paths = [], []
    for d, n in enumerate(shape):
        last = d == len(shape) - 1
        path = axis_path(n, dtype, total // n, one_launch_allowed)
        paths.append(path)
        h = hartley and last
        if path == "native":
            e = tc.c2c_rel_bound((n,), dtype) if n > 1 else 0.0
            bounds.append(np.sqrt(2.0) * (e + 2 * u) if h else e)
        elif path == "one-launch":
            m = tc.smallest_m(n)
            terr = device_tables(n, m, dtype, inverse)[3]
            bounds.append(tc.bluestein_rel_bound(n, m, dtype, hartley and d == 0, h, inverse, terr))
        else:
            m, terr = chirp_table_error(n, dtype, inverse)
            assert m == tc.smallest_m(n)
            bounds.append(tc.composition_rel_bound(n, m, dtype, h, inverse, terr))
    return tc.seam_rel_bound(bounds, dtype, separate_scale=not hartley and scale != 1.0), paths


class Spy:
    """counts the launches of the three ways an axis can go"""

    def __init__(self, monkeypatch):
        self.blu = self.rows = self.fft = 0
        lib = L.load()
        real_blu, real_rows, real_fftn = lib.nk_bluestein_rows, B.cplx_rows, lib.nk_fftn

        def blu(*a):
            self.blu += 1
            return real_blu(*a)

        def rows(*a, **k):
            self.rows += 1
            return real_rows(*a, **k)

        def fftn(*a):
            self.fft += 1
            return real_fftn(*a)

        monkeypatch.setattr(lib, "nk_bluestein_rows", blu)
        monkeypatch.setattr(lib, "nk_fftn", fftn)
        monkeypatch.setattr(B, "cplx_rows", rows)


def path_kind(paths, kind):
    """the record's kind after the path actually taken"""
    if "composition" in paths:
        return "composition"
    if "one-launch" in paths:
        return "bluestein"
    return "hartley" if kind == "hartley" else "c2c"


def seam_call(x, kind, scale):
    xd = torch.from_numpy(x).cuda()
    if kind == "hartley":
        return B.hartley(xd, scale=scale).cpu().numpy()
    return B.fftn(xd, inverse=(kind == "ifft"), scale=scale).cpu().numpy()


def seam_reference(x, kind, scale, sign):
    nd = x.ndim
    if kind == "hartley":
        F = tc.fft_ld(x, nd)
        return LD(scale) * (F.real + sign * F.imag)
    return LD(scale) * tc.fft_ld(x, nd, kind == "ifft")


def host_seam_error(x, kind, scale, sign, ref, ndim=None):
    xc = x.astype(tc.complex_dtype(x.dtype))
    F = tc.fft_same_precision(xc, x.ndim if ndim is None else ndim, kind == "ifft")
    got = (F.real + sign * F.imag) if kind == "hartley" else F
    return tc.err_l2c(np.asarray(got) * x.real.dtype.type(scale), ref) / tc.l2c(ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", tc.SEAM_SHAPES)
def test_seam_with_and_without_the_one_launch_kernel(shape, dtype, monkeypatch):
    """backend.fftn (both directions, scale != 1) and backend.hartley (both conventions, scale != 1) on NUFFT's odd
    oversampled lengths and on shapes that mix native and rejected axes, with NK_BLUESTEIN unset and NK_BLUESTEIN=0: each
    inside its own bound, and the two inside the sum of their bounds of each other."""
    from nifty_amd.nufft import oversampled_length

    assert oversampled_length(31, 4) == 63
    spy = Spy(monkeypatch)
    xc = tc.normal_complex(shape, dtype, 60)
    xr = np.ascontiguousarray(tc.normal_complex(shape, dtype, 61).real)
    for kind, conv, scale in (("fft", None, 1.0), ("ifft", None, 0.5), ("hartley", "non_canonical_hartley", 0.75),
                              ("hartley", "canonical_hartley", 0.75)):
        if conv is not None:
            monkeypatch.setitem(config._config, "hartley_convention", conv)
        sign = -1 if conv == "canonical_hartley" else 1
        x = xr if kind == "hartley" else xc
        ref = seam_reference(x, kind, scale, sign)
        nrm = tc.l2c(ref)
        host = host_seam_error(x, kind, scale, sign, ref)
        res = {}
        for setting in (None, "0"):
            if setting is None:
                monkeypatch.delenv("NK_BLUESTEIN", raising=False)
            else:
                monkeypatch.setenv("NK_BLUESTEIN", setting)
            spy.blu = spy.rows = 0
            got = seam_call(x, kind, scale)
            assert not np.isnan(got.view(got.real.dtype)).any()
            bound, paths = seam_bound(shape, dtype, kind == "ifft", setting is None, kind == "hartley", scale)
            assert (spy.blu > 0) == ("one-launch" in paths) and (setting is None or spy.blu == 0), (paths, spy.blu)
            assert ("composition" in paths) <= (spy.rows > 0)
            e = tc.err_l2c(got, ref) / nrm
            record(path_kind(paths, kind), dtype, f"seam/{kind}/{conv or '-'}/s{scale}/{'+'.join(paths)}", e, bound, host, shape=shape)
            assert host <= bound, (kind, paths, host, bound)  # scipy.fft in T on this very input
            assert e <= bound, (kind, conv, setting, paths, e, bound)
            res[setting] = (got, bound)
        d = tc.err_l2c(res[None][0], res["0"][0].astype(CLD)) / nrm
        assert d <= res[None][1] + res["0"][1], (kind, d)


def seam_length_params():
    return [pytest.param(n, path, d, id=f"{n}-{path}-{np.dtype(d).name}") for d in DTYPES
            for n, path in [(2048 if np.dtype(d) == np.float64 else 4096, "native")] + tc.SEAM_LENGTHS[np.dtype(d)]]


@pytest.mark.parametrize("n,path,dtype", seam_length_params())
def test_seam_hand_over_and_longest_lengths(n, path, dtype, monkeypatch):
    """The hand-over from the one-launch kernel to the composition at the 64 KiB row (2047 | 2048 native | 2049 in fp64,
    4095 | 4096 | 4097 in fp32) and the longest rejected length the fallback serves (fp64: 4095, m = 8192 is the longest
    power of two nk_fftn takes; fp32: 8191, m = 16384 is the seam's own cap): each run takes the path named here."""
    monkeypatch.delenv("NK_BLUESTEIN", raising=False)
    spy = Spy(monkeypatch)
    assert axis_path(n, dtype, 2, True) == path
    xc = tc.normal_complex((2, n), dtype, 62)
    xr = np.ascontiguousarray(xc.real)
    for kind, x, scale in (("fft", xc, 1.0), ("hartley", xr, 0.75)):
        spy.blu = spy.rows = spy.fft = 0
        xd = torch.from_numpy(x).cuda()
        got = (B.hartley(xd, ndim=1, scale=scale) if kind == "hartley" else B.fftn(xd, ndim=1)).cpu().numpy()
        F = tc.fft_ld(x, 1)
        ref = LD(scale) * (F.real + F.imag) if kind == "hartley" else F
        if path == "native":
            assert spy.blu == 0 and spy.rows == 0
            bound = (tc.transform_rel_bound((n,), dtype) + tc.unit_roundoff(dtype) + 8 * tc.U64) if kind == "hartley" else tc.c2c_rel_bound((n,), dtype)
        elif path == "one-launch":
            assert spy.blu == 1 and spy.rows == 0 and spy.fft == 0
            m = tc.smallest_m(n)
            bound = tc.bluestein_rel_bound(n, m, dtype, kind == "hartley", kind == "hartley", False, device_tables(n, m, dtype, False)[3])
        else:
            assert spy.blu == 0 and spy.fft >= 2 and spy.rows >= 3
            m, terr = chirp_table_error(n, dtype, False)
            bound = tc.composition_rel_bound(n, m, dtype, kind == "hartley", False, terr)
        e = tc.err_l2c(got, ref) / tc.l2c(ref)
        host = host_seam_error(x, kind, scale, 1, ref, ndim=1)
        record(path_kind([path], kind), dtype, f"seam/{kind}/{path}", e, bound, host, n=n, m=0 if path == "native" else tc.smallest_m(n))
        assert host <= bound, (kind, path, host, bound)
        assert e <= bound, (kind, path, e, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_refuses_by_naming_the_axis_length(dtype, monkeypatch):
    """One past the longest served length, and a 7-smooth even length between the limit of the c2c kernel and the limit of
    the Hartley planner (fp64: 10 000, fp32: 20 000): the call raises NotImplementedError whose text names the axis
    length, whichever internal transform would have refused, and nothing of the padded length was built before."""
    monkeypatch.delenv("NK_BLUESTEIN", raising=False)
    f64 = np.dtype(dtype) == np.float64
    past, between = (4097, 10000) if f64 else (8193, 20000)
    assert between + between // 16 + 1 > tc.c2c_line_limit(dtype) >= between // 2 + between // 32 + 1
    assert B.plan_supported((between,), tdt(dtype)) and not B.plan_supported((between,), tdt(dtype), complex=True)
    spy = Spy(monkeypatch)
    plans_before = set(B._plans)
    for n in (past, between):
        z = torch.zeros(n, dtype=tdt(dtype, True), device="cuda")
        calls = [lambda: B.fftn(z), lambda: B.fftn(z, inverse=True, scale=0.5)]
        if n == past:  # (the REAL transform of the length in between is native: below)
            calls.append(lambda: B.hartley(torch.zeros(n, dtype=tdt(dtype), device="cuda")))
        for call in calls:
            with pytest.raises(NotImplementedError, match=str(n)):
                call()
        assert spy.blu == 0 and spy.rows == 0 and spy.fft == 0
        assert set(B._plans) == plans_before  # no plan of the padded length either: the refusal is host arithmetic
        cdt = tdt(dtype, True)  # (the other precision may have served this length in another test)
        assert all(k[:2] != (n, cdt) for k in B._chirps) and all((k[0], k[2]) != (n, cdt) for k in B._blu_tables)
    # ... while the real transform of the length in between is the planner's own
    x = np.ascontiguousarray(tc.normal_complex((between,), dtype, 63).real)
    got = B.hartley(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = tc.hartley_ld(x, 1)
    assert spy.blu == 0 and spy.rows == 0
    assert tc.err_l2(got, ref) <= tc.transform_rel_bound((between,), dtype) * tc.l2(ref) + tc.store_term(ref, dtype)
    # and a mixed shape whose LAST axis only the complex side refuses names that axis too
    with pytest.raises(NotImplementedError, match=str(between)):
        B.hartley(torch.zeros((11, between), dtype=tdt(dtype), device="cuda"))
