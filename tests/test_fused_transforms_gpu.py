"""nk_hartley / nk_hartley_fused / nk_hartley_sandwich called directly through the C ABI on every route of the planner,
against long-double transforms with DERIVED bounds (tests/transform_cases.py: reference, derivation, comparators).

Every test asserts nk_plan_route for its shape and dtype (a planner change must fail here, not quietly test another
route), puts every operand, output and the workspace -- a slice of exactly nk_plan_workspace_bytes -- between guard bands
of NaN (all-ones bytes), checks the bands bit-wise afterwards, that no NaN reached an output, and that every array the
call may only read is unchanged.  Every case prints one line `ERR route class dtype error bound host-error` (the host
error: scipy.fft in T on the same transform input); profiles/r08_fused_transform_errors.txt keeps one run's lines."""
import ctypes

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from tests import transform_cases as tc

pytestmark = pytest.mark.gpu

LD = np.longdouble
GUARD = 4096  # bytes on either side
DTYPES = [np.float64, np.float32]
ALL_SHAPES = [s for s, _, _ in tc.ROUTES]


class Guarded:
    """`arr` on the device between two guard bands of all-ones bytes (NaN as fp32 and fp64, -1 as an index)."""

    def __init__(self, arr=None, nbytes=None):
        self.arr = None if arr is None else np.ascontiguousarray(arr)
        self.nbytes = self.arr.nbytes if nbytes is None else int(nbytes)
        self.buf = torch.full((2 * GUARD + self.nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        if self.arr is not None:
            self.buf[GUARD:GUARD + self.nbytes] = torch.from_numpy(self.arr.reshape(-1).view(np.uint8).copy()).cuda()
        self.ptr = self.buf.data_ptr() + GUARD

    def guards_intact(self):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.nbytes:]
        return bool((lo == 0xFF).all().item() and (hi == 0xFF).all().item())

    def get(self):
        raw = self.buf[GUARD:GUARD + self.nbytes].cpu().numpy()
        return raw.view(self.arr.dtype).reshape(self.arr.shape)

    def unchanged(self):
        return np.array_equal(self.get().reshape(-1).view(np.uint8), self.arr.reshape(-1).view(np.uint8))


class PlanH:
    def __init__(self, shape, dtype, batch=1):
        self.lib = L.load()
        self.shape, self.dtype, self.batch = tuple(shape), np.dtype(dtype), batch
        self.p = ctypes.c_void_p()
        shp = (ctypes.c_int64 * len(shape))(*shape)
        L.check(self.lib.nk_plan_create(ctypes.byref(self.p), len(shape), shp, L.NK_F32 if self.dtype == np.float32 else L.NK_F64,
                                        batch), "nk_plan_create")
        r = (ctypes.c_int * 4)()
        L.check(self.lib.nk_plan_route(self.p, r), "nk_plan_route")
        self.route = tuple(r)
        self.ws_bytes = int(self.lib.nk_plan_workspace_bytes(self.p))
        self.octant = bool(self.lib.nk_plan_octant_vjp(self.p))
        self.sandwich = bool(self.lib.nk_plan_sandwich(self.p))

    def workspace(self):
        return Guarded(nbytes=self.ws_bytes)  # the slice itself pre-filled with NaN as well

    def close(self):
        self.lib.nk_plan_destroy(self.p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def assert_route(plan, shape, dtype):
    want = tc.route_of(shape, dtype)
    assert plan.route == want, f"planner changed: {shape} {np.dtype(dtype).name} runs route {plan.route}, this test is for {want}"
    assert plan.octant == (want[0] == 2)
    pow2 = all(64 <= n <= 4096 and n & (n - 1) == 0 for n in shape)
    assert plan.sandwich == (want[0] == 2 and pow2 and shape[-1] >= 128)
    assert bool(plan.lib.nk_plan_batch_ok(plan.p)) == (want[0] == 2 and len(shape) == 2 and plan.batch == 1)


def stream():
    return torch.cuda.current_stream().cuda_stream


def record(plan, cls, dtype, err, bound, host):
    print(f"ERR shape={'x'.join(map(str, plan.shape))} route={','.join(map(str, plan.route))} class={cls} dtype={np.dtype(dtype).name} err={err:.3e} bound={bound:.3e} "
          f"host={host:.3e}")


def host_rel_error(x, ndim, sign=1):
    """relative 2-norm error of scipy.fft run in the dtype of x on the same transform input"""
    ref = tc.hartley_ld(x, ndim, sign)
    return tc.err_l2(tc.hartley_same_precision(x, ndim, sign), ref) / max(tc.l2(ref), 1e-300)


# ---- plain nk_hartley -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_plain_hartley_on_every_route(shape, dtype):
    """nk_hartley in place and out of place, batch 1 and 2, both conventions, scale != 1."""
    nd = len(shape)
    x2 = np.random.default_rng(21).normal(size=(2,) + shape).astype(dtype)
    scale = 0.75
    refs = {sign: LD(scale) * tc.hartley_ld(x2, nd, sign) for sign in (1, -1)}
    host = host_rel_error(x2[0], nd)
    for batch in (1, 2):
        with PlanH(shape, dtype, batch) as plan:
            assert_route(plan, shape, dtype)
            rel = tc.transform_rel_bound(shape, dtype, plan.route)
            x = x2[:batch]
            for conv, sign in ((0, 1), (1, -1)):
                ref = refs[sign][:batch]
                bound = rel * tc.l2(ref) + tc.store_term(ref, dtype)
                for inplace in (False, True):
                    gin, ws = Guarded(x), plan.workspace()
                    gout = gin if inplace else Guarded(np.full_like(x, np.nan))
                    L.check(plan.lib.nk_hartley(plan.p, gin.ptr, gout.ptr, scale, conv, ws.ptr, stream()), "nk_hartley")
                    torch.cuda.synchronize()
                    got = gout.get()
                    tag = (batch, conv, inplace)
                    assert gin.guards_intact() and gout.guards_intact() and ws.guards_intact(), tag
                    assert inplace or gin.unchanged(), tag
                    assert not np.isnan(got).any(), tag
                    ok, e = tc.within_l2(got, ref, bound)
                    record(plan, f"hartley/b{batch}/c{conv}/{'in' if inplace else 'out'}place", dtype, e / tc.l2(ref),
                           bound / tc.l2(ref), host)
                    assert ok, (tag, e, bound)
                    # the suite's earlier max-norm bar stays in force beside the derived bound
                    assert np.max(np.abs(got - ref)) < (1e-12 if np.dtype(dtype) == np.float64 else 3e-5) * np.max(np.abs(ref)), tag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_impulses_element_by_element(shape, dtype):
    """A unit impulse gives scale * cas(2 pi sum k_d p_d / n_d): one chain of twiddle products per output element, so an
    index permutation or a single bad twiddle shows element by element.  The impulse sits in the second member of a
    batch of two (the first member must come out as exact zeros); positions: tc.impulse_positions."""
    nd = len(shape)
    scale = 1.5
    with PlanH(shape, dtype, 2) as plan:
        assert_route(plan, shape, dtype)
        bound = scale * tc.impulse_elem_bound(shape, dtype, plan.route)
        worst_all = 0.0
        for i, p in enumerate(tc.impulse_positions(shape)):
            conv, sign = ((0, 1), (1, -1))[i % 2]
            x = np.zeros((2,) + shape, dtype=dtype)
            x[(1,) + p] = 1.0
            gin, gout, ws = Guarded(x), Guarded(np.full_like(x, np.nan)), plan.workspace()
            L.check(plan.lib.nk_hartley(plan.p, gin.ptr, gout.ptr, scale, conv, ws.ptr, stream()), "nk_hartley")
            torch.cuda.synchronize()
            got = gout.get()
            assert gin.guards_intact() and gout.guards_intact() and ws.guards_intact() and gin.unchanged(), p
            assert not np.isnan(got).any(), p
            assert not got[0].any(), p
            ok, worst = tc.within_elem(got[1], LD(scale) * tc.impulse_reference(shape, p, sign), bound)
            worst_all = max(worst_all, worst)
            assert ok, (p, conv, worst)
        x = np.zeros(shape, dtype=dtype)
        x[tc.impulse_positions(shape)[-1]] = 1.0
        host = float(np.max(np.abs(tc.hartley_same_precision(x, nd) - tc.impulse_reference(shape, tc.impulse_positions(shape)[-1]))))
        record(plan, "impulse/elementwise", dtype, worst_all * bound, bound, host)


# ---- fused classes ----------------------------------------------------------------------------------------------------
def run_case(plan, case, sign, cls, use_ws=True, sandwich_first=None):
    """One nk_hartley_fused (or nk_hartley_sandwich) call of `case` with guards; returns the outputs after the call."""
    bufs = {k: Guarded(v) for k, v in list(case.inputs.items()) + list(case.outputs.items())}
    f = case.fill(L.Fuse(), lambda k: bufs[k].ptr)
    ws = plan.workspace()
    wsp = ws.ptr if use_ws else None
    conv = 0 if sign == 1 else 1
    if sandwich_first is None:
        L.check(plan.lib.nk_hartley_fused(plan.p, ctypes.byref(f), conv, wsp, stream()), "nk_hartley_fused " + cls)
    else:
        L.check(plan.lib.nk_hartley_sandwich(plan.p, ctypes.byref(f), sandwich_first, conv, wsp, stream()), "nk_hartley_sandwich " + cls)
    torch.cuda.synchronize()
    assert ws.guards_intact(), cls
    for k, g in bufs.items():
        assert g.guards_intact(), (cls, k)
        if k in case.inputs:
            assert g.unchanged(), (cls, k)
    got = {k: bufs[k].get() for k in case.outputs}
    for k, v in got.items():
        assert not np.isnan(v).any(), (cls, k)
    return got, bufs


def check_case(plan, case, sign, cls, rel, **kw):
    got, _ = run_case(plan, case, sign, cls, **kw)
    # energy / curvature sums: slots and fixed-order folds with a workspace, one atomic per workgroup without (1-D: one
    # workgroup per batch member)
    depth = tc.reduction_depth(plan.ws_bytes) if kw.get("use_ws", True) else tc.reduction_depth(None, atomics=plan.batch)
    ref = case.reference(sign, rel, depth)
    rows = tc.compare(case, ref, got)
    x = case.transform_input(sign)
    host = host_rel_error(x, len(case.shape), sign)
    for name, e, b, ok in rows:
        if ref[name][1] == "l2":
            nrm = max(tc.l2(ref[name][0]), 1e-300)
            e, b = e / nrm, b / nrm
        record(plan, f"{cls}/{name}", case.dtype, e, b, host)
    assert all(r[3] for r in rows), (cls, rows)
    return got


def class_params():
    return [pytest.param(s, d, id=f"{'x'.join(map(str, s))}-{np.dtype(d).name}") for s in tc.CLASS_SHAPES for d in DTYPES]


@pytest.mark.parametrize("shape,dtype", class_params())
def test_every_prologue_with_the_affine_epilogue(shape, dtype):
    with PlanH(shape, dtype) as plan:
        assert_route(plan, shape, dtype)
        rel = tc.transform_rel_bound(shape, dtype, plan.route)
        for i, pro in enumerate(tc.PROLOGUES + (tc.PROLOGUES_OCTANT if plan.octant else [])):
            case = tc.FusedCase(shape, dtype, pro, "affine", plan.octant, seed=31)
            check_case(plan, case, 1 if i % 2 == 0 else -1, f"{pro}->affine", rel)


@pytest.mark.parametrize("shape,dtype", class_params())
def test_every_epilogue_with_the_plain_prologue(shape, dtype):
    with PlanH(shape, dtype) as plan:
        assert_route(plan, shape, dtype)
        rel = tc.transform_rel_bound(shape, dtype, plan.route)
        for i, epi in enumerate(tc.EPILOGUES):
            case = tc.FusedCase(shape, dtype, "plain", epi, plan.octant, seed=32)
            check_case(plan, case, 1 if i % 2 == 0 else -1, f"plain->{epi}", rel)
        if len(shape) == 1:  # 1-D calls may omit the workspace: the energy then goes through atomics
            for epi in ("lh_gauss_id", "lh_poisson_exp"):
                case = tc.FusedCase(shape, dtype, "plain", epi, plan.octant, seed=33)
                check_case(plan, case, 1, f"plain->{epi}/no-workspace", rel, use_ws=False)


@pytest.mark.parametrize("shape,dtype", class_params())
def test_vjp_epilogue_variants(shape, dtype):
    """abar by atomics, eight private accumulators + nk_fold_copies, addend / accumulate / value, carry1 / carry2, the
    octant sums w8 (+ w8max in 3-D) on octant plans, wfull on the others (hybrids included)."""
    with PlanH(shape, dtype) as plan:
        assert_route(plan, shape, dtype)
        rel = tc.transform_rel_bound(shape, dtype, plan.route)
        for i, epi in enumerate(tc.VJPS + (["vjp_w8"] if plan.octant else ["vjp_wfull"])):
            case = tc.FusedCase(shape, dtype, "plain", epi, plan.octant, seed=34)
            sign = 1 if i % 2 == 0 else -1
            got = check_case(plan, case, sign, f"plain->{epi}", rel)
            if epi == "vjp_copies8":  # the device's own fold of the eight accumulators
                src = torch.from_numpy(got["abar"]).cuda()
                dst = torch.full((case.nb + 1,), float("nan"), dtype=torch.float64, device="cuda")
                L.check(plan.lib.nk_fold_copies(case.nb + 1, 8, case.stride, src.data_ptr(), dst.data_ptr(), stream()), "nk_fold_copies")
                torch.cuda.synchronize()
                ref, _, bound = case.reference(sign, rel)["abar_bins"]
                assert np.all(np.abs(dst.cpu().numpy().astype(LD) - ref) <= bound)


ENGINE_PAIRS = [("amp_afield", "lh_gauss_exp"), ("jvp_afield_dampT", "mul_field"), ("mul", "vjp_atomic")]


@pytest.mark.parametrize("shape,dtype", class_params())
def test_the_pairs_the_engine_launches(shape, dtype):
    with PlanH(shape, dtype) as plan:
        assert_route(plan, shape, dtype)
        rel = tc.transform_rel_bound(shape, dtype, plan.route)
        for i, (pro, epi) in enumerate(ENGINE_PAIRS):
            if plan.octant and pro.endswith("afield"):
                pro = {"amp_afield": "amp_afield_oct", "jvp_afield_dampT": "jvp_dafield_oct"}[pro]
            case = tc.FusedCase(shape, dtype, pro, epi, plan.octant, seed=35)
            check_case(plan, case, 1 if i % 2 == 0 else -1, f"{pro}->{epi}", rel)


# ---- sandwich H D H ---------------------------------------------------------------------------------------------------
def sandwich_params():
    return [pytest.param(s, d, id=f"{'x'.join(map(str, s))}-{np.dtype(d).name}") for s, only in tc.SANDWICH for d in DTYPES
            if only is None or np.dtype(only) == np.dtype(d)]


@pytest.mark.parametrize("shape,dtype", sandwich_params())
def test_sandwich_plain_affine(shape, dtype):
    """nk_hartley_sandwich PLAIN -> AFFINE with the scalar and with a field diagonal against the long-double H D H."""
    nd, n = len(shape), float(np.prod(shape))
    rng = np.random.default_rng(41)
    x, m = rng.normal(size=shape).astype(dtype), rng.normal(size=shape).astype(dtype)
    sf, ms, scale, offset = 0.5 / np.sqrt(n), 1.5, 2.0 / np.sqrt(n), 0.75
    u = tc.unit_roundoff(dtype)
    with PlanH(shape, dtype) as plan:
        assert plan.route == (2, 1, 1 if nd == 3 else -1, 1) and plan.sandwich
        host = host_rel_error(x, nd)
        for i, mul in enumerate((None, m)):
            conv, sign = ((0, 1), (1, -1))[i]
            # composed twiddles of the fused first-axis pass only where the library can take that build (both transforms
            # of the sandwich go through it)
            rel = tc.transform_rel_bound(shape, dtype, plan.route, tc.sandwich_composed_axis(shape, dtype, mul is not None))
            t1 = tc.hartley_ld(x, nd, sign)
            d = LD(ms * sf) * (LD(1) if mul is None else mul.astype(LD))
            mid = d * t1
            ref = LD(scale) * tc.hartley_ld(mid, nd, sign) + LD(offset)
            e_mid = float(np.max(np.abs(d))) * rel * tc.l2(t1) + tc.gamma(3, u) * tc.l2(mid)
            bound = abs(scale) * np.sqrt(n) * ((1 + rel) * e_mid + rel * tc.l2(mid)) + tc.store_term(ref, dtype)
            gin, gout, ws = Guarded(x), Guarded(np.full_like(x, np.nan)), plan.workspace()
            gm = Guarded(m)
            f = L.Fuse()
            f.in_, f.out, f.scale, f.offset, f.mul_scalar = gin.ptr, gout.ptr, scale, offset, ms
            if mul is not None:
                f.mul = gm.ptr
            L.check(plan.lib.nk_hartley_sandwich(plan.p, ctypes.byref(f), sf, conv, ws.ptr, stream()), "nk_hartley_sandwich")
            torch.cuda.synchronize()
            got = gout.get()
            assert gin.guards_intact() and gout.guards_intact() and ws.guards_intact() and gm.guards_intact()
            assert gin.unchanged() and gm.unchanged()
            assert not np.isnan(got).any()
            ok, e = tc.within_l2(got, ref, bound)
            record(plan, f"sandwich/plain->affine/{'field' if mul is not None else 'scalar'}", dtype, e / tc.l2(ref),
                   bound / tc.l2(ref), host)
            assert ok, (i, e, bound)


# (1024, 64, 128) and (64, 1024, 128) are in the table for the builds of the MIDDLE passes (MidCfg::TWO, SchedW), which the
# plain sandwich above runs; the octant classes live in the first and the final pass, whose kernels do not depend on those
# builds, and three long-double references of 8 M points per class would take a test far beyond a few seconds
OCTANT_SANDWICH_SHAPES = [(64, 128), (64, 64, 128), (64, 64, 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OCTANT_SANDWICH_SHAPES)
def test_sandwich_octant_metric_application(shape, dtype):
    """The metric application J^T M J as one call: octant AMP_JVP prologue (da as an octant field; da gathered from its
    table through pidx_octant; the pending CG direction update cg_r / cg_scal written back to `in`), scalar and field
    diagonal, octant VJP epilogue with w8 (+ w8max in 3-D), addend, accumulation and the curvature sum `value`."""
    n = float(np.prod(shape))
    with PlanH(shape, dtype) as plan:
        assert plan.route == (2, 1, 1 if len(shape) == 3 else -1, 1) and plan.sandwich and plan.octant
        for i, (pro, field) in enumerate((("jvp_dafield_oct", False), ("jvp_pidxoct_oct", True), ("jvp_cg_oct", False))):
            sf = 0.5 / np.sqrt(n)
            rel = tc.transform_rel_bound(shape, dtype, plan.route, tc.sandwich_composed_axis(shape, dtype, field))
            case = tc.FusedCase(shape, dtype, pro, "vjp_w8", True, seed=42, sandwich=(sf, 0.7, field))
            case.outputs["value"] = np.array([0.25])
            check_case(plan, case, 1 if i % 2 == 0 else -1, f"sandwich/{pro}->vjp_w8/{'field' if field else 'scalar'}", rel,
                       sandwich_first=sf)


@pytest.mark.parametrize("shape", [(64, 128), (64, 64, 64)])
def test_io32_forward(shape):
    """nk_fuse.io32: float excitations, data and outputs around an fp64 transform (AMP prologue with an fp64 octant field,
    LIKELIHOOD epilogue): bounds of the fp64 transform, ONE rounding of the outputs to float."""
    dtype = np.float64
    with PlanH(shape, dtype) as plan:
        assert_route(plan, shape, dtype)
        rel = tc.transform_rel_bound(shape, dtype, plan.route)
        for i, epi in enumerate(("lh_gauss_id", "lh_gaussf_exp", "lh_poisson_exp")):
            case = tc.FusedCase(shape, dtype, "amp_afield_oct", epi, True, seed=43, io32=True)
            assert case.inputs["in"].dtype == np.float32 and case.outputs["out"].dtype == np.float32
            check_case(plan, case, 1 if i % 2 == 0 else -1, f"io32/amp_afield_oct->{epi}", rel)
