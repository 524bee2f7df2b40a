"""nk_hartley_fused_batch called directly through the C ABI, kernel class by kernel class, against the long-double
references and DERIVED bounds of tests/transform_cases.py (nothing here introduces a tolerance) and, bit for bit, against
one nk_hartley_fused call per member on fresh buffers (the contract of include/niftyk.h, "batched launches").

A batch of `count` members with count >= 2 does not run the kernels tests/test_fused_transforms_gpu.py pins: a plan with
nk_plan_batch_ok and both axes >= 512 runs separate instantiations, the BATCHED TWINS, whose second grid dimension walks
the members --

    first pass   k2_strided_b (nk_fft_b.hip)   N = 512, 1024, 2048, 4096 x prologue class PLAIN (0), octant AMP (4),
                                               octant AMP_JVP (5), MUL (6)
                 k2_tl_b (nk_fft_t.hip)        the two launches of the two-level first axis: 4096 points in fp64
    final pass   k2_final_b (nk_fft_b.hip)     NL = 512 .. 4096 x epilogue class MUL (1), LIKELIHOOD (3), run-time generic
                                               (-1: NONLIN), VJP with an amplitude field on line couples (2) and, where
                                               the couple tile exceeds 60 KiB of LDS (nk_final_single_2d: 2048 and 4096
                                               points in fp64, 4096 in fp32), the VJP on single line pairs
    slots        k_zero_slots_b, k_fold_slots_a_b, k_fold_slots_b_b (nk_fft.hip): the energy / curvature sums per member

-- and every other class, plan or count 1 runs member by member.  Which twin a shape of tc.BATCH_SHAPES covers:

    (512, 512)                  N = NL = 512
    (1024, 512), (512, 1024)    N = 1024 / NL = 1024
    (2048, 512), (512, 2048)    N = 2048 / NL = 2048 (fp64: single-pair VJP)
    (4096, 512)                 N = 4096: k2_tl_b in fp64 (route first == 2), k2_strided_b<4096> in fp32 (first == 1)
    (512, 4096)                 NL = 4096: single-pair VJP in both dtypes

The records of CHAINS together reach all eight twin classes; nk_plan_batch_class_ok (host only) proves that a call took the
shared launches -- nk_profile_collect cannot, it counts a batched launch with weight `count`.

Every call: operands, outputs and every member's workspace -- a slice of exactly nk_plan_workspace_bytes -- sit between
guard bands of all-ones bytes, checked bit-wise afterwards; every array the call may only read is unchanged; no NaN in
an output; every member within the bounds of case.reference through tc.compare; every member bit-identical to its single
call.  ONE exemption from the bit equality, by construction and not by measurement: a VJP epilogue without w8 adds to
`abar` with atomics, whose order is free (tc: "the atomically accumulated abar has no fixed order") -- two single calls
do not agree in the last bit either; such an abar is held to its reference bound only.

One line per class and output, `ERR shape route class dtype error bound host-error` of the member closest to its bound
(host: scipy.fft in T on member 0's prologue output rounded to T, against the long-double transform);
profiles/r10_batched_transform_errors.txt keeps one run's lines."""
import ctypes
import time

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from tests import transform_cases as tc
from tests.test_fused_transforms_gpu import DTYPES, Guarded, PlanH, assert_route, record, run_case, stream

pytestmark = pytest.mark.gpu

SHAPES = [s for s, _, _ in tc.BATCH_SHAPES]
BASE = (512, 512)
CHAINS = [("amp_afield_oct", "lh_gauss_exp"), ("jvp_dafield_oct", "mul_field"), ("mul", "vjp_w8"), ("mul", "vjp_addend_acc"),
          ("plain", "nonlin_sigmoid")]  # PC 4 EC 3 | PC 5 EC 1 | PC 6 EC 2 (twice: w8; atomics + value) | PC 0 EC -1


CLOCK = {"calls": 0, "device_ms": 0.0, "single_s": 0.0}


@pytest.fixture(scope="module", autouse=True)
def clock():
    """`TIME` line at the end of the module: its wall time, the device time of the batched calls themselves (events
    around nk_hartley_fused_batch) and the wall time of the single calls with their transfers; the rest is the host's
    (operands, long-double references, comparisons, transfers of the batched buffers)"""
    t0 = time.perf_counter()
    yield
    print(f"\nTIME module wall={time.perf_counter() - t0:.1f}s batched_calls={CLOCK['calls']} batched_device={CLOCK['device_ms'] / 1e3:.3f}s "
          f"single_calls_with_transfers={CLOCK['single_s']:.1f}s")


def vary(case, m):
    """Member m gets its own value of every scalar its class reads (a twin that took them from member 0 would differ
    from the reference at once).  Steps of 1/32 keep s = t + offset of the Poisson cases positive."""
    S = case.set
    case.scale *= 1.0 + 0.03125 * m
    if S["epi"] in (L.EPI_NONLIN, L.EPI_LIKELIHOOD, L.EPI_AFFINE):
        case.offset += 0.0625 * m
    for k, step in (("mul_scalar", -0.25), ("addend_scale", 0.5), ("icov_scalar", 0.25)):
        if k in S:
            S[k] += step * m
    S["scale"], S["offset"] = case.scale, case.offset
    return case


def make_cases(shape, dtype, pro, epi, count, seed=700, **kw):
    return [vary(tc.FusedCase(shape, dtype, pro, epi, True, seed=seed + m, **kw), m) for m in range(count)]


def class_rule(plan, f):
    """What nk_plan_batch_class_ok must say, from the record's fields by the rule of its header comment."""
    pro_ok = f.pro in (L.PRO_PLAIN, L.PRO_MUL) or (f.pro in (L.PRO_AMP, L.PRO_AMP_JVP) and bool(f.field_octant) and not f.io32)
    epi_ok = (f.epi in (L.EPI_MUL, L.EPI_NONLIN) or (f.epi == L.EPI_LIKELIHOOD and not f.io32) or
              (f.epi == L.EPI_VJP and bool(f.afield)))
    return int(bool(plan.lib.nk_plan_batch_ok(plan.p)) and min(plan.shape) >= 512 and pro_ok and epi_ok)


def atomic_abar(case):
    return "abar" in case.outputs and "w8" not in case.outputs and "wfull" not in case.outputs


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Batch:
    """The device side of ONE nk_hartley_fused_batch call: guarded buffers of every member (`shared`: operand names all
    members pass the SAME pointer for), the record array, one guarded workspace per member."""

    def __init__(self, plan, cases, shared=()):
        self.plan, self.cases = plan, cases
        self.bufs, common = [], {}
        for case in cases:
            b = {}
            for k, v in list(case.inputs.items()) + list(case.outputs.items()):
                if k in shared:
                    assert k in case.inputs and v is cases[0].inputs[k]
                    b[k] = common.setdefault(k, Guarded(v))
                else:
                    b[k] = Guarded(v)
            self.bufs.append(b)
        self.fuses = (L.Fuse * len(cases))()
        for m, case in enumerate(cases):
            case.fill(self.fuses[m], lambda k, m=m: self.bufs[m][k].ptr)
        self.ws = [plan.workspace() for _ in cases]

    def query(self, m=0):
        lib, f = self.plan.lib, self.fuses[m]
        q = lib.nk_plan_batch_class_ok(self.plan.p, ctypes.byref(f))
        assert q == class_rule(self.plan, f), (self.cases[m].pro, self.cases[m].epi, q)
        return q

    def call(self, sign, count=None, ws_ptrs=None):
        """-> nk_status; count / ws_ptrs: the argument checks pass their own"""
        n = len(self.cases) if count is None else count
        ptrs = [w.ptr for w in self.ws] if ws_ptrs is None else ws_ptrs
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = self.plan.lib.nk_hartley_fused_batch(self.plan.p, self.fuses, n, 0 if sign == 1 else 1, arr, stream())
        t1.record()
        torch.cuda.synchronize()
        CLOCK["calls"] += 1
        CLOCK["device_ms"] += t0.elapsed_time(t1)
        return rc

    def guards(self, tag):
        for m, (case, b) in enumerate(zip(self.cases, self.bufs)):
            assert self.ws[m].guards_intact(), (tag, m, "workspace")
            for k, g in b.items():
                assert g.guards_intact(), (tag, m, k)
                if k in case.inputs:
                    assert g.unchanged(), (tag, m, k)

    def outputs(self, tag):
        self.guards(tag)
        gots = [{k: b[k].get() for k in case.outputs} for case, b in zip(self.cases, self.bufs)]
        for m, got in enumerate(gots):
            for k, v in got.items():
                assert not np.isnan(v).any(), (tag, m, k)
        return gots

    def untouched(self, tag):
        self.guards(tag)
        for m, (case, b) in enumerate(zip(self.cases, self.bufs)):
            for k in case.outputs:
                assert b[k].unchanged(), (tag, m, k)


def host_error(case, sign):
    """scipy.fft in T on the prologue's output rounded to T against the long-double transform of the case (whose spectrum
    the reference has computed already)"""
    x = case.transform_input(sign)
    ref = case._spectrum.real + sign * case._spectrum.imag
    return tc.err_l2(tc.hartley_same_precision(x, len(case.shape), sign), ref) / max(tc.l2(ref), 1e-300)


class Pinned:
    """reference and single-call outputs of a case, computed once per convention and shared by every batch it is a member of"""

    def __init__(self, plan, rel):
        self.plan, self.rel, self.depth = plan, rel, tc.reduction_depth(plan.ws_bytes)
        self.refs, self.singles = {}, {}

    def ref(self, case, sign):
        key = (id(case), sign)
        if key not in self.refs:
            self.refs[key] = (case, case.reference(sign, self.rel, self.depth))
        return self.refs[key][1]

    def single(self, case, sign, cls):
        """one nk_hartley_fused call of the case on fresh guarded buffers (run_case checks its guards, inputs and NaN)"""
        key = (id(case), sign)
        if key not in self.singles:
            t0 = time.perf_counter()
            self.singles[key] = (case, run_case(self.plan, case, sign, cls + "/single")[0])
            CLOCK["single_s"] += time.perf_counter() - t0
        return self.singles[key][1]


def run_and_check(plan, cases, sign, cls, pinned, want_query=None, shared=()):
    """One batched call of `cases` with every check of the module docstring; -> what nk_plan_batch_class_ok said."""
    batch = Batch(plan, cases, shared)
    q = batch.query()
    assert all(batch.query(m) == q for m in range(len(cases)))
    assert want_query is None or q == want_query, (cls, "nk_plan_batch_class_ok", q)
    rc = batch.call(sign)
    assert rc == L.NK_OK, (cls, rc, plan.lib.nk_last_error().decode(errors="replace"))
    tag = f"{cls}/n{len(cases)}/c{0 if sign == 1 else 1}"
    gots = batch.outputs(tag)
    worst = {}
    for m, (case, got) in enumerate(zip(cases, gots)):
        ref = pinned.ref(case, sign)
        rows = tc.compare(case, ref, got)
        for name, e, b, ok in rows:
            if ref[name][1] == "l2":
                nrm = max(tc.l2(ref[name][0]), 1e-300)
                e, b = e / nrm, b / nrm
            if name not in worst or e * worst[name][1] > worst[name][0] * b or not ok:
                worst[name] = (e, b)
        assert all(r[3] for r in rows), (tag, m, rows)
        one = pinned.single(case, sign, cls)
        for k in case.outputs:
            if k == "abar" and atomic_abar(case):
                continue  # atomics in a free order: no two calls agree in the last bit (module docstring)
            assert same_bits(got[k], one[k]), (tag, m, k, "differs from its single nk_hartley_fused call")
    host = host_error(cases[0], sign)
    for name, (e, b) in worst.items():
        record(plan, f"batch{'' if q else '-fallback'}/{tag}/{name}", cases[0].dtype, e, b, host)
    return q


def open_plan(shape, dtype):
    plan = PlanH(shape, dtype)
    assert_route(plan, shape, dtype)  # (nk_plan_route as tabulated, nk_plan_batch_ok on every 2-D strided-first plan)
    return plan


# ---- the chains on every twin size --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pro,epi", CHAINS, ids=[f"{p}->{e}" for p, e in CHAINS])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chains_on_every_twin_size(shape, dtype, pro, epi):
    """count 3, both conventions, shared launches asserted by name on every shape and dtype"""
    with open_plan(shape, dtype) as plan:
        assert plan.lib.nk_plan_batch_ok(plan.p) == 1
        assert plan.route[3] == (2 if shape == (4096, 512) and np.dtype(dtype) == np.float64 else 1)
        pinned = Pinned(plan, tc.transform_rel_bound(shape, dtype, plan.route))
        cases = make_cases(shape, dtype, pro, epi, 3)
        build = "/single-pair" if epi.startswith("vjp") and tc.final_single_pair_vjp(shape, dtype) else ""
        for sign in (1, -1):
            assert run_and_check(plan, cases, sign, f"{pro}->{epi}{build}", pinned, want_query=1) == 1


# ---- every class on the smallest twin grid: shared launches or the fallback, as the query says ----------------------------
MATRIX = list(dict.fromkeys([(p, "mul_scalar") for p in tc.PROLOGUES + tc.PROLOGUES_OCTANT] +
                            [("plain", e) for e in tc.EPILOGUES + tc.VJPS + ["vjp_w8"]]))  # (plain -> mul_scalar once)
# what the header rule gives for them (the test derives it from the record again: class_rule)
SHARED_PROLOGUES = {"plain", "mul", "amp_afield_oct", "jvp_dafield_oct"}
FALLBACK_EPILOGUES = {"vjp_atomic", "vjp_copies8", "vjp_carry"}  # a VJP without `afield`


@pytest.mark.parametrize("pro,epi", MATRIX, ids=[f"{p}->{e}" for p, e in MATRIX])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_class_matrix(dtype, pro, epi):
    with open_plan(BASE, dtype) as plan:
        pinned = Pinned(plan, tc.transform_rel_bound(BASE, dtype, plan.route))
        cases = make_cases(BASE, dtype, pro, epi, 2, seed=720)
        want = int(pro in SHARED_PROLOGUES and epi not in FALLBACK_EPILOGUES)
        sign = 1 if (MATRIX.index((pro, epi)) % 2 == 0) else -1
        run_and_check(plan, cases, sign, f"{pro}->{epi}", pinned, want_query=want)


def test_classes_without_a_twin_fall_back():
    """AFFINE and io32 (fp64 plans only) have no twin either: the query says 0 and the members run one by one"""
    with open_plan(BASE, np.float64) as plan:
        pinned = Pinned(plan, tc.transform_rel_bound(BASE, np.float64, plan.route))
        run_and_check(plan, make_cases(BASE, np.float64, "plain", "affine", 2, seed=730), 1, "plain->affine", pinned, want_query=0)
        cases = make_cases(BASE, np.float64, "amp_afield_oct", "lh_gauss_id", 2, seed=732, io32=True)
        assert cases[0].inputs["in"].dtype == np.float32
        run_and_check(plan, cases, -1, "io32/amp_afield_oct->lh_gauss_id", pinned, want_query=0)


# ---- every count --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pro,epi", CHAINS, ids=[f"{p}->{e}" for p, e in CHAINS])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_count(dtype, pro, epi):
    """members 0 .. count - 1 of eight fixed cases for count = 1 .. 8 (count 1 runs the single kernels by contract);
    references and single calls once per case"""
    with open_plan(BASE, dtype) as plan:
        pinned = Pinned(plan, tc.transform_rel_bound(BASE, dtype, plan.route))
        cases = make_cases(BASE, dtype, pro, epi, 8, seed=740)
        keys = [(c.set["scale"], c.set["offset"], c.set.get("mul_scalar"), c.set.get("addend_scale")) for c in cases]
        assert len(set(keys)) == 8 and len({k[0] for k in keys}) == 8
        sign = 1 if CHAINS.index((pro, epi)) % 2 == 0 else -1
        for count in range(1, L.MAX_BATCH + 1):
            run_and_check(plan, cases[:count], sign, f"{pro}->{epi}", pinned, want_query=1)


# ---- members that differ where the header allows it ---------------------------------------------------------------------------
def vjp_variants(shape, dtype):
    """four octant VJP members (afield, field_octant: one class) that differ in every optional field"""
    rng = np.random.default_rng(751)
    cases = make_cases(shape, dtype, "mul", "vjp_addend_acc", 4, seed=750)
    a, b, c, d = cases
    assert all(k in a.inputs for k in ("addend", "afield")) and "value" in a.outputs and a.set["accumulate"] == 1
    # b: no addend, no value, overwrites `out`
    del b.inputs["addend"], b.outputs["value"]
    b.set["accumulate"] = 0
    b.outputs["out"] = np.full(shape, np.nan, dtype=dtype)
    # c: addend, both carries, accumulates, no value
    del c.outputs["value"]
    c.inputs["carry1"], c.inputs["carry2"] = rng.normal(size=shape).astype(dtype), rng.normal(size=shape).astype(dtype)
    # d: addend and value, one carry, overwrites `out`
    d.inputs["carry1"] = rng.normal(size=shape).astype(dtype)
    d.set["accumulate"] = 0
    d.outputs["out"] = np.full(shape, np.nan, dtype=dtype)
    return cases


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", ["likelihood", "vjp", "nonlin"])
def test_members_differ_in_their_optional_fields(kind, dtype):
    """ONE launch of four members of one kernel class whose run-time fields differ; every record is also accepted by
    nk_hartley_fused on its own and meets its reference there"""
    with open_plan(BASE, dtype) as plan:
        pinned = Pinned(plan, tc.transform_rel_bound(BASE, dtype, plan.route))
        if kind == "likelihood":
            epis = ["lh_gauss_id", "lh_gaussf_exp", "lh_poisson_exp", "lh_poisson_sigmoid"]
            cases = [vary(tc.FusedCase(BASE, dtype, "amp_afield_oct", e, True, seed=760 + m), m) for m, e in enumerate(epis)]
            assert len({(c.set["lh_kind"], c.set["nonlin"], "icov" in c.inputs) for c in cases}) == 4
        elif kind == "nonlin":
            epis = ["nonlin_id", "nonlin_exp", "nonlin_sigmoid", "nonlin_exp"]
            cases = [vary(tc.FusedCase(BASE, dtype, "plain", e, True, seed=770 + m), m) for m, e in enumerate(epis)]
        else:
            cases = vjp_variants(BASE, dtype)
        for sign in (1, -1):
            run_and_check(plan, cases, sign, f"mixed-{kind}", pinned, want_query=1)
        for case in cases:
            got = pinned.single(case, 1, f"mixed-{kind}")
            assert all(r[3] for r in tc.compare(case, pinned.ref(case, 1), got))


# ---- shared read-only operands ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_members_share_read_only_operands(dtype):
    """all members pass the same `in` (the common direction of a KL metric) / the same amplitude field, bin index and
    tables (sampling solves at one point): outputs stay per member"""
    with open_plan(BASE, dtype) as plan:
        pinned = Pinned(plan, tc.transform_rel_bound(BASE, dtype, plan.route))
        cases = make_cases(BASE, dtype, "jvp_dafield_oct", "mul_field", 4, seed=780)
        for c in cases[1:]:
            c.inputs["in"] = cases[0].inputs["in"]
        run_and_check(plan, cases, 1, "shared-in/jvp_dafield_oct->mul_field", pinned, want_query=1, shared=("in",))
        for pro, epi, sign in (("amp_afield_oct", "lh_gauss_exp", -1), ("mul", "vjp_w8", 1), ("mul", "vjp_addend_acc", -1)):
            cases = make_cases(BASE, dtype, pro, epi, 4, seed=784)
            for c in cases[1:]:
                for k in ("pidx", "amp", "damp", "afield"):
                    c.inputs[k] = cases[0].inputs[k]
            run_and_check(plan, cases, sign, f"shared-afield/{pro}->{epi}", pinned, want_query=1,
                          shared=("pidx", "amp", "damp", "afield"))


# ---- plans without twins ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(64, 64), (64, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_fallback_plans(shape, dtype):
    """axes below 512 (nk_plan_batch_ok still 1 in 2-D) and a 3-D plan (nk_plan_batch_ok 0): member by member inside the
    library, same checks"""
    with open_plan(shape, dtype) as plan:
        assert plan.lib.nk_plan_batch_ok(plan.p) == (1 if len(shape) == 2 else 0)
        pinned = Pinned(plan, tc.transform_rel_bound(shape, dtype, plan.route))
        for i, (pro, epi) in enumerate((("amp_afield_oct", "lh_gauss_exp"), ("mul", "vjp_addend_acc"))):
            cases = make_cases(shape, dtype, pro, epi, 3, seed=790)
            run_and_check(plan, cases, 1 if i == 0 else -1, f"{pro}->{epi}", pinned, want_query=0)


# ---- argument checks: every one returns before any launch ----------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_alone():
    with open_plan(BASE, np.float64) as plan:
        lib = plan.lib
        assert lib.nk_plan_batch_class_ok(None, None) == 0 and lib.nk_plan_batch_class_ok(plan.p, None) == 0
        cases = make_cases(BASE, np.float64, "plain", "mul_field", 3, seed=800)
        batch = Batch(plan, cases)
        assert lib.nk_plan_batch_class_ok(None, ctypes.byref(batch.fuses[0])) == 0 and batch.query() == 1
        ws = [w.ptr for w in batch.ws]
        for what, kw in (("count 0", dict(count=0)), ("NULL workspace", dict(ws_ptrs=[ws[0], None, ws[2]])),
                         ("one workspace twice", dict(ws_ptrs=[ws[0], ws[1], ws[0]]))):
            assert batch.call(1, **kw) == L.NK_ERR_INVALID, what
            batch.untouched(what)
        # nine valid records on nine workspaces: one more than NK_MAX_BATCH
        nine = Batch(plan, make_cases(BASE, np.float64, "plain", "mul_scalar", L.MAX_BATCH + 1, seed=801))
        assert nine.call(1) == L.NK_ERR_INVALID
        nine.untouched("count 9")
        # members of different kernel classes: w8 on one member only; an amplitude field on one member only
        a, b = make_cases(BASE, np.float64, "mul", "vjp_w8", 2, seed=802)
        del b.outputs["w8"]
        c, d = make_cases(BASE, np.float64, "plain", "vjp_addend_acc", 2, seed=804)
        del d.inputs["afield"]
        d.set["field_octant"] = 0
        for what, pair in (("w8 on one member", [a, b]), ("afield on one member", [c, d]), ("two epilogues", [cases[0], a])):
            mixed = Batch(plan, pair)
            assert mixed.call(1) == L.NK_ERR_INVALID, what
            assert b"different kernel classes" in lib.nk_last_error(), what
            mixed.untouched(what)
