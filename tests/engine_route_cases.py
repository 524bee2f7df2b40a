"""The engine routes that grid geometry and size select, as one table of cases with the flags that prove a route
was taken, and the test bodies the cases run: shared by tests/test_engine_gpu.py (the default routes) and
tests/test_engine_routes_gpu.py (everything else); tests/test_engine_route_cases.py holds the table to the binning on the host.

Routes (FusedModel.__init__, draw_samples, the generic distributors):
  1  3-D octant + sandwich grid with unequal harmonic distances: no integer k^2 table, the octant sums are added bin by bin
     by nk_csr_rowsum over `seg_plan`
  2  natural binning without the fixed-point shell scatter (`w8max` not wired, no grouped scatter): the busiest (shell,
     a mod 16) cell holds engine.SCATTER_FIXED_POINT_MAX_POINTS points or more.  The bins are summed over `seg_plan` in a fixed
     order; with NK_SEGMENT_SUM=0 by the floating-point LDS atomics of the shell scatter, whose order varies from launch to
     launch (compared with the oracle only)
  3  generic grid beyond backend.BIN_PLAN_MAX: the VJP epilogue adds into 8 private copies of abar, nk_fold_copies folds them
  4  NK_SEGMENT_SUM=0: octant sums through the global atomics of nk_octant_scatter, with and without merged swapped lines
  5  grids beyond engine.SPECTRUM_DEVICE_DRAW_MAX_POINTS: the spectrum excitations of a prior draw come from the host
     generator, one sample ahead on a worker thread (_HostDrawAhead)
  6  index maps beyond backend.BIN_PLAN_MAX: DOFDistributor / PowerDistributor ADJOINT and the partial ContractionOperator
     through the atomics of backend.scatter_add
A size limit is lowered (monkeypatch) so that a small grid takes the route; the geometry routes need no forcing."""
import threading
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble

ANISO = (0.02, 0.03, 0.013)       # three different harmonic distances
ANISO_EQ01 = (0.02, 0.02, 0.013)  # equal on the two leading axes: swapped lines may be merged
HALF_LAST = (1 / 64, 1 / 64, 1 / 64)  # harmonic distances (1, 1, 0.5) on (64, 64, 128)
ANISO_2D = (0.02, 0.013)

# (shape, distances): (power bins, integer k^2 table exists, harmonic distances of the two leading axes are equal)
GEOMETRIES = {
    ((64, 64, 128), None): (4492, True, True),
    ((64, 64, 128), HALF_LAST): (4390, False, True),
    ((64, 64, 128), ANISO_EQ01): (28966, False, True),
    ((64, 64, 128), ANISO): (55995, False, False),
    ((64, 128), ANISO_2D): (2134, False, False),
    ((30, 50), ANISO_2D): (413, False, False),
    ((64, 128, 128), None): (6732, True, True),
    ((64, 128), None): (1232, True, True),
    ((30, 50), None): (245, True, True),
    ((12, 10, 14), None): (79, True, True),
}

FLAG_NAMES = ("octant_vjp", "sandwich", "bin_k2", "seg_plan", "group_scatter", "scatter_fixed_point", "merge_swapped",
              "full_plan", "wfull", "pair_ready", "wide", "wide_generic")


def route_flags(model):
    """What FusedModel decided, by name: arrays and plans as present / absent."""
    return dict(octant_vjp=bool(model.octant_vjp), sandwich=bool(model.sandwich), bin_k2=model.bin_k2 is not None,
                seg_plan=model.seg_plan is not None, group_scatter=bool(model.group_scatter),
                scatter_fixed_point=bool(model.scatter_fixed_point), merge_swapped=int(model.merge_swapped),
                full_plan=model.full_plan is not None, wfull=model.wfull is not None, pair_ready=bool(model.pair_ready()),
                wide=bool(model.wide), wide_generic=bool(model.wide_generic))


@dataclass(frozen=True)
class RouteCase:
    name: str
    route: int
    shape: tuple
    distances: tuple = None
    dtype: str = "float64"
    kind: str = "gaussian"
    nonlin: str = None
    env: tuple = ()      # ((variable, value), ...) set before the model is built
    attrs: tuple = ()    # (("engine" | "backend", constant, value), ...) lowered before the model is built
    flags: dict = field(default_factory=dict, hash=False)  # subset of route_flags the model must show
    fp32_class: str = None  # key of FP32_TOL

    @property
    def id(self):
        return self.name


# the flags of a route
R1 = dict(octant_vjp=True, sandwich=True, bin_k2=False, seg_plan=True, group_scatter=False, pair_ready=False)
R2 = dict(octant_vjp=True, sandwich=True, bin_k2=True, scatter_fixed_point=False, group_scatter=False, seg_plan=True,
          pair_ready=True)
R3 = dict(octant_vjp=False, full_plan=False, wfull=False)
R4 = dict(octant_vjp=True, seg_plan=False, bin_k2=False)
NO_FIXED_POINT = (("engine", "SCATTER_FIXED_POINT_MAX_POINTS", 0),)
NO_BIN_PLAN = (("backend", "BIN_PLAN_MAX", 0),)
NO_SEGMENT_SUM = (("NK_SEGMENT_SUM", "0"),)
CUBE = (64, 64, 128)

# single applications: value, gradient, metric against the oracle (`seeded_engine_vs_oracle`)
SEEDED_CASES = [
    # route 1, unforced: the geometry selects it
    RouteCase("r1-aniso-gauss-f64", 1, CUBE, ANISO, flags=dict(R1, merge_swapped=0)),
    RouteCase("r1-aniso-poisson-f64", 1, CUBE, ANISO, kind="poisson", nonlin="exp", flags=dict(R1, merge_swapped=0)),
    RouteCase("r1-aniso-gauss-f32", 1, CUBE, ANISO, dtype="float32", flags=dict(R1, merge_swapped=0, wide=True),
              fp32_class="aniso3d"),
    RouteCase("r1-eq01-gauss-f64", 1, CUBE, ANISO_EQ01, flags=dict(R1, merge_swapped=1)),
    RouteCase("r1-eq01-poisson-f64", 1, CUBE, ANISO_EQ01, kind="poisson", nonlin="exp", flags=dict(R1, merge_swapped=1)),
    # (other pipelines with a distance of their own: the 2-D quadrant pipeline and the generic kernels)
    RouteCase("r1-aniso2d-gauss-f64", 1, (64, 128), ANISO_2D,
              flags=dict(octant_vjp=True, sandwich=False, bin_k2=False, seg_plan=True)),
    RouteCase("r1-generic-aniso-gauss-f64", 1, (30, 50), ANISO_2D, flags=dict(octant_vjp=False, full_plan=True, wfull=True)),
    # route 2
    RouteCase("r2-cube-gauss-f64", 2, CUBE, attrs=NO_FIXED_POINT, flags=R2),
    # (pairs need a constant metric weight: `pair_ready()` is False for the Poisson likelihood)
    RouteCase("r2-cube-poisson-f64", 2, CUBE, kind="poisson", nonlin="exp", attrs=NO_FIXED_POINT,
              flags=dict(R2, pair_ready=False)),
    RouteCase("r2-cube-gauss-f32", 2, CUBE, dtype="float32", attrs=NO_FIXED_POINT, flags=dict(R2, wide=True),
              fp32_class="default"),
    RouteCase("r2-64x128x128-gauss-f64", 2, (64, 128, 128), attrs=NO_FIXED_POINT, flags=R2),
    # (NK_SEGMENT_SUM=0: the shell scatter with floating-point LDS atomics)
    RouteCase("r2-float-cube-gauss-f64", 2, CUBE, attrs=NO_FIXED_POINT, env=NO_SEGMENT_SUM, flags=dict(R2, seg_plan=False)),
    RouteCase("r2-float-cube-poisson-f64", 2, CUBE, kind="poisson", nonlin="exp", attrs=NO_FIXED_POINT, env=NO_SEGMENT_SUM,
              flags=dict(R2, seg_plan=False, pair_ready=False)),
    RouteCase("r2-float-64x128x128-gauss-f64", 2, (64, 128, 128), attrs=NO_FIXED_POINT, env=NO_SEGMENT_SUM,
              flags=dict(R2, seg_plan=False)),
    # route 3
    RouteCase("r3-30x50-gauss-f64", 3, (30, 50), attrs=NO_BIN_PLAN, flags=R3),
    RouteCase("r3-30x50-poisson-f64", 3, (30, 50), kind="poisson", nonlin="exp", attrs=NO_BIN_PLAN, flags=R3),
    RouteCase("r3-12x10x14-gauss-f64", 3, (12, 10, 14), attrs=NO_BIN_PLAN, flags=R3),
    RouteCase("r3-12x10x14-poisson-f64", 3, (12, 10, 14), kind="poisson", nonlin="exp", attrs=NO_BIN_PLAN, flags=R3),
    RouteCase("r3-30x50-aniso-gauss-f64", 3, (30, 50), ANISO_2D, attrs=NO_BIN_PLAN, flags=R3),
    RouteCase("r3-30x50-aniso-poisson-f64", 3, (30, 50), ANISO_2D, kind="poisson", nonlin="exp", attrs=NO_BIN_PLAN, flags=R3),
    RouteCase("r3-30x50-gauss-f32", 3, (30, 50), dtype="float32", attrs=NO_BIN_PLAN, flags=dict(R3, wide_generic=True),
              fp32_class="default"),
    # route 4
    RouteCase("r4-halflast-gauss-f64", 4, CUBE, HALF_LAST, env=NO_SEGMENT_SUM, flags=dict(R4, merge_swapped=1)),
    RouteCase("r4-halflast-poisson-f64", 4, CUBE, HALF_LAST, kind="poisson", nonlin="exp", env=NO_SEGMENT_SUM,
              flags=dict(R4, merge_swapped=1)),
    # (equal leading AXES, unequal leading DISTANCES: the lines (a, b) and (b, a) lie in different bins and must not be merged)
    RouteCase("r4-aniso-gauss-f64", 4, CUBE, ANISO, env=NO_SEGMENT_SUM, flags=dict(R4, merge_swapped=0)),
    RouteCase("r4-64x128-gauss-f64", 4, (64, 128), env=NO_SEGMENT_SUM, flags=dict(R4, merge_swapped=0)),
]

# pairs and groups: the body of test_sandwich_engine_vs_oracle and the five-sample KL metric (`kl5_metric`).  On route 1
# `pair_ready()` is False (it asks for the k^2 table), so the KL applies sample by sample there; on route 2 the pair and group
# launches run and every member's bin sums come from `_bin_sums` (over `seg_plan`), not from the group shell walk
PAIR_CASES = [
    RouteCase("r1-aniso-pairs-f64", 1, CUBE, ANISO, flags=dict(R1, merge_swapped=0)),
    RouteCase("r2-cube-pairs-f64", 2, CUBE, attrs=NO_FIXED_POINT, flags=R2),
    RouteCase("r2-64x128x128-pairs-f64", 2, (64, 128, 128), attrs=NO_FIXED_POINT, flags=R2),
]

ALL_CASES = SEEDED_CASES + PAIR_CASES

# fp32 bounds (value / gradient, metric) per class: twice the worst error measured on the GPU (profiles/engine_route_errors.txt),
# starting from the default route's numbers; nothing above the suite's 1.2e-4 ceiling
FP32_CEILING = 1.2e-4
FP32_TOL = {
    "default": (1e-5, 3e-6),  # tests/test_engine_gpu.py: `wide`, `wide_generic` or Gaussian
    # 55995 bins on 64 x 64 x 128: measured 1.5e-7 (gradient, key loglogavgslope) and 8.8e-8 (metric, key asperity) -- the
    # many-bin geometry stays inside the default numbers, so no bound of its own
    "aniso3d": (1e-5, 3e-6),
}


def torch_dtype(case):
    import torch

    return getattr(torch, case.dtype)


def force(case, monkeypatch):
    """Lower the limits and set the variables of a case -- before the model is built; undone by monkeypatch."""
    import nifty_amd as ift
    from nifty_amd import backend, engine

    mods = {"engine": engine, "backend": backend}
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    for mod, name, value in case.attrs:
        monkeypatch.setattr(mods[mod], name, value)
    ift.PowerSpace._cache.clear()


def assert_route(model, case):
    """The model shows every flag of the case: a case cannot fall back to the default route unnoticed."""
    got = route_flags(model)
    shown = {k: got[k] for k in case.flags}
    print(f"ROUTE {case.name}: route {case.route} nb {model.nb} " + " ".join(f"{k}={v}" for k, v in shown.items()))
    assert shown == dict(case.flags), (case.name, shown, case.flags)
    assert model.nb == GEOMETRIES[(case.shape, case.distances)][0]


def per_key_relerr(a, b):
    """goldenlib.lat_relerr key by key: every key's largest error over its own largest entry (scalars: over at least 1e-3 of the
    vector's largest entry)"""
    scale = max(float(np.max(np.abs(b[k]))) for k in b)
    return {k: float(np.max(np.abs(np.asarray(a[k], dtype=np.float64) - b[k]))) / max(float(np.max(np.abs(b[k]))), 1e-3 * scale)
            for k in b}


def _fmt(per):
    return " ".join(f"{k}={e:.1e}" for k, e in sorted(per.items()))


# ---- single applications ----------------------------------------------------------------------------------------------------
def seeded_engine_vs_oracle(shape, kind, nonlin, dtype, tolerances, distances=None, check_model=None, label=""):
    """Same seeded inputs through the HIP engine and the numpy oracle: value, gradient and one metric application against
    orc.Linearized, and the metric's self-adjointness.  tolerances(model) -> (value / gradient bound, metric bound);
    check_model(model) runs before anything is compared.  Returns the measured errors."""
    import torch

    from nifty_amd.engine import FusedModel, LatentVec
    from oracle import nifty_oracle as orc
    from tests import goldenlib as gl

    rng = np.random.default_rng(11)
    cf = orc.CFModel(shape, distances, orc.CFParams(offset_mean=1.5))
    truth = cf.draw_latent(rng)
    s = cf.forward(truth)
    g, _ = orc.NONLIN[nonlin]
    if kind == "gaussian":
        data = g(s) + 0.1 * rng.normal(size=shape)
        lh = orc.Likelihood("gaussian", data, icov=100.0, nonlin=nonlin)
        model = FusedModel(shape, distances, offset_mean=1.5, likelihood="gaussian", data=data, icov=100.0, nonlin=nonlin,
                           dtype=dtype)
    else:
        data = rng.poisson(g(s)).astype(np.int64)
        lh = orc.Likelihood("poisson", data, nonlin=nonlin)
        model = FusedModel(shape, distances, offset_mean=1.5, likelihood="poisson", data=data, nonlin=nonlin, dtype=dtype)
    if check_model is not None:
        check_model(model)
    x = {k: 0.3 * a for k, a in cf.draw_latent(rng).items()}
    v = cf.draw_latent(rng)
    if dtype == torch.float32:  # identical inputs for both paths
        x["xi"] = x["xi"].astype(np.float32).astype(np.float64)
        v["xi"] = v["xi"].astype(np.float32).astype(np.float64)
        if kind == "gaussian":
            lh.data = lh.data.astype(np.float32).astype(np.float64)
    lin = orc.Linearized(cf, lh, x)
    val, grad = lin.value_grad()
    mv = lin.metric(v)
    xl, vl = LatentVec.from_dict(model, x), LatentVec.from_dict(model, v)
    lp = model.linearize(xl)
    # fp32 fields: value + gradient within the 1e-5 of north_star on every grid (their forward transform runs in fp64:
    # FusedModel.wide on the register-resident pipelines, FusedModel.wide_generic on mixed-radix grids and short axes);
    # a metric application is two fp32 transforms with a pointwise weight in between
    if dtype == torch.float32:
        assert model.wide or model.wide_generic
    tol, mtol = tolerances(model)
    e_val = abs(float(lp.value.item()) - val) / abs(val)
    got_grad, got_met = lp.grad.to_dict(), model.metric(lp, vl).to_dict()
    e_grad, e_met = gl.lat_relerr(got_grad, grad), gl.lat_relerr(got_met, mv)
    print(f"{label}{shape} {distances} {kind} {nonlin} {dtype}: value {e_val:.1e} gradient {e_grad:.1e} metric {e_met:.1e}")
    per_grad, per_met = per_key_relerr(got_grad, grad), per_key_relerr(got_met, mv)
    print(f"{label}  gradient per key: {_fmt(per_grad)}")
    print(f"{label}  metric per key: {_fmt(per_met)}")
    assert e_val < tol and e_grad < tol and e_met < mtol
    # adjointness of the metric (reference extra.py:220-231): <u, M v> == <M u, v>
    u = LatentVec.from_dict(model, cf.draw_latent(rng))
    mvl = model.metric(lp, vl)
    a = u.s_vdot(mvl)
    b = model.metric(lp, u).s_vdot(vl)
    # <u, M v> of two random vectors cancels to a small number: the rounding scale is |u| |M v|, not |a|
    e_adj = abs(a - b) / (u.norm() * mvl.norm())
    print(f"{label}  adjointness {e_adj:.1e}")
    assert e_adj < (1e-12 if dtype == torch.float64 else 2e-6)
    return dict(value=e_val, gradient=e_grad, metric=e_met, adjointness=e_adj, gradient_per_key=per_grad,
                metric_per_key=per_met)


def route_tolerances(case):
    """fp64: the default route's 1e-10; fp32: the bounds of the case's class"""
    if case.dtype == "float64":
        return lambda model: (1e-10, 1e-10)
    return lambda model: FP32_TOL[case.fp32_class]


# ---- pairs and groups -------------------------------------------------------------------------------------------------------
def sandwich_inputs(shape, lh, distances=None):
    """(cf, x, v, oracle likelihood, FusedModel keywords) of `sandwich_engine_vs_oracle`"""
    from oracle import nifty_oracle as orc

    rng = np.random.default_rng(3)
    cf = orc.CFModel(shape, distances, orc.CFParams(offset_mean=1.0))
    x = {k: 0.2 * v for k, v in cf.draw_latent(rng).items()}
    v = cf.draw_latent(rng)
    if lh == "poisson":
        data = rng.poisson(np.exp(cf.forward(cf.draw_latent(rng)) * 0.3)).astype(np.int64)
        lho = orc.Likelihood("poisson", data, nonlin="exp")
        kw = dict(likelihood="poisson", data=data, nonlin="exp")
    else:
        data = cf.forward(cf.draw_latent(rng)) + 0.1 * rng.normal(size=shape)
        lho = orc.Likelihood("gaussian", data, icov=100.0)
        kw = dict(likelihood="gaussian", data=data, icov=100.0)
    return cf, x, v, lho, kw, rng


def rel_xi_spectrum(a, b):
    return max(float(np.max(np.abs(a[k] - b[k])) / max(np.max(np.abs(b[k])), 1e-30)) for k in ("xi", "spectrum"))


def sandwich_engine_vs_oracle(shape, dtype, lh, monkeypatch, distances=None, check_model=None, label=""):
    """Metric application, MGVI sample (CG with the fused curvature dot AND the direction update riding in the first
    transform pass) and KL against the numpy oracle, over the sandwich / fused-direction combinations; check_model(model,
    sandwich) runs on every model before anything is compared."""
    import torch

    from nifty_amd import random
    from nifty_amd.engine import FusedKL, FusedModel, LatentVec, draw_samples
    from nifty_amd.minimization import AbsDeltaEnergyController
    from oracle import nifty_oracle as orc

    cf, x, v, lho, kw, _ = sandwich_inputs(shape, lh, distances)
    lin = orc.Linearized(cf, lho, x)
    mv = lin.metric(v)
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    rel = rel_xi_spectrum
    results = []
    for sandwich, fused_dir, recur in (("2", "1", "0"), ("2", "0", "0"), ("0", "0", "0"), ("2", "1", "1")):
        monkeypatch.setenv("NK_SANDWICH", sandwich)
        monkeypatch.setenv("NK_CG_FUSED_DIRECTION", fused_dir)
        monkeypatch.setenv("NK_CG_ENERGY_RECURRENCE", recur)  # 1: energy of the CG iterate by recurrence (nk_cg_update_dr)
        model = FusedModel(shape, distances, offset_mean=1.0, dtype=dtype, device="cuda:0", **kw)
        assert model.sandwich == (sandwich == "2") and model.fused_direction == (fused_dir == "1")
        if check_model is not None:
            check_model(model, sandwich == "2")
        xl, vl = LatentVec.from_dict(model, x), LatentVec.from_dict(model, v)
        lp = model.linearize(xl)
        e_met = rel(model.metric(lp, vl).to_dict(), mv)
        print(f"{label}sandwich={sandwich} fused_direction={fused_dir} recurrence={recur}: metric {e_met:.1e}")
        assert e_met < tol
        random.push_sseq_from_seed(7)
        res, negs, _ = draw_samples(model, xl, 1, True, lambda: AbsDeltaEnergyController(0.05, iteration_limit=6))
        random.pop_sseq()
        kl = FusedKL(model, xl, res, negs)
        results.append((res[0].to_dict(), kl.value, kl.apply_metric(vl).to_dict()))
    res_o, negs_o = orc.draw_samples(cf, lho, x, 1, True, np.random.SeedSequence(7),
                                     lambda: orc.AbsDeltaEnergyController(0.05, iteration_limit=6))
    kl_o = orc.SampledKL(cf, lho, x, res_o, negs_o)
    ctol = 1e-7 if dtype == torch.float64 else 5e-3  # six CG iterations amplify rounding differences
    for r0, val, mv_kl in results:
        e_res, e_val, e_klm = rel(r0, res_o[0]), abs(val - kl_o.value) / abs(kl_o.value), rel(mv_kl, kl_o.apply_metric(v))
        print(f"{label}  residual {e_res:.1e} KL value {e_val:.1e} KL metric {e_klm:.1e}")
        assert e_res < ctol
        assert e_val < (1e-8 if dtype == torch.float64 else 1e-4)
        assert e_klm < ctol
    # the fused and the separate direction update are the same arithmetic
    assert rel(results[0][0], results[1][0]) < (1e-12 if dtype == torch.float64 else 1e-5)


def kl5_metric(case, monkeypatch, check_model):
    """A five-sample FusedKL.apply_metric on the large-grid path (pair launches for the samples (0, 1) and (2, 3) where the
    model is `pair_ready`, counted) against the oracle's SampledKL at the bound of a single metric application (the residuals
    are inputs here, not CG results), and against the same applications with NK_PAIR_FINAL=0, bit for bit.

    Before route 2 summed its bins over `seg_plan`, it missed the bit equality in the `small` part, measured on an MI355X: xi
    identical, `small` off by 2.8e-16 (64 x 64 x 128) and 4.8e-18 .. 1.5e-16 (64 x 128 x 128, two runs) of its largest entry,
    all within 6.2e-15 of the oracle.  The cause was the route, not the pair launch: the floating-point LDS atomics of the
    shell scatter add in an order that varies from launch to launch, and two runs of the SAME launches differed alike."""
    import torch

    from nifty_amd.engine import FusedKL, FusedModel, LatentVec
    from oracle import nifty_oracle as orc

    cf, x, v, lho, kw, rng = sandwich_inputs(case.shape, "gaussian", case.distances)
    # (the stream lanes of small grids would take the samples one by one: the large-grid path, as in group_cases.sampling_case)
    monkeypatch.setenv("NK_LANE_MAX_POINTS", "0")
    model = FusedModel(case.shape, case.distances, offset_mean=1.0, dtype=torch_dtype(case), device="cuda:0", **kw)
    check_model(model)
    pair_calls = []
    launch_pair = model.lh_metric_accumulate_pair
    monkeypatch.setattr(model, "lh_metric_accumulate_pair", lambda *a, **k: (pair_calls.append(1), launch_pair(*a, **k))[1])
    res = [{k: 0.1 * a for k, a in cf.draw_latent(rng).items()} for _ in range(5)]
    negs = [False] * 5
    xl, vl = LatentVec.from_dict(model, x), LatentVec.from_dict(model, v)
    kl = FusedKL(model, xl, [LatentVec.from_dict(model, r) for r in res], negs)
    assert len(kl._lanes) == 1 and not kl._batched
    paired = kl.apply_metric(vl)
    assert len(pair_calls) == (2 if case.flags["pair_ready"] else 0)  # samples (0, 1), (2, 3) and a single one
    monkeypatch.setenv("NK_PAIR_FINAL", "0")
    assert not model.pair_ready()
    single = kl.apply_metric(vl)
    assert len(pair_calls) == (2 if case.flags["pair_ready"] else 0)
    monkeypatch.delenv("NK_PAIR_FINAL")
    same_xi, same_small = torch.equal(paired.xi, single.xi), torch.equal(paired.small, single.small)
    d_small = float((paired.small - single.small).abs().max() / single.small.abs().max())
    ref = orc.SampledKL(cf, lho, x, res, negs).apply_metric(v)
    e_pair, e_single = rel_xi_spectrum(paired.to_dict(), ref), rel_xi_spectrum(single.to_dict(), ref)
    print(f"KL5 {case.name}: pair_ready {case.flags['pair_ready']} xi equal {same_xi} small equal {same_small} "
          f"(largest difference {d_small:.1e}) against the oracle: paired {e_pair:.1e} single {e_single:.1e}")
    assert e_pair < 1e-9 and e_single < 1e-9
    assert same_xi
    assert same_small


# ---- route 5: draws -----------------------------------------------------------------------------------------------------------
ZIGGURAT_TAIL = 3.6541528853610087  # |x| beyond it goes through log1p: device math library against the host's (tests/test_rng.py)


def ulps(a, b):
    view = np.int64 if a.dtype == np.float64 else np.int32
    return np.abs(a.view(view).astype(np.int64) - b.view(view).astype(np.int64))


def device_draw_matches(got, ref):
    """The bar tests/test_rng.py sets for the device stream of standard normals: identical outside the ziggurat tail, 4 ulp
    inside it.  Returns (ok, draws in the tail, draws that differ)."""
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1).astype(got.dtype)
    tail = np.abs(ref) > ZIGGURAT_TAIL
    ok = np.array_equal(got[~tail], ref[~tail]) and (not tail.any() or int(ulps(got[tail], ref[tail]).max()) <= 4)
    return bool(ok), int(tail.sum()), int((got != ref).sum())


def numpy_prior_draw(seed, shape, nb):
    """What np.random.default_rng(seed) gives in LATENT_KEYS order, and the generator's state afterwards"""
    from nifty_amd.engine import LATENT_KEYS

    rng = np.random.default_rng(seed)
    sizes = {"xi": tuple(shape), "spectrum": (2, nb - 2)}
    return {k: rng.normal(0.0, 1.0, sizes.get(k, ())) for k in LATENT_KEYS}, rng.bit_generator.state


def draw_ahead_workers(timeout=10.0):
    """The worker threads of engine._HostDrawAhead still alive, by thread name; a worker that has been told to stop is given
    the time to do so (join returns as soon as it has)."""
    from nifty_amd.engine import _HostDrawAhead

    mine = [t for t in threading.enumerate() if t.name.startswith(_HostDrawAhead.THREAD_PREFIX)]
    for t in mine:
        t.join(timeout)
    return [t.name for t in mine if t.is_alive()]


# ---- route 6: generic operators -----------------------------------------------------------------------------------------------
def binned_reference(index, values, nbins):
    """Long-double sums of `values` per bin of `index` and the bound gamma(n_max) sum |terms| per bin, n_max the longest bin
    (any order of the atomic additions: Higham 3.1, tests/binmap_cases.py)"""
    from tests.binmap_cases import bin_sums, gamma

    index = np.asarray(index).reshape(-1)
    v = np.asarray(values, dtype=LD).reshape(-1)
    n_max = int(np.bincount(index, minlength=nbins).max())
    return bin_sums(index, v, nbins), gamma(n_max) * bin_sums(index, np.abs(v), nbins), n_max
