"""The engine routes that grid geometry and size select, end to end against the numpy oracle (tests/engine_route_cases.py holds
the case table, the forcing and the shared test bodies; DESIGN 3.1 lists the routes).  Every test asserts the flags of its route
before it compares anything.  The atomics of routes 3, 4 and 6 (and of route 2 under NK_SEGMENT_SUM=0) add in an order that
varies from run to run: those results are held to the reference only, never to each other."""
import numpy as np
import pytest
import torch

import nifty_amd as ift
from nifty_amd import backend as B
from nifty_amd import batched, engine, random
from nifty_amd.engine import FusedModel, LatentVec, draw_samples
from nifty_amd.minimization import AbsDeltaEnergyController
from oracle import nifty_oracle as orc
from tests import engine_route_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_power_spaces():
    """A PowerSpace built under a lowered limit must not outlive its test"""
    yield
    ift.PowerSpace._cache.clear()


# ---- routes 1 - 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.SEEDED_CASES, ids=lambda c: c.id)
def test_route_vs_oracle_seeded(case, monkeypatch):
    """The body of test_engine_vs_oracle_seeded on every route case: value, gradient and metric against orc.Linearized at the
    default route's bounds, and the metric's self-adjointness."""
    rc.force(case, monkeypatch)
    rc.seeded_engine_vs_oracle(case.shape, case.kind, case.nonlin, rc.torch_dtype(case), rc.route_tolerances(case),
                               distances=case.distances, check_model=lambda m: rc.assert_route(m, case),
                               label=f"ERR {case.name} ")


@pytest.mark.parametrize("case", rc.PAIR_CASES, ids=lambda c: c.id)
def test_route_sandwich_vs_oracle(case, monkeypatch):
    """The body of test_sandwich_engine_vs_oracle on routes 1 and 2: one mirrored pair from draw_samples, FusedKL value and
    apply_metric against orc.draw_samples / orc.SampledKL over the sandwich / fused-direction combinations."""
    rc.force(case, monkeypatch)

    def check(model, sandwich):  # (NK_SANDWICH=0 of the body's third combination: no sandwich, hence no pairs)
        flags = dict(case.flags) if sandwich else dict(case.flags, sandwich=False, pair_ready=False)
        rc.assert_route(model, rc.RouteCase(case.name, case.route, case.shape, case.distances, flags=flags))

    rc.sandwich_engine_vs_oracle(case.shape, rc.torch_dtype(case), "gaussian", monkeypatch, distances=case.distances,
                                 check_model=check, label=f"ERR {case.name} ")


@pytest.mark.parametrize("case", rc.PAIR_CASES, ids=lambda c: c.id)
def test_route_kl_metric_pairs_and_groups(case, monkeypatch):
    """Five samples: FusedKL.apply_metric (route 2: two pair launches, every member's bin sums from `_bin_sums`) against
    orc.SampledKL, and against NK_PAIR_FINAL=0 bit for bit (engine_route_cases.kl5_metric)."""
    rc.force(case, monkeypatch)
    rc.kl5_metric(case, monkeypatch, lambda m: rc.assert_route(m, case))


# ---- route 5: the draws of large grids ------------------------------------------------------------------------------------------
def _host_spectrum(monkeypatch, lanes_off=False):
    monkeypatch.setattr(engine, "SPECTRUM_DEVICE_DRAW_MAX_POINTS", 0)
    monkeypatch.delenv("NK_DRAW_AHEAD", raising=False)
    if lanes_off:
        monkeypatch.setenv("NK_LANE_MAX_POINTS", "0")


def test_prior_draw_with_the_host_spectrum(monkeypatch):
    """draw_prior beyond SPECTRUM_DEVICE_DRAW_MAX_POINTS: scalars and spectrum are numpy's own draws bit for bit, xi the device
    stream at the bar of tests/test_rng.py, the context generator ends in numpy's state; draw_prior(ahead=...) gives the same
    tensors and the same state, and refuses a context that has drawn since its seed was handed out."""
    _host_spectrum(monkeypatch)
    seed, shape = 23, (64, 128)
    model = FusedModel(shape, offset_mean=1.0, likelihood="gaussian", icov=100.0, dtype=torch.float64, device="cuda:0")
    assert model.N > engine.SPECTRUM_DEVICE_DRAW_MAX_POINTS
    sseq = np.random.SeedSequence(seed)
    with random.Context(sseq):
        x = model.draw_prior()
        state = random.current_rng().bit_generator.state
    ref, ref_state = rc.numpy_prior_draw(np.random.SeedSequence(seed), shape, model.nb)
    small = x.small.cpu().numpy()
    assert np.array_equal(small[:5], np.array([ref[k] for k in engine.SMALL_KEYS]))
    assert np.array_equal(small[5:], ref["spectrum"].reshape(-1))
    ok, ntail, ndiff = rc.device_draw_matches(x.xi.cpu().numpy(), ref["xi"])
    print(f"DRAW prior (64, 128): xi {ntail} draws in the ziggurat tail, {ndiff} differ from numpy")
    assert ok
    assert state == ref_state
    # the same draw with its host part made ahead
    ahead = model.host_draws_before_xi(np.random.SeedSequence(seed))
    with random.Context(np.random.SeedSequence(seed)):
        y = model.draw_prior(ahead=ahead)
        assert random.current_rng().bit_generator.state == ref_state
    assert torch.equal(x.xi, y.xi) and torch.equal(x.small, y.small)
    with random.Context(np.random.SeedSequence(seed)):
        random.current_rng().normal()
        with pytest.raises(RuntimeError):
            model.draw_prior(ahead=ahead)


class _CountingAhead(engine._HostDrawAhead):
    made, taken = 0, 0

    def __init__(self, model, seeds):
        _CountingAhead.made += 1
        super().__init__(model, seeds)

    def take(self, seed):
        got = super().take(seed)
        _CountingAhead.taken += got is not None
        return got


@pytest.mark.parametrize("shape,grouped,fixed_point", [((64, 128), False, False), ((64, 64, 128), True, True),
                                                      ((64, 64, 128), True, False)],
                         ids=["serial", "grouped", "grouped-route2"])
def test_draw_samples_with_draws_ahead(shape, grouped, fixed_point, monkeypatch):
    """draw_samples beyond SPECTRUM_DEVICE_DRAW_MAX_POINTS and NK_LANE_MAX_POINTS, two mirrored pairs (two announced seeds):
    the serial path and the grouped solves -- those once more on route 2, where every member of a group launch
    (lh_metric_group) reduces its octant sums on its own, over `seg_plan`.  The residuals with the host draws made ahead by
    the worker and with NK_DRAW_AHEAD=0 are the same bits, both meet orc.draw_samples, and no worker thread outlives a run."""
    _host_spectrum(monkeypatch, lanes_off=True)
    monkeypatch.setattr(engine, "_HostDrawAhead", _CountingAhead)
    if grouped and not fixed_point:
        monkeypatch.setattr(engine, "SCATTER_FIXED_POINT_MAX_POINTS", 0)
    cf, x, _, lho, kw, _ = rc.sandwich_inputs(shape, "gaussian")
    model = FusedModel(shape, offset_mean=1.0, dtype=torch.float64, device="cuda:0", **kw)
    assert engine._sampling_lanes(model, 2) is None and not batched.ready(model)
    assert model.group_ready() == grouped
    assert model.scatter_fixed_point == fixed_point and model.group_scatter == fixed_point
    assert (model.seg_plan is not None) == (not fixed_point)
    print(f"ROUTE draw_samples {shape}: lanes None, batched False, grouped {grouped}, fixed point {fixed_point}")
    xl = LatentVec.from_dict(model, x)
    runs = []
    for ahead in (True, False):
        if not ahead:
            monkeypatch.setenv("NK_DRAW_AHEAD", "0")
        _CountingAhead.made = _CountingAhead.taken = 0
        random.push_sseq_from_seed(7)
        try:
            res, negs, n_total = draw_samples(model, xl, 2, True, lambda: AbsDeltaEnergyController(0.05, iteration_limit=6))
        finally:
            random.pop_sseq()
        assert (_CountingAhead.made, _CountingAhead.taken) == ((1, 2) if ahead else (0, 0))
        assert rc.draw_ahead_workers() == []
        assert n_total == 4 and negs == [False, True, False, True]
        runs.append(res)
    for a, b in zip(*runs):
        assert torch.equal(a.xi, b.xi) and torch.equal(a.small, b.small)
    res_o, negs_o = orc.draw_samples(cf, lho, x, 2, True, np.random.SeedSequence(7),
                                     lambda: orc.AbsDeltaEnergyController(0.05, iteration_limit=6))
    assert negs_o == [False, True, False, True]
    for name, run in zip(("ahead", "in place"), runs):
        for i, (r, ro) in enumerate(zip(run, res_o)):
            e = rc.rel_xi_spectrum(r.to_dict(), ro)
            print(f"ERR draw_samples {shape} fixed point {fixed_point} {name} residual {i}: {e:.1e}")
            assert e < 1e-7  # the ctol of test_sandwich_engine_vs_oracle: six CG iterations amplify rounding differences


# ---- route 6: generic operators beyond BIN_PLAN_MAX -----------------------------------------------------------------------------
def _distributors():
    """(name, operator, bin index of every target point): built by the caller AFTER the limit is lowered (the plans are cached
    per device on the instance)"""
    out = []
    for shape in ((16, 12), (8, 6, 10)):
        hsp = ift.RGSpace(shape).get_default_codomain()
        op = ift.PowerDistributor(hsp)
        out.append((f"PowerDistributor{shape}", op, np.array(op.domain[0].pindex)))
    dom = ift.RGSpace((6, 5))
    dofdex = np.arange(30).reshape(6, 5) % 4  # every dof 7 or 8 times
    out.append(("DOFDistributor(6, 5)", ift.DOFDistributor(ift.Field.from_raw(dom, dofdex)), dofdex))
    return out


def _assert_bins(name, got, ref, bound, n_max):
    err = np.abs(got.astype(rc.LD).reshape(-1) - ref.reshape(-1))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))))
    print(f"ERR {name}: longest bin {n_max}, largest error {float(err.max()):.1e}, error / bound {ratio:.2e}")
    assert np.all(err <= bound.reshape(-1))


def test_distributors_adjoint_through_atomics(monkeypatch):
    """ADJOINT of the distributors beyond BIN_PLAN_MAX against long-double bin sums within gamma(n_max) sum |terms|, and the
    package's own operator check on the device (its purity check holds such an application to the reference's device bar)."""
    monkeypatch.setattr(B, "BIN_PLAN_MAX", 0)
    ift.PowerSpace._cache.clear()
    rng = np.random.default_rng(31)
    for name, op, index in _distributors():
        x = rng.normal(size=op.target.shape) * 10.0 ** rng.uniform(-3, 3, size=op.target.shape)
        before = B.unordered_sums
        got = op.adjoint_times(ift.makeField(op.target, x, 0))
        assert got.device_id == 0 and op._bin_plans == {"cuda:0": None}  # the route: no plan, the atomics
        assert B.unordered_sums == before + 1
        ref, bound, n_max = rc.binned_reference(index, x, op.domain.shape[0])
        _assert_bins(name, got.asnumpy(), ref, bound, n_max)
        with random.Context(17):
            ift.extra.check_linear_operator(op, atol=1e-11, rtol=1e-11, force_device_ids=[0])


@pytest.mark.parametrize("space", [0, 1])
def test_partial_contraction_through_atomics(space, monkeypatch):
    """The partial sum over either space of a two-space domain beyond BIN_PLAN_MAX, as for the distributors."""
    monkeypatch.setattr(B, "BIN_PLAN_MAX", 0)
    dom = ift.DomainTuple.make((ift.RGSpace(7), ift.RGSpace((5, 6))))
    op = ift.ContractionOperator(dom, space)
    rng = np.random.default_rng(37)
    x = rng.normal(size=dom.shape) * 10.0 ** rng.uniform(-3, 3, size=dom.shape)
    before = B.unordered_sums
    got = op(ift.makeField(dom, x, 0))
    assert got.device_id == 0 and isinstance(op._kept_index["cuda:0"], torch.Tensor)  # the route: an index, not a plan
    assert B.unordered_sums == before + 1
    kept = np.arange(int(np.prod(op.target.shape))).reshape([1 if i in op._axes else n for i, n in enumerate(dom.shape)])
    ref, bound, n_max = rc.binned_reference(np.broadcast_to(kept, dom.shape), x, kept.size)
    assert n_max == (7 if space == 0 else 30)
    _assert_bins(f"ContractionOperator space {space}", got.asnumpy(), ref, bound, n_max)
    with random.Context(19):
        ift.extra.check_linear_operator(op, atol=1e-11, rtol=1e-11, force_device_ids=[0])
