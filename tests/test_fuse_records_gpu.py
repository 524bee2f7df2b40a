"""The records (L.Fuse, mirror of struct nk_fuse) that the routes of the metric application hand to the transform library.

lh_metric_accumulate_pair, lh_metric_group and batched.metric promise, per member, the kernels, the arithmetic and the bits
of the single route lh_metric_accumulate.  The kernels see a member only through its record, so the promise is pinned here
field by field: a member's record equals the single route's record for the same member in every field except the pointers
that belong to the member's place in the launch (its scratch set, its output), which are named case by case and must differ
from member to member.  The grids are the smallest that pair_ready() / group_ready() accept."""
import itertools

import pytest
import torch

from tests import group_cases as gc

pytestmark = pytest.mark.gpu

SCRATCH = ("damp", "dafield", "w8", "w8max")  # the scratch set of a member (FusedModel.scratch_sets)


def _set_pointers(model, count):
    return [{name: getattr(s, name).data_ptr() for name in SCRATCH} for s in model.scratch_sets(count)]


class _Spy:
    """Wraps the transform entry points of the routes: a byte copy of every record they receive, then the original call."""

    def __init__(self, monkeypatch):
        from nifty_amd import _lib as L
        from nifty_amd import backend as B
        from nifty_amd import batched

        self._fuse, self.calls = L.Fuse, []
        for module, name in ((B, "hartley_fused"), (B, "hartley_sandwich"), (B, "hartley_sandwich_pair"),
                             (B, "hartley_sandwich_group"), (batched, "_transform")):
            monkeypatch.setattr(module, name, self._wrap(name, getattr(module, name)))

    def _wrap(self, name, original):
        def wrapper(*args, **kw):
            records = []
            for arg in args:
                for f in (arg if isinstance(arg, (list, tuple)) else (arg,)):
                    if isinstance(f, self._fuse):
                        records.append(bytes(f))
            self.calls.append((name, records))
            return original(*args, **kw)

        return wrapper

    def take(self, name):
        """The records of the calls since the last take, all of which went to `name`, as dicts field -> value."""
        calls, self.calls = self.calls, []
        assert calls and all(n == name for n, _ in calls), [n for n, _ in calls]
        out = []
        for _, records in calls:
            for raw in records:
                f = self._fuse.from_buffer_copy(raw)
                out.append({field: getattr(f, field) for field, _ in self._fuse._fields_})
        return out


@pytest.fixture
def spy(monkeypatch):
    return _Spy(monkeypatch)


@pytest.fixture(scope="module", params=gc.PASS_SHAPES, ids=lambda p: "x".join(map(str, p[0])))
def problem(request):
    model, xs, ds, rs = gc.pass_setup(*request.param)
    assert model.pair_ready() and model.group_ready() and model.scatter_fixed_point
    return model, [model.linearize(x) for x in xs], ds, rs


def _same_except(single, member, differ):
    for field in single:
        if field not in differ:
            assert single[field] == member[field], field


def _all_differ(members, fields):
    for a, b in itertools.combinations(members, 2):
        for field in fields:
            assert a[field] is not None and a[field] != b[field], field


def _on_their_sets(model, members):
    for record, pointers in zip(members, _set_pointers(model, len(members))):
        assert {name: record[name] for name in SCRATCH} == pointers


@pytest.mark.parametrize("count", [2, 4])
def test_group_members_at_their_own_points(problem, spy, count):
    """lh_metric(lp_m, d, minus=x_m) as job m of a group: one direction, a linearisation point per member"""
    model, lps, ds, _ = problem
    d, keep, singles = ds[0], [], []
    for m in range(count):
        keep.append(model.lh_metric(lps[m], d, minus=lps[m].x))
        singles += spy.take("hartley_sandwich")
    keep.append(model.lh_metric_group(lps[0], [dict(d=d, addend=(lps[m].x, -1.0), lp=lps[m]) for m in range(count)]))
    members = spy.take("hartley_sandwich_group")
    assert len(singles) == len(members) == count
    for single, member in zip(singles, members):
        _same_except(single, member, SCRATCH + ("out",))
    _all_differ(members, SCRATCH + ("out", "in2", "xi", "amp", "afield", "addend"))
    _on_their_sets(model, members)


@pytest.mark.parametrize("count", [2, 4])
def test_group_members_of_conjugate_gradient_solves(problem, spy, count):
    """metric(lp, d_m, dot_out=..., cg_direction=...) as job m of a group: one linearisation point, every member with its
    direction (rewritten in the first pass), residual, workspace scalars, identity addend and curvature dot"""
    model, lps, ds, rs = problem
    jobs, _ = gc.class8_jobs(model, ds, rs, count)
    keep, singles = [], []
    for job in jobs:
        keep.append(model.metric(lps[0], job["d"], dot_out=job["dot_out"], cg_direction=job["cg_direction"]))
        singles += spy.take("hartley_sandwich")
    keep.append(model.lh_metric_group(lps[0], jobs))
    members = spy.take("hartley_sandwich_group")
    assert len(singles) == len(members) == count
    for single, member in zip(singles, members):
        assert single["cg_r"] is not None and single["value"] is not None
        _same_except(single, member, SCRATCH + ("out",))
    _all_differ(members, SCRATCH + ("out", "value", "in_", "addend", "cg_r", "cg_scal"))
    _on_their_sets(model, members)


@pytest.mark.parametrize("first", [True, False])
def test_pair_onto_one_output(problem, spy, first):
    """lh_metric_accumulate_pair onto `out`: sample A as lh_metric_accumulate(lpa, d, out, scale, first, cg_direction=...),
    sample B as lh_metric_accumulate(lpb, d, out, scale, False, identity=..., dot_out=...)"""
    from nifty_amd.engine import LatentVec

    model, lps, ds, rs = problem
    d, ws = gc._clone(ds[0]), gc._cg_ws(model, 0)
    ws.direction_small(d, rs[0])
    dot = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    out = LatentVec(torch.zeros_like(d.xi), torch.zeros_like(d.small))
    model.lh_metric_accumulate(lps[0], d, out, 0.125, first, cg_direction=(rs[0], ws))
    model.lh_metric_accumulate(lps[1], d, out, 0.125, False, identity=0.25, dot_out=dot)
    singles = spy.take("hartley_sandwich")
    model.lh_metric_accumulate_pair(lps[0], lps[1], d, out, 0.125, first, identity=0.25, dot_out=dot, cg_direction=(rs[0], ws))
    members = spy.take("hartley_sandwich_pair")
    assert len(singles) == len(members) == 2
    _same_except(singles[0], members[0], ())  # (sample A works on the model's own scratch set, like the single route)
    _same_except(singles[1], members[1], SCRATCH)
    # what the docstring says of the two samples: the direction update rides with A, the identity term and the dot with B
    a, b = members
    assert a["cg_r"] is not None and b["cg_r"] is None and a["accumulate"] == (0 if first else 1) and b["accumulate"] == 1
    assert (a["addend"], a["addend_scale"], a["value"]) == (None, 0.0, None)
    assert (b["addend"], b["addend_scale"], b["value"]) == (d.xi.data_ptr(), 0.25, dot.data_ptr())
    _all_differ(members, SCRATCH)
    _on_their_sets(model, members)


def test_pair_of_a_pairwise_sum(problem, spy):
    """lh_metric_accumulate_pair with `dests`: A stores a fresh vector and adds the prior term, B joins A's vector and a
    carried partial sum -- against lh_metric_accumulate(..., dest=...) of either sample"""
    from nifty_amd.engine import _Dest

    model, lps, ds, _ = problem
    d = ds[1]
    fresh, carried = torch.zeros_like(d.xi), torch.zeros_like(d.xi)
    dests = (_Dest(fresh, small=[], fresh=True), _Dest(fresh, accumulate=True, carries=(carried,), small=[]))
    model.lh_metric_accumulate(lps[0], d, None, 0.125, True, identity=1.0, dest=dests[0])
    model.lh_metric_accumulate(lps[1], d, None, 0.125, True, dest=dests[1])
    singles = spy.take("hartley_sandwich")
    model.lh_metric_accumulate_pair(lps[0], lps[1], d, None, 0.125, True, dests=dests, identity_first=1.0)
    members = spy.take("hartley_sandwich_pair")
    assert len(singles) == len(members) == 2
    _same_except(singles[0], members[0], ())
    _same_except(singles[1], members[1], SCRATCH)
    a, b = members
    assert (a["accumulate"], a["carry1"], a["addend"], a["addend_scale"]) == (0, None, d.xi.data_ptr(), 1.0)
    assert (b["accumulate"], b["carry1"], b["addend"], b["addend_scale"]) == (1, carried.data_ptr(), None, 0.0)
    assert a["out"] == b["out"] == fresh.data_ptr() and a["carry2"] is None and b["carry2"] is None
    _all_differ(members, SCRATCH)


def test_batched_members():
    """Member m of batched.metric against lh_metric_accumulate(lp_m, d_m, out_m, scale, True, addend=..., dot_out=...) on
    a 2-D grid, where the single route is two transforms (tangent -> metric weight, then the VJP epilogue): the members'
    records of either transform equal the single route's.  A member's scratch is a lane here, which also owns the field
    between the two transforms and the bin sums."""
    from nifty_amd import batched, random
    from nifty_amd.engine import FusedModel, LatentVec

    count = 3
    model = FusedModel((64, 64), offset_mean=2.0, likelihood="gaussian", icov=100.0, dtype=torch.float64, device="cuda:0")
    random.push_sseq_from_seed(13)
    try:
        model.set_data(model.signal(model.draw_prior()), 100.0)
        lps = [model.linearize(0.1 * model.draw_prior()) for _ in range(count)]
        ds = [model.draw_prior() for _ in range(count)]
    finally:
        random.pop_sseq()
    assert model.octant_vjp and not model.sandwich and model.seg_plan is not None
    dots = batched.scalars(count, model.device)
    outs = [LatentVec(torch.empty_like(d.xi), None) for d in ds]
    with pytest.MonkeyPatch.context() as patch:
        spy = _Spy(patch)
        singles = []
        for lp, d, out, dot in zip(lps, ds, outs, dots):
            model.lh_metric_accumulate(lp, d, out, 0.5, True, addend=(d, 1.0), dot_out=dot)
            singles.append(spy.take("hartley_fused"))
        batched.metric(model, batched.Scratch(model, count), [batched.Point.of(lp) for lp in lps], ds, outs, 0.5,
                       [(d, 1.0) for d in ds], dots)
        members = spy.take("_transform")
    assert [len(s) for s in singles] == [2] * count and len(members) == 2 * count
    tangent, vjp = members[:count], members[count:]
    for single, first, second in zip(singles, tangent, vjp):
        _same_except(single[0], first, ("damp", "dafield", "out"))
        _same_except(single[1], second, ("in_", "abar", "w8"))
        assert first["out"] == second["in_"]
    _all_differ(tangent, ("damp", "dafield", "out", "in_", "in2", "amp", "afield"))
    _all_differ(vjp, ("in_", "abar", "w8", "out", "value", "xi", "amp", "afield", "addend"))
