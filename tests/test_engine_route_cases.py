"""Host checks of tests/engine_route_cases.py: the case table against the binning PowerSpace and the oracle produce today (a
change of the binning shows as a failing table, not as a route that is silently no longer reached), the forcing against the
constants it lowers, and the helpers of the draw and operator tests on data with a known answer."""
import numpy as np
import pytest

import nifty_amd as ift
from nifty_amd import backend as B
from nifty_amd import engine
from oracle import nifty_oracle as orc
from tests import engine_route_cases as rc


@pytest.mark.parametrize("shape,distances", list(rc.GEOMETRIES), ids=lambda v: "x".join(map(str, v)) if v else "unit")
def test_geometry_table(shape, distances):
    nb, k2table, equal01 = rc.GEOMETRIES[(shape, distances)]
    hsp = ift.RGSpace(shape, distances).get_default_codomain()
    ps = ift.PowerSpace(hsp)
    assert ps.shape[0] == nb
    assert (ps._data.get("k2table") is not None) == k2table
    assert (hsp.distances[0] == hsp.distances[1]) == equal01
    assert orc.power_geometry(shape, distances).nb == nb  # both sides of every comparison bin alike


def test_issue_geometries_are_in_the_table():
    want = {((64, 64, 128), None): (4492, True), ((64, 64, 128), (1 / 64,) * 3): (4390, False),
            ((64, 64, 128), (0.02, 0.02, 0.013)): (28966, False), ((64, 64, 128), (0.02, 0.03, 0.013)): (55995, False),
            ((64, 128), (0.02, 0.013)): (2134, False), ((30, 50), (0.02, 0.013)): (413, False)}
    for key, val in want.items():
        assert rc.GEOMETRIES[key][:2] == val


def test_case_table_is_consistent():
    names = [c.name for c in rc.ALL_CASES]
    assert len(set(names)) == len(names)
    assert {c.route for c in rc.SEEDED_CASES} == {1, 2, 3, 4} and {c.route for c in rc.PAIR_CASES} == {1, 2}
    mods = {"engine": engine, "backend": B}
    for c in rc.ALL_CASES:
        nb, k2table, equal01 = rc.GEOMETRIES[(c.shape, c.distances)]
        assert set(c.flags) <= set(rc.FLAG_NAMES) and c.flags, c.name
        assert max(c.shape) <= 128 and c.dtype in ("float64", "float32")
        assert (c.dtype == "float32") == (c.fp32_class is not None), c.name
        for mod, name, value in c.attrs:
            assert value < getattr(mods[mod], name), c.name  # lowered, and the constant exists
        for name, _ in c.env:
            assert name == "NK_SEGMENT_SUM"
        assert c.flags.get("seg_plan", True) == (c.env != rc.NO_SEGMENT_SUM) or not c.flags.get("octant_vjp", True), c.name
        # what the flags claim about the geometry follows from the table
        if "merge_swapped" in c.flags:
            assert c.flags["merge_swapped"] == int(len(c.shape) == 3 and c.shape[0] == c.shape[1] and equal01), c.name
        if c.flags.get("bin_k2"):
            assert k2table and len(c.shape) == 3 and max(c.shape) >= 64, c.name
        if c.route in (1, 4) and len(c.shape) == 3:
            assert not k2table, c.name  # no shell scatter without the k^2 table: bin_k2 is None by geometry
        # every route is forced the way the engine selects it
        if c.route == 2:
            assert c.attrs == rc.NO_FIXED_POINT and c.distances is None
        if c.route == 3:
            assert c.attrs == rc.NO_BIN_PLAN
        if c.route == 4:
            assert c.env == rc.NO_SEGMENT_SUM
        if c.route == 1:
            assert not c.attrs and not c.env  # the geometry alone
    # the two merge decisions of nk_octant_scatter, and the combination it must not merge (equal axes, unequal distances)
    r4 = [c for c in rc.SEEDED_CASES if c.route == 4 and len(c.shape) == 3]
    assert {c.flags["merge_swapped"] for c in r4} == {0, 1}
    assert any(c.shape[0] == c.shape[1] and c.flags["merge_swapped"] == 0 for c in r4)
    assert {c.flags["merge_swapped"] for c in rc.SEEDED_CASES if c.route == 1 and "merge_swapped" in c.flags} == {0, 1}
    # route 2 both ways: the fixed-order sums, and the floating-point shell scatter; pairs only on the reproducible one
    assert {c.flags["seg_plan"] for c in rc.SEEDED_CASES if c.route == 2} == {True, False}
    assert all(c.flags["seg_plan"] for c in rc.PAIR_CASES)


def test_the_limits_the_cases_lower():
    assert engine.SCATTER_FIXED_POINT_MAX_POINTS == 1 << 18
    assert B.BIN_PLAN_MAX == 1 << 28
    assert engine.SPECTRUM_DEVICE_DRAW_MAX_POINTS > 0  # (NK_SPECTRUM_DEVICE_DRAW_MAX_POINTS may move it)
    assert engine._HostDrawAhead.THREAD_PREFIX


def test_fp32_bounds_stay_below_the_ceiling():
    for name, (tol, mtol) in rc.FP32_TOL.items():
        assert 0 < tol <= rc.FP32_CEILING and 0 < mtol <= rc.FP32_CEILING, name
    assert rc.FP32_TOL["default"] == (1e-5, 3e-6)
    assert {c.fp32_class for c in rc.ALL_CASES if c.fp32_class} <= set(rc.FP32_TOL)


def test_per_key_relerr_is_lat_relerr_key_by_key():
    from tests import goldenlib as gl

    rng = np.random.default_rng(1)
    b = {"xi": rng.normal(size=(4, 5)) * 100.0, "spectrum": rng.normal(size=(2, 3)), "zeromode": np.array(1e-4)}
    a = {k: v + 1e-6 * rng.normal(size=v.shape) for k, v in b.items()}
    per = rc.per_key_relerr(a, b)
    assert set(per) == set(b) and max(per.values()) == gl.lat_relerr(a, b)
    assert per["zeromode"] == abs(float(a["zeromode"] - b["zeromode"])) / (1e-3 * np.max(np.abs(b["xi"])))


def test_device_draw_bar():
    ref = np.array([0.5, -1.25, 3.7, -4.0, 3.6])
    assert rc.device_draw_matches(ref.copy(), ref) == (True, 2, 0)
    near = ref.copy()
    near[2] = np.nextafter(np.nextafter(ref[2], 9.0), 9.0)  # 2 ulp, in the tail
    assert rc.device_draw_matches(near, ref) == (True, 2, 1)
    far = ref.copy()
    far[3] = ref[3] * (1 + 2.0 ** -49)  # 8 ulp
    assert rc.device_draw_matches(far, ref)[0] is False
    body = ref.copy()
    body[4] = np.nextafter(ref[4], 9.0)  # 1 ulp, but outside the tail
    assert rc.device_draw_matches(body, ref)[0] is False
    assert rc.device_draw_matches(ref.astype(np.float32), ref) == (True, 2, 0)


def test_numpy_prior_draw_follows_the_latent_keys():
    vals, state = rc.numpy_prior_draw(np.random.SeedSequence(4), (3, 4), 7)
    rng = np.random.default_rng(np.random.SeedSequence(4))
    for k in ("asperity", "flexibility", "fluctuations", "loglogavgslope"):
        assert vals[k] == rng.normal()
    assert np.array_equal(vals["spectrum"], rng.normal(size=(2, 5)))
    assert np.array_equal(vals["xi"], rng.normal(size=(3, 4)))
    assert vals["zeromode"] == rng.normal() and state == rng.bit_generator.state
    # the host part of a draw made ahead is the same stream up to xi
    class _Model:
        nb = 7
        host_draws_before_xi = engine.FusedModel.host_draws_before_xi

    ahead, _, _ = _Model().host_draws_before_xi(np.random.SeedSequence(4))
    assert all(np.array_equal(ahead[k], vals[k]) for k in ahead) and "xi" not in ahead


def test_no_draw_ahead_worker_is_left_by_a_finished_pool():
    class _Model:
        nb = 50
        host_draws_before_xi = engine.FusedModel.host_draws_before_xi

    seeds = np.random.SeedSequence(2).spawn(2)
    ahead = engine._HostDrawAhead(_Model(), seeds)
    for sq in seeds:
        assert ahead.take(sq) is not None
    ahead.close()
    assert rc.draw_ahead_workers() == []


def test_binned_reference():
    index = np.array([[0, 2, 2], [2, 0, 2]])
    values = np.array([[1.0, 2.0 ** -60, 1.0], [-1.0, 3.0, 2.0 ** -60]])
    ref, bound, n_max = rc.binned_reference(index, values, 4)
    assert n_max == 4 and ref.dtype == rc.LD
    assert ref[0] == 4.0 and ref[1] == 0.0 and ref[3] == 0.0 and bound[1] == 0.0
    assert ref[2] == rc.LD(2.0) ** -59  # what fp64 left-to-right addition would lose
    assert np.isclose(float(bound[2]), 4 * 2.0 ** -53 * 2.0, rtol=1e-12)
    # the host operators sum what the reference sums
    dom = ift.RGSpace((6, 5))
    dofdex = np.arange(30).reshape(6, 5) % 4
    op = ift.DOFDistributor(ift.Field.from_raw(dom, dofdex))
    x = np.random.default_rng(3).normal(size=(6, 5))
    ref, bound, n_max = rc.binned_reference(dofdex, x, 4)
    assert n_max == 8
    assert np.all(np.abs(op.adjoint_times(ift.makeField(dom, x)).asnumpy() - ref) <= bound)


def test_purity_check_knows_the_unordered_sums():
    """extra._same_answer_twice: equal bits, except for an application that counted an order-dependent sum -- that one is
    held to the reference's bar for device results (rtol 1e-7), not let off."""
    from nifty_amd import extra

    dom = ift.RGSpace(4)

    class Wobbly(ift.LinearOperator):
        def __init__(self, step, counted):
            self._domain = self._target = ift.DomainTuple.make(dom)
            self._capability = self.TIMES
            self._step, self._counted, self._calls = step, counted, 0

        def apply(self, x, mode):
            self._check_input(x, mode)
            self._calls += 1
            if self._counted:
                B.note_unordered_sum()
            return x * (1.0 + self._step * self._calls)

    x = ift.makeField(dom, np.arange(1.0, 5.0))
    extra._same_answer_twice(Wobbly(0.0, False), x)
    extra._same_answer_twice(Wobbly(1e-15, True), x)
    with pytest.raises(AssertionError):
        extra._same_answer_twice(Wobbly(1e-15, False), x)
    with pytest.raises(AssertionError):
        extra._same_answer_twice(Wobbly(1e-5, True), x)
