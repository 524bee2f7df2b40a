"""nk_amp_forward / nk_amp_jvp / nk_amp_vjp and their batch entries called directly through the C ABI on raw geo / hyp / lat
arrays, at every branch of the scan and reduction geometry, against the long-double model and the DERIVED bounds of
tests/amp_cases.py (tests/test_amp_cases.py keeps those honest on the host).

Every array sits between guard bands of NaN; state and outputs are prefilled with NaN, so an entry the kernels leave
unwritten or a read of the state before it is written shows; inputs must come back bit-identical.  Every case prints one line
per mode, `ERR kind=amp nb= geom= mode=fwd|jvp|vjp|adj err= bound= err_u= host=` followed by `ratio= zm= at= case=`: err and
bound at the element (and tangent / cotangent `at`) with the largest err / bound = ratio AMONG THE OUTPUTS THAT DEPEND ON THE
SCAN AND THE REDUCTIONS (every one but the zero mode's amp[0], damp[0], latbar[4], which are three products with a bound of a
few u: their largest ratio is `zm`, asserted like the rest), err_u that error in units of u |exact|, host the error of the
float64 restatement at ITS worst such element.  profiles/r10_amp_errors.txt keeps one run's lines."""
import ctypes

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from tests import amp_cases as ac
from tests.test_fused_transforms_gpu import GUARD, Guarded, stream

pytestmark = pytest.mark.gpu

LD = ac.LD
CASE_IDS = list(ac.CASES)
NAN = float("nan")


def ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def nan_out(n):
    return Guarded(np.full(n, NAN))


def state_buf(nb):
    return Guarded(nbytes=8 * (8 * nb + 16))  # all-ones bytes: NaN in every slot, the ticket included


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Device:
    """the static arrays of a Problem on the device and guarded calls of the three entries on one state"""

    def __init__(self, pr):
        self.pr, self.lib = pr, L.load()
        self.geo, self.hyp = Guarded(pr.geo), Guarded(pr.hyp)
        self.state = state_buf(pr.nb)
        self.inputs = [self.geo, self.hyp]

    def put(self, arr):
        g = Guarded(np.asarray(arr, dtype=np.float64))
        self.inputs.append(g)
        return g

    def forward(self, lat, state=None):
        out, st = nan_out(self.pr.nb), state or self.state
        L.check(self.lib.nk_amp_forward(self.pr.nb, self.geo.ptr, self.hyp.ptr, lat.ptr, st.ptr, out.ptr, stream()), "nk_amp_forward")
        return self._result(out, st)

    def jvp(self, lat, dlat, state=None):
        out, st = nan_out(self.pr.nb), state or self.state
        L.check(self.lib.nk_amp_jvp(self.pr.nb, self.geo.ptr, self.hyp.ptr, lat.ptr, st.ptr, dlat.ptr, out.ptr, stream()), "nk_amp_jvp")
        return self._result(out, st)

    def vjp(self, lat, abar, state=None):
        out, st = nan_out(self.pr.nsmall), state or self.state
        L.check(self.lib.nk_amp_vjp(self.pr.nb, self.geo.ptr, self.hyp.ptr, lat.ptr, st.ptr, abar.ptr, out.ptr, stream()), "nk_amp_vjp")
        return self._result(out, st)

    def _result(self, out, st):
        torch.cuda.synchronize()
        got = out.get()
        assert out.guards_intact() and st.guards_intact()
        assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} entries unwritten or NaN"
        return got

    def state_rest_untouched(self, state=None):
        """the unused fourth row and everything behind ac.state_used still hold the NaN prefill"""
        nb, raw = self.pr.nb, (state or self.state).buf[GUARD:]
        return bool((raw[8 * (16 + 3 * nb):8 * (16 + 4 * nb)] == 0xFF).all().item()
                    and (raw[8 * ac.state_used(nb):8 * (8 * nb + 16)] == 0xFF).all().item())

    def inputs_untouched(self):
        return all(g.guards_intact() and g.unchanged() for g in self.inputs)


def record(case, mode, w, host, at="-", zm=0.0):
    ratio, err, bound, exact = w
    err_u = err / (ac.U64 * exact) if exact > 0 else 0.0
    print(f"ERR kind=amp nb={case.pr.nb} geom={case.pr.family} mode={mode} err={err:.3e} bound={bound:.3e} err_u={err_u:.2f} "
          f"host={host:.3e} ratio={ratio:.3e} zm={zm:.3f} at={at} case={case.id}")


def split(got, exact, bound, zero_mode):
    """(worst of the outputs but the zero mode's, ratio of the zero mode's)"""
    rest = np.arange(len(got)) != zero_mode
    return ac.worst(got[rest], exact[rest], bound[rest]), ac.worst(got[[zero_mode]], exact[[zero_mode]], bound[[zero_mode]])[0]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_against_the_reference(cid):
    case = ac.get_case(cid)
    pr = case.pr
    assert case.well_conditioned()
    refs_j, refs_v = case.references()
    hst = ac.forward(pr, case.lat, T=np.float64)
    dev = Device(pr)
    lat = dev.put(case.lat)
    failures = []

    amp = dev.forward(lat)
    w, zm = split(amp, case.st["amp"], case.fb["amp"], 0)
    record(case, "fwd", w, split(hst["amp"], case.st["amp"], case.fb["amp"], 0)[0][1], zm=zm)
    if max(w[0], zm) > 1:
        failures.append(("fwd", w, zm))

    best, best_host, worst_zm, kept = (-1.0,), 0.0, 0.0, {}
    for name, dlat, damp, bound in refs_j:
        got = dev.jvp(lat, dev.put(dlat))
        w, zm = split(got, damp, bound, 0)
        worst_zm = max(worst_zm, zm)
        if w[0] > best[0]:
            best, at, best_host = w, name, split(ac.jvp(pr, hst, dlat), damp, bound, 0)[0][1]
        if max(w[0], zm) > 1:
            failures.append(("jvp", name, w, zm))
        if name == "dense":
            kept["damp"], kept["dlat"], kept["b_damp"] = got, dlat, bound
    record(case, "jvp", best, best_host, at, worst_zm)

    best, worst_zm = (-1.0,), 0.0
    for name, abar, latbar, bound in refs_v:
        got = dev.vjp(lat, dev.put(abar))
        w, zm = split(got, latbar, bound, 4)
        worst_zm = max(worst_zm, zm)
        if w[0] > best[0]:
            best, at, best_host = w, name, split(ac.vjp(pr, hst, abar), latbar, bound, 4)[0][1]
        if max(w[0], zm) > 1:
            failures.append(("vjp", name, w, zm))
        if name == "dense":
            kept["latbar"], kept["abar"], kept["b_latbar"] = got, abar, bound
    record(case, "vjp", best, best_host, at, worst_zm)

    # <abar, damp> = <latbar, dlat> from the DEVICE outputs, summed in long double; each side may be off by its bound
    lhs = np.sum(kept["abar"].astype(LD) * kept["damp"].astype(LD))
    rhs = np.sum(kept["latbar"].astype(LD) * kept["dlat"].astype(LD))
    tol = float(np.sum(np.abs(kept["abar"]) * kept["b_damp"]) + np.sum(np.abs(kept["dlat"]) * kept["b_latbar"]))
    hl = np.sum(kept["abar"].astype(LD) * ac.jvp(pr, hst, kept["dlat"]).astype(LD))
    hr = np.sum(ac.vjp(pr, hst, kept["abar"]).astype(LD) * kept["dlat"].astype(LD))
    w = (float(abs(lhs - rhs)) / tol, float(abs(lhs - rhs)), tol, float(abs(lhs)))
    record(case, "adj", w, float(abs(hl - hr)), "dense")
    if w[0] > 1:
        failures.append(("adj", w))

    assert dev.inputs_untouched()
    assert not failures, failures


@pytest.mark.parametrize("cid", CASE_IDS)
def test_order_reuse_and_repeatability(cid):
    """No reference here: only bits.  On ONE state: forward, JVP, VJP, JVP, VJP (both derivatives write tmp); forward at A, at B,
    at A again (the ticket, stale partials and aggregates); the derivatives after a second forward at the same point.  On
    fresh NaN states: three runs of the chain give the same bits, and the kernels write nothing outside ac.state_used."""
    _, nb, family, hyp, extreme = ac.CASES[cid]
    pr = ac.Problem(nb, family, hyp)
    dev = Device(pr)
    lat_a, lat_b = dev.put(ac.latents(pr, 0, extreme)), dev.put(ac.latents(pr, 1, extreme))
    dlat, abar = dev.put(ac.tangents(pr)[0][1]), dev.put(ac.cotangents(pr)[0][1])
    amp = dev.forward(lat_a)
    damp, latbar = dev.jvp(lat_a, dlat), dev.vjp(lat_a, abar)
    assert np.array_equal(bits(dev.jvp(lat_a, dlat)), bits(damp))
    assert np.array_equal(bits(dev.vjp(lat_a, abar)), bits(latbar))
    amp_b = dev.forward(lat_b)
    assert not np.array_equal(amp_b, amp)
    assert np.array_equal(bits(dev.forward(lat_a)), bits(amp))
    assert np.array_equal(bits(dev.vjp(lat_a, abar)), bits(latbar))
    assert np.array_equal(bits(dev.jvp(lat_a, dlat)), bits(damp))
    assert np.array_equal(bits(dev.forward(lat_a)), bits(amp))
    assert np.array_equal(bits(dev.jvp(lat_a, dlat)), bits(damp))
    assert np.array_equal(bits(dev.vjp(lat_a, abar)), bits(latbar))
    for _ in range(2):
        fresh = state_buf(nb)
        assert np.array_equal(bits(dev.forward(lat_a, fresh)), bits(amp))
        assert np.array_equal(bits(dev.jvp(lat_a, dlat, fresh)), bits(damp))
        assert np.array_equal(bits(dev.vjp(lat_a, abar, fresh)), bits(latbar))
        assert dev.state_rest_untouched(fresh)
    assert dev.state_rest_untouched() and dev.inputs_untouched()


# ---- batches ---------------------------------------------------------------------------------------------------------------
_members = {}


def batch_members(nb):
    """NK_MAX_BATCH distinct points with a tangent and a cotangent each and their long-double results, computed once per nb"""
    if nb not in _members:
        from concurrent.futures import ThreadPoolExecutor

        pr = ac.Problem(nb)

        def member(k):
            lat = ac.latents(pr, 20 + k, extreme=(k == 5))
            dlat, abar = ac.tangents(pr, 20 + k)[0][1], ac.cotangents(pr, 20 + k)[0][1]
            st = ac.forward(pr, lat)
            fb = ac.forward_bounds(pr, st)
            dj, dv = ac.jvp(pr, st, dlat, detail=True), ac.vjp(pr, st, abar, detail=True)
            return dict(lat=lat, dlat=dlat, abar=abar, amp=st["amp"], b_amp=fb["amp"], damp=dj["damp"],
                        b_damp=ac.jvp_bounds(pr, st, fb, dj, dlat)[0], latbar=dv["latbar"], b_latbar=ac.vjp_bounds(pr, st, fb, dv))

        with ThreadPoolExecutor(ac.NK_MAX_BATCH) as ex:
            _members[nb] = (pr, list(ex.map(member, range(ac.NK_MAX_BATCH))))
    return _members[nb]


@pytest.mark.parametrize("count", [3, ac.NK_MAX_BATCH])
@pytest.mark.parametrize("nb", [1027, 262147])
def test_batches(nb, count):
    pr, members = batch_members(nb)
    members = members[:count]
    dev = Device(pr)
    lib, geo, hyp = dev.lib, dev.geo.ptr, dev.hyp.ptr
    lat, dlat, abar = ([dev.put(m[k]) for m in members] for k in ("lat", "dlat", "abar"))
    states = [state_buf(nb) for _ in members]
    amp, damp, latbar = ([nan_out(n) for _ in members] for n in (nb, nb, pr.nsmall))
    P = lambda gs: ptrs([g.ptr for g in gs])  # noqa: E731
    L.check(lib.nk_amp_forward_batch(nb, geo, hyp, count, P(lat), P(states), P(amp), stream()))
    L.check(lib.nk_amp_jvp_batch(nb, geo, hyp, count, P(lat), P(states), P(dlat), P(damp), stream()))
    L.check(lib.nk_amp_vjp_batch(nb, geo, hyp, count, P(lat), P(states), P(abar), P(latbar), stream()))
    torch.cuda.synchronize()
    for k, m in enumerate(members):
        assert all(g.guards_intact() for g in (states[k], amp[k], damp[k], latbar[k]))
        for mode, got, ref, bound in (("fwd", amp[k].get(), m["amp"], m["b_amp"]), ("jvp", damp[k].get(), m["damp"], m["b_damp"]),
                                      ("vjp", latbar[k].get(), m["latbar"], m["b_latbar"])):
            assert not np.isnan(got).any()
            ratio = ac.worst(got, ref, bound)[0]
            print(f"batch nb={nb} count={count} member={k} mode={mode}: {ratio:.3e} of the bound")
            assert ratio <= 1, (k, mode, ratio)
        single = Device.__new__(Device)  # the single entries on a state of their own, sharing the static arrays
        single.pr, single.lib, single.geo, single.hyp, single.state = pr, lib, dev.geo, dev.hyp, state_buf(nb)
        assert np.array_equal(bits(single.forward(lat[k])), bits(amp[k].get()))
        assert np.array_equal(bits(single.jvp(lat[k], dlat[k])), bits(damp[k].get()))
        assert np.array_equal(bits(single.vjp(lat[k], abar[k])), bits(latbar[k].get()))
    assert dev.inputs_untouched()


# ---- argument checks -------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """every refusal is NK_ERR_INVALID, names the entry, and launches nothing: state and outputs keep their NaN prefill"""
    nb = 7
    pr = ac.Problem(nb)
    dev = Device(pr)
    lib, s_ = dev.lib, stream()
    n = ac.NK_MAX_BATCH + 1
    lat = [dev.put(ac.latents(pr, k)) for k in range(n)]
    dlat = [dev.put(ac.tangents(pr, k)[0][1]) for k in range(n)]
    abar = [dev.put(ac.cotangents(pr, k)[0][1]) for k in range(n)]
    states = [state_buf(nb) for _ in range(n)]
    outs = [nan_out(pr.nsmall) for _ in range(n)]  # long enough for either kind of output
    geo, hyp = dev.geo.ptr, dev.hyp.ptr

    def refused(rc, name):
        assert rc == L.NK_ERR_INVALID, (name, rc)
        assert name in lib.nk_last_error().decode(), (name, lib.nk_last_error())

    singles = {"nk_amp_forward": lambda a: lib.nk_amp_forward(a["nb"], a["geo"], a["hyp"], a["lat"], a["state"], a["out"], s_),
               "nk_amp_jvp": lambda a: lib.nk_amp_jvp(a["nb"], a["geo"], a["hyp"], a["lat"], a["state"], a["in"], a["out"], s_),
               "nk_amp_vjp": lambda a: lib.nk_amp_vjp(a["nb"], a["geo"], a["hyp"], a["lat"], a["state"], a["in"], a["out"], s_)}
    ins = {"nk_amp_forward": None, "nk_amp_jvp": dlat, "nk_amp_vjp": abar}
    for name, call in singles.items():
        good = dict(nb=nb, geo=geo, hyp=hyp, lat=lat[0].ptr, state=states[0].ptr, out=outs[0].ptr,
                    **({"in": ins[name][0].ptr} if ins[name] else {}))
        refused(call({**good, "nb": 2}), name)
        for key in good:
            if key != "nb":
                refused(call({**good, key: None}), name)

    batches = {
        "nk_amp_forward": lambda a: lib.nk_amp_forward_batch(a["nb"], a["geo"], a["hyp"], a["count"], a["lat"], a["state"], a["out"], s_),
        "nk_amp_jvp": lambda a: lib.nk_amp_jvp_batch(a["nb"], a["geo"], a["hyp"], a["count"], a["lat"], a["state"], a["in"], a["out"], s_),
        "nk_amp_vjp": lambda a: lib.nk_amp_vjp_batch(a["nb"], a["geo"], a["hyp"], a["count"], a["lat"], a["state"], a["in"], a["out"], s_)}
    for name, call in batches.items():
        def table(gs, count, null=None, same=None):
            v = [g.ptr for g in gs[:count]]
            if null is not None:
                v[null] = None
            if same is not None:
                v[same[1]] = v[same[0]]
            return ptrs(v)

        def args(count, **change):
            a = dict(nb=nb, geo=geo, hyp=hyp, count=count, lat=table(lat, max(count, 1)), state=table(states, max(count, 1)),
                     out=table(outs, max(count, 1)))
            if ins[name]:
                a["in"] = table(ins[name], max(count, 1))
            a.update(change)
            return a

        refused(call(args(3, nb=2)), name)
        for key in ("geo", "hyp", "lat", "state", "out") + (("in",) if ins[name] else ()):
            refused(call(args(3, **{key: None})), name)
        refused(call(args(0)), name)
        refused(call(args(n)), name)  # NK_MAX_BATCH + 1
        for key, gs in (("lat", lat), ("state", states), ("out", outs)) + ((("in", ins[name]),) if ins[name] else ()):
            refused(call(args(3, **{key: table(gs, 3, null=1)})), name)
        refused(call(args(3, state=table(states, 3, same=(0, 2)))), name)
        refused(call(args(3, out=table(outs, 3, same=(1, 2)))), name)

    torch.cuda.synchronize()
    for g in states:
        assert bool((g.buf == 0xFF).all().item())
    for g in outs:
        assert g.unchanged() and g.guards_intact()
    assert dev.inputs_untouched()
