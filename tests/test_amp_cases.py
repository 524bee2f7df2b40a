"""Keeps tests/amp_cases.py honest without a GPU: its long-double reference against the oracle the goldens verify, the JVP
against the VJP, a plain float64 restatement inside the derived bounds at every case, every listed fault outside them, and
the launch geometry each size of the table was chosen for."""
import numpy as np
import pytest

from oracle import nifty_oracle as orc
from tests import amp_cases as ac

LD = ac.LD
CASE_IDS = list(ac.CASES)
U_LD = float(np.finfo(LD).eps) / 2


def test_constants_and_geometry_branches():
    src = open(ac.os.path.join(ac.CSRC, "nk_amp.hip")).read()
    assert (ac.AMP_THREADS, ac.EPT, ac.MAXG, ac.AMP_WAVES, ac.TILE) == (256, 4, 256, 4, 1024)
    assert "constexpr int AMP_WAVES = AMP_THREADS / 64;" in src and "const int tile = AMP_THREADS * EPT;" in src
    assert "#define NK_MAX_BATCH %d" % ac.NK_MAX_BATCH in open(ac.os.path.join(ac.CSRC, "..", "..", "include", "niftyk.h")).read()
    # the rules scan_geom / amp_grid and the chain counts mirror
    assert "int chunk = (m + ng - 1) / ng;" in src and "chunk = (chunk + tile - 1) / tile * tile;" in src
    assert "int g = (nb + AMP_THREADS - 1) / AMP_THREADS;" in src and "g > MAXG ? MAXG : g" in src
    assert "for (int off = 1; off < 64; off <<= 1)" in src and "for (int off = 32; off > 0; off >>= 1)" in src
    for nb, want in ac.GEOMETRY.items():
        assert ac.scan_geom(nb - 2) + (ac.amp_grid(nb),) == want, nb
    # what the sizes are there for
    assert [ac.scan_geom(nb - 2)[1] for nb in (1026, 1027, 2050, 2051)] == [1, 2, 2, 3]
    assert ac.amp_grid(256) == 1 and ac.amp_grid(257) == 2 and ac.amp_grid(65536) == ac.MAXG
    assert -(-65536 // (ac.MAXG * ac.AMP_THREADS)) == 1 and -(-65537 // (ac.MAXG * ac.AMP_THREADS)) == 2  # grid stride starts
    assert (258 - 2) // ac.EPT == 64 and (259 - 2 - 1) // ac.EPT == 64  # element 256 is the first of thread 64 = wavefront 1
    assert ac.scan_geom(262144) == (ac.TILE, ac.MAXG)
    chunk, ng = ac.scan_geom(262145)
    assert (chunk, ng) == (2 * ac.TILE, 129) and 262145 - 128 * chunk == 1  # a last workgroup of one element
    assert ac.scan_geom(524289)[0] == 3 * ac.TILE
    assert ac.scan_depth(7) == 32 and ac.c_scan(7) == 65 and ac.c_scan(524291) == 73
    assert ac.output_depth(7).tolist() == [0, 1, 2, 3, 4] and ac.output_depth(7, reverse=True).tolist() == [4, 3, 2, 1, 0]
    assert ac.output_depth(2051).max() == ac.scan_depth(2051) == ac.output_depth(2051)[40]
    assert set(ac.GEOMETRY) <= {c[1] for c in ac.CASES.values()}
    # the scratch behind the four rows of the state stays inside the documented 8 nb + 16 doubles
    assert "a.segs = amp_segs(nb, state);" in src and "return state + 16 + 4 * (size_t)nb;" in src
    assert "int ng = (nb + 1023) / 1024 + 1;" in src and "3 * (ng > MAXG ? MAXG : ng)" in src
    for nb in list(range(3, 5000)) + list(ac.GEOMETRY):
        assert ac.state_used(nb) <= 8 * nb + 16 and ac.scan_geom(nb - 2)[1] <= min((nb + 1023) // 1024 + 1, ac.MAXG)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_is_well_conditioned(cid):
    case = ac.get_case(cid)
    assert case.well_conditioned()
    geo = case.pr.geo
    assert np.isnan(geo[-2:]).all() and np.isfinite(geo[:-2]).all() and geo[2 * case.pr.nb] == 0.0
    assert np.all(np.isfinite(case.fb["amp"])) and np.all(case.fb["amp"] > 0)


# ---- against the oracle the goldens verify -----------------------------------------------------------------------------------
def _oracle_problem(shape):
    cf = orc.CFModel(shape, None, orc.CFParams())
    nb = cf.geo.nb
    geo = np.concatenate([cf.rel, cf.sc, cf.mult, cf.delta, [np.nan, np.nan]])
    hyp = np.array([*cf.ln["fluctuations"], *cf.ln["flexibility"], *cf.ln["asperity"], *cf.ln["zeromode"], *cf.slope_ms, cf.V])
    return cf, ac.Problem(nb, "oracle", geo=geo, hyp_values=hyp)


def _as_dict(pr, v):
    return {"asperity": v[0], "flexibility": v[1], "fluctuations": v[2], "loglogavgslope": v[3], "zeromode": v[4],
            "spectrum": v[5:].reshape(2, pr.m)}


@pytest.mark.parametrize("shape", [(64, 64), (12, 10, 14)])
def test_reference_agrees_with_the_oracle(shape):
    cf, pr = _oracle_problem(shape)
    lat = ac.latents(pr, 3)
    st = ac.forward(pr, lat)
    fb = ac.forward_bounds(pr, st)
    ost = cf.amplitude_state(_as_dict(pr, lat))
    ratio = ac.worst(ost["a"], st["amp"], fb["amp"])[0]
    print(f"oracle {shape} nb={pr.nb} fwd: {ratio:.3f} of the bound")
    assert ratio <= 1
    for name, dlat in ac.tangents(pr):
        dj = ac.jvp(pr, st, dlat, detail=True)
        ratio = ac.worst(cf.amplitude_jvp(ost, _as_dict(pr, dlat)), dj["damp"], ac.jvp_bounds(pr, st, fb, dj, dlat)[0])[0]
        assert ratio <= 1, (name, ratio)
    for name, abar in ac.cotangents(pr):
        dv = ac.vjp(pr, st, abar, detail=True)
        o = cf.amplitude_vjp(ost, abar)
        got = np.concatenate([[o["asperity"], o["flexibility"], o["fluctuations"], o["loglogavgslope"], o["zeromode"]],
                              o["spectrum"].reshape(-1)])
        ratio = ac.worst(got, dv["latbar"], ac.vjp_bounds(pr, st, fb, dv))[0]
        assert ratio <= 1, (name, ratio)


# ---- the JVP is the transpose of the VJP -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c for c in CASE_IDS if ac.CASES[c][1] <= 67])
def test_jacobian_by_jvp_is_the_transpose_of_the_vjp(cid):
    case = ac.get_case(cid)
    pr = case.pr
    cols = [case.jvp(ac.unit(pr.nsmall, k)) for k in range(pr.nsmall)]
    J = np.stack([c[0] for c in cols], axis=1)      # (nb, nsmall)
    mag = np.stack([c[2] for c in cols], axis=1)    # the JVP's magnitude companion, column by column
    JT = np.stack([case.vjp(ac.unit(pr.nb, b))[0] for b in range(pr.nb)], axis=1)  # (nsmall, nb)
    assert np.all(np.abs(J - JT.T) <= LD(1e-17) * mag), float(np.max(np.abs(J - JT.T) / np.where(mag > 0, mag, 1)))
    assert np.all(J[mag == 0] == 0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_reference_is_adjoint(cid):
    """<abar, J d> = <J^T abar, d> in long double.  Both sides are sequential long-double sums of at most 2 nb steps over the
    same terms: they agree within gamma(2 nb) in long double of sum |abar| mag(J d), mag the JVP's magnitude companion."""
    case = ac.get_case(cid)
    pr = case.pr
    dlat, abar = case.tangents[0][1], case.cotangents[0][1]
    damp, _, mag = case.jvp(dlat)
    latbar, _ = case.vjp(abar)
    lhs, rhs = np.sum(abar.astype(LD) * damp), np.sum(latbar * dlat.astype(LD))
    tol = 2 * pr.nb * U_LD * float(np.sum(np.abs(abar) * mag))
    print(f"adjoint {cid}: |lhs - rhs| = {float(abs(lhs - rhs)):.3e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol


# ---- a plain float64 restatement stays inside the bounds ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_float64_restatement_meets_the_bounds(cid):
    case = ac.get_case(cid)
    pr = case.pr
    h = ac.forward(pr, case.lat, T=np.float64)
    ratio = ac.worst(h["amp"], case.st["amp"], case.fb["amp"])[0]
    print(f"host {cid} fwd: {ratio:.3f} of the bound")
    assert ratio <= 1
    refs_j, refs_v = case.references()
    for name, dlat, damp, bound in refs_j:
        ratio = ac.worst(ac.jvp(pr, h, dlat), damp, bound)[0]
        assert ratio <= 1, (name, ratio)
    for name, abar, latbar, bound in refs_v:
        ratio = ac.worst(ac.vjp(pr, h, abar), latbar, bound)[0]
        assert ratio <= 1, (name, ratio)


# ---- every listed fault breaks a bound by 10 x -------------------------------------------------------------------------------
def _fault_ratio(case, mut):
    """largest |faulty - exact| / bound over the outputs of the case, the search ending at the first output beyond 10"""
    pr, best = case.pr, 0.0
    if mut in ("drop_x0_tile2", "drop_carry_c", "drop_tile_carry_c", "delta_shift"):
        best = ac.worst(ac.forward(pr, case.lat, mut=mut)["amp"], case.st["amp"], case.fb["amp"])[0]
        for name, dlat, damp, bound in case.references()[0]:
            if best >= 10:
                break
            best = max(best, ac.worst(ac.jvp(pr, case.st, dlat, mut=mut), damp, bound)[0])
    else:
        for name, abar, latbar, bound in case.references()[1]:
            if best >= 10:
                break
            best = max(best, ac.worst(ac.vjp(pr, case.st, abar, mut=mut), latbar, bound)[0])
    return best


@pytest.mark.parametrize("cid", CASE_IDS)
def test_mutations_are_caught(cid):
    case = ac.get_case(cid)
    seen = 0
    for mut in ac.MUTATIONS:
        if not ac.mutation_defined(mut, case.pr):
            continue
        ratio = _fault_ratio(case, mut)
        print(f"mutation {mut} at {cid}: {ratio:.3e} of the bound")
        assert ratio >= 10, (mut, ratio)
        seen += 1
    assert seen >= 2


def test_every_mutation_is_defined_somewhere():
    for mut in ac.MUTATIONS:
        n = sum(ac.mutation_defined(mut, ac.Problem(c[1], c[2], c[3])) for c in ac.CASES.values() if c[1] <= 2051 or c[1] == 262147)
        assert n >= 3, mut
