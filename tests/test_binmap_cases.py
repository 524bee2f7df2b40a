"""Keeps tests/binmap_cases.py honest without a GPU: the geometry against PowerSpace, the restated shell walk against the
set it has to cover at every shape of the device test, the exact fixed-point restatement against the long-double sums and
np.bincount, and deliberate faults written into copies of the restatement -- each one caught by the coverage check, by changed
bits or by an exceeded bound.  The lines `FAULT name caught= ratio=` are what profiles/r11_binmap_errors.txt keeps."""
import math

import numpy as np
import pytest

from tests import binmap_cases as bc

LD = bc.LD
SHELL_IDS = ["x".join(map(str, s)) for s in bc.SHELL_SHAPES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_constants_and_the_lines_the_restatement_mirrors():
    assert (bc.NK_SHELL_BINS, bc.NK_SHELL_SPLITS, bc.NK_SHELL_NU, bc.NG, bc.MARG_ROWS, bc.PROD_THREADS) == (4096, 16, 8, 16, 128, 256)
    for line in ("for (int a = s; a < o.Ah; a += NK_SHELL_SPLITS) {", "if (ra >= khi) break;",
                 "const int b_hi = last ? o.Mh : min(o.Mh, nk_isqrt_ceil(khi - ra));",
                 "const int b_lo = nk_isqrt_ceil(klo - hc2 - ra);", "for (int b0 = b_lo + grp; b0 < b_hi; b0 += NG * NU) {",
                 "cc[u] = nk_isqrt_ceil(klo - r2) + l16;", "ce[u] = on ? (last ? o.Ch : min(o.Ch, nk_isqrt_ceil(khi - r2))) : 0;",
                 "for (int c = cc[u] + 16; c < ce[u]; c += 16)",
                 "const int khi = bin0 + NK_SHELL_BINS < nb ? bin_k2[bin0 + NK_SHELL_BINS] : 0x7fffffff;"):
        assert bc.VEC_SRC.count(line) >= 2, line  # the floating-point and the fixed-point kernel walk alike
    for line in ("if (finite && gmax > 0.0) (void)frexp(gmax, &e);", "e = max(e, %d);" % bc.E_MIN,
                 "const double scale = ldexp(1.0, 44 - e), inv = ldexp(1.0, e - 44);", "const double magic = 6755399441055744.0;",
                 "dst[i] = ok ? (double)(long long)acc[i] * inv", "const int64_t pstride = (nb + 31) / 32 * 32;",
                 "return nk_fold_copies(nb, NK_SHELL_SPLITS, pstride, scratch, abar, stream);",
                 "for (int c = 0; c < copies; ++c) s += src[c * stride + i];", ">= (1 << 24))"):
        assert line in bc.VEC_SRC, line
    assert math.isinf(math.ldexp(1.0, 44 - bc.E_MIN) * 2) and math.ldexp(1.0, 44 - bc.E_MIN) == 2.0 ** 1023
    assert math.ldexp(1.0, bc.E_MIN - 44) == 2.0 ** -1023 > 0  # the quantum itself is an exact (subnormal) double
    for line in ("for (int64_t c = lane; c < C; c += 64)", "const int64_t a0 = (int64_t)blockIdx.y * MARG_ROWS",
                 "for (int64_t c = 0; c < chunks; ++c) s += partial[c * Bn + b];",
                 "const int64_t b = (int64_t)blockIdx.x * PROD_THREADS + threadIdx.x;"):
        assert line in bc.PROD_SRC, line
    header = open(bc.os.path.join(bc.ROOT, "include", "niftyk.h")).read()
    assert "scratch: >= 64*(nb+32) doubles" in header and "max(frexp exponent of *w8max, %d)" % bc.E_MIN in header
    for nb in list(range(1, 300)) + [4096, 4097, 10153]:  # what the launcher uses of the documented scratch
        assert bc.NK_SHELL_SPLITS * ((nb + 31) // 32 * 32) <= 64 * (nb + 32)


@pytest.mark.parametrize("shape,distances", [((64, 64, 64), None), ((9, 9), None), ((15, 15, 15), None), ((600,), None),
                                             ((16, 16, 256), (16.0, 16.0, 1.0)), ((8, 12), (3.0, 2.0))])
def test_geometry_agrees_with_power_space(shape, distances):
    import nifty_amd as ift

    hsp = ift.RGSpace(shape, distances=distances).get_default_codomain()
    assert hsp.equal_distances()
    ps = ift.PowerSpace(hsp)
    geo = bc.geometry(shape)
    assert geo.nb == ps.shape[0] and np.array_equal(np.asarray(ps.pindex), geo.pidx)
    assert np.array_equal(np.asarray(ps.rho), geo.rho)
    assert np.array_equal(np.nonzero(hsp._k2_flags())[0], geo.bin_k2)
    assert np.array_equal(geo.pidx8, geo.k2table[geo.k2[geo.osl]]) and geo.pidx8.shape == geo.oshape


def test_the_shapes_are_the_branches_they_stand_for():
    for shape, (nb, shells) in bc.SHELL_SHAPES.items():
        geo = bc.geometry(shape)
        assert (geo.nb, geo.shells) == (nb, shells) and geo.k2_supported, shape
        assert np.all(np.diff(geo.bin_k2) > 0) and geo.count8.min() >= 1
    g = bc.geometry((16, 16, 256))
    assert g.Ah == 9 < bc.NK_SHELL_SPLITS and bc.walk_counts(g)[1] == 115 > 16 and not bc.walk_counts(g)[0][:, 9:].any()
    assert bc.walk_counts(bc.geometry((128, 128, 128)))[0].max() == 13212 < 1 << 18
    assert bc.geometry((8191,)).nb == bc.NK_SHELL_BINS and bc.geometry((8191,)).Ch - 1 == 4095
    assert all(n % 2 for n in (33, 31, 255)) and len({64, 64, 64}) == 1 and bc.geometry((129, 255)).Ah == 1
    assert (8192 // 2) ** 2 == bc.K2_LIMIT and (8191 // 2) ** 2 < bc.K2_LIMIT  # (8192,): (Ch - 1)^2 = 2^24 is refused
    assert [bc.isqrt_ceil(x) for x in (-3, 0, 1, 2, 4, 5, 16777215, 16777216)] == [0, 0, 1, 2, 2, 3, 4096, 4096]
    # what the other lists are there for
    assert any(n // 2 + 1 >= 256 for s in bc.SCATTER_SHAPES for n in s[-1:]) and any(all(n % 2 for n in s) for s in bc.SCATTER_SHAPES)
    sizes = bc.PRODUCT_SIZES
    abc = [bc.ProductCase(s).abc(w) for s in sizes for w in range(len(s))]
    assert {128, 129, 257} <= {a for a, _, _ in abc} and {1, 63, 64, 65, 200} <= {c for _, _, c in abc}
    assert {1, 255, 256, 257, 600} <= {b for _, b, _ in abc} and {1, 2, 3} == {len(s) for s in sizes}
    assert any(1 in s for s in sizes) and max(int(np.prod(s)) for s in sizes) < 3_000_000
    for s in sizes:
        for w in range(len(s)):
            steps, k = bc.ProductCase(s).marginal_steps(w)
            assert 1 <= steps <= k, (s, w)


@pytest.mark.parametrize("shape", list(bc.SHELL_SHAPES), ids=SHELL_IDS)
def test_walk_covers_every_octant_point_once(shape):
    geo = bc.geometry(shape)
    failures, visits = bc.walk_coverage(geo)
    assert failures == []                # every (shell, split) visits exactly its set, each point once
    assert np.all(visits == 1)           # and every octant point belongs to exactly one workgroup


def test_fixed_rn_is_the_exact_rounding():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.normal(size=2000), (2.0 * rng.integers(-1 << 42, 1 << 42, size=2000) + 1.0) * 2.0 ** -44,
                        [0.0, -0.0, 0.5 * 2.0 ** -43, -0.5 * 2.0 ** -43, 1.5 * 2.0 ** -43, -1.5 * 2.0 ** -43, 2.5 * 2.0 ** -43, 1.0,
                         -1.0, 5e-324, -5e-324, 2.0 ** -60]])
    for shift in (43, 44, 30):
        got = bc.fixed_rn(v, shift)
        assert got.tolist() == [bc.fixed_rn_exact(x, shift) for x in v]
    assert bc.fixed_rn(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]), 0).tolist() == [0, 2, 2, 0, -2, -2]
    tiny = np.ldexp(rng.integers(-1 << 20, 1 << 20, size=500).astype(np.float64), -1074)
    assert bc.fixed_rn(tiny, 1023).tolist() == [bc.fixed_rn_exact(x, 1023) for x in tiny] == [0] * 500
    # the magic-number conversion of the kernel, restated: (x + 1.5 2^52) - 1.5 2^52 as integers of the bit patterns
    magic = 6755399441055744.0
    x = np.ldexp(v, 43)
    trick = (x + magic).view(np.int64) - np.array(magic).view(np.int64)
    assert np.array_equal(trick, bc.fixed_rn(v, 43))
    assert [bc.fixed_exponent(w) for w in (1.0, 0.75, 8.0, 0.0, 2.0 ** -979, 2.0 ** -980, 2.0 ** -981, 5e-324, 1.7e308)] == \
        [1, 0, 4, 0, -978, -979, -979, -979, 1024]
    with np.errstate(over="ignore"):
        inf_scale = np.ldexp(1.0, 44 - (-1040))  # what the kernel computed before the clamp: +inf, and its "integer"
    assert np.isinf(inf_scale) and int((np.array(inf_scale) + magic).view(np.int64) - np.array(magic).view(np.int64)) == 4375247037990436864


@pytest.mark.parametrize("shape", list(bc.SHELL_SHAPES), ids=SHELL_IDS)
def test_fixed_point_restatement_stays_inside_its_bound(shape):
    geo = bc.geometry(shape)
    for name, w8, wmax, _ in bc.scatter_datasets(geo):
        assert wmax >= np.max(np.abs(w8)) > 0 and np.isfinite(wmax)
        ref, mag = bc.shell_reference(geo, w8)
        assert np.all(mag < 1e308)
        abar, partial, e = bc.fixed_point_scatter(geo, w8, wmax)
        bound = bc.fixed_bound(geo, partial, e)
        w = bc.worst(abar, ref, bound)
        assert w[0] <= 1, (name, w)
        plain = np.bincount(geo.pidx8.ravel(), weights=w8.ravel(), minlength=geo.nb)  # sequential fp64 sums
        assert bc.worst(plain, ref, bc.gamma(geo.count8) * mag)[0] <= 1, name
        assert bc.worst(abar, plain.astype(LD), bound + bc.gamma(geo.count8) * mag)[0] <= 1, name
        if name == "ties":
            assert e == 1 and np.all(np.ldexp(w8, 43) % 1 == 0.5)
        if name == "wmax_pow2_is_max":
            assert math.frexp(wmax)[0] == 0.5 and np.max(np.abs(w8)) == wmax
        if name in ("scaled_1e-300", "subnormal_max"):
            assert e == bc.E_MIN and wmax < 2.0 ** -979
        if name == "subnormal_max":
            assert wmax < 2.0 ** -1022 and not abar.any()  # every point is below half a quantum


# ---- deliberate faults --------------------------------------------------------------------------------------------------------
def test_every_deliberate_fault_is_caught():
    lines, exceeded = [], []
    geo = bc.geometry((33, 31, 255))
    sets = {name: (w8, wmax) for name, w8, wmax, _ in bc.scatter_datasets(geo)}
    w8, wmax = sets["normal_wmax_true"]
    ref, mag = bc.shell_reference(geo, w8)
    fbound = bc.float_shell_bound(geo, mag)
    for mut in bc.WALK_FAULTS:
        failures, visits = bc.walk_coverage(geo, mut)
        assert failures or not np.all(visits == 1), mut
        # the sums such a walk would produce (a point counted as often as it is visited), against the floating-point bound
        got = np.bincount(geo.pidx8.ravel(), weights=w8.ravel() * visits, minlength=geo.nb)
        ratio = bc.worst(got, ref, fbound)[0]
        assert ratio > 1, mut
        exceeded.append(ratio)
        lines.append("FAULT %s caught=coverage+bound workgroups_failing=%d ratio=%.3e" % (mut, len(failures), ratio))
    dropped = w8.copy().reshape(-1)
    victim = int(np.argmin(np.abs(dropped)))  # the hardest point to miss: the smallest magnitude of the set
    dropped[victim] = 0.0
    ratio = bc.worst(np.bincount(geo.pidx8.ravel(), weights=dropped, minlength=geo.nb), ref, fbound)[0]
    assert ratio > 1
    exceeded.append(ratio)
    lines.append("FAULT smallest_point_dropped caught=bound ratio=%.3e" % ratio)
    for mut, data in (("ties_away", "ties"), ("e_too_small_at_pow2", "wmax_pow2_is_max"), ("reversed_fold", "normal_wmax_true"),
                      ("truncate", "all_negative"), ("convert_after_fold", "normal_wmax_true"),
                      ("fold_drops_last_split", "normal_wmax_true")):
        w8, wmax = sets[data]
        good, partial, e = bc.fixed_point_scatter(geo, w8, wmax)
        bad = bc.fixed_point_scatter(geo, w8, wmax, mut)[0]
        changed = int(np.count_nonzero(bits(good) != bits(bad)))
        if mut in ("reversed_fold", "convert_after_fold"):
            # NOT visible through the scatter at these sizes, and harmless there: a bin of m <= 165 points (the largest of
            # every listed shape) sums below 165 * 2^44 < 2^53 quanta, so the conversions and the 15 additions of the fold are
            # exact in any order.  The order of nk_fold_copies is pinned by its own test, on data whose sums do round:
            assert changed == 0 and max(bc.geometry(s).count8.max() for s in bc.SHELL_SHAPES) * 2 ** 44 < 2 ** 53
            src, n, copies, stride = bc.fold_data(4097, 16)
            want = bc.fold_copies_host(src, n, copies, stride)
            other = sum((src[c * stride:c * stride + n] for c in reversed(range(copies))), np.zeros(n))
            changed = int(np.count_nonzero(bits(want) != bits(other)))
            assert changed > 0
            lines.append("FAULT %s caught=bits_of_nk_fold_copies (exact, hence invisible, in the scatter up to 128^3) "
                         "entries_changed=%d" % (mut, changed))
            continue
        assert changed > 0, mut
        ratio = bc.worst(bad, bc.shell_reference(geo, w8)[0], bc.fixed_bound(geo, partial, e))[0]
        if ratio > 1:
            exceeded.append(ratio)
        lines.append("FAULT %s caught=bits%s bins_changed=%d ratio=%.3e" % (mut, "+bound" if ratio > 1 else "", changed, ratio))
    assert len(lines) >= 6 and len(set(bc.WALK_FAULTS + bc.ARITH_FAULTS)) == len(lines) - 1
    lines.append("FAULT smallest_factor_over_a_bound=%.3e (of %d faults that exceed one)" % (min(exceeded), len(exceeded)))
    print("\n".join(lines))


def test_other_references_against_plain_numpy():
    """the atomic-scatter, product and mirror references are the operations the existing tests compare with numpy"""
    rng = np.random.default_rng(2)
    geo = bc.geometry((8, 8, 12))
    w8, a0 = rng.normal(size=geo.oshape), rng.normal(size=geo.nb)
    plain = a0 + np.bincount(geo.pidx8.ravel(), weights=w8.ravel(), minlength=geo.nb)
    for merged in (False, True):
        ref, bound = bc.atomic_scatter_reference(geo, geo.pidx, w8, a0, merged, geo.nb)
        assert np.all(bound > 0) and np.max(np.abs(plain - ref.astype(np.float64))) < 1e-13
    pc = bc.ProductCase((6, 10, 8), null_dtab=1)
    fac = [t[p] for t, p in zip(pc.tab, pc.pidx)]
    full = pc.scale * np.einsum("i,j,k->ijk", *fac)
    assert np.allclose(pc.field(0)[0].astype(np.float64).reshape(full.shape), full, rtol=1e-14)
    d0, d2 = pc.dtab[0][pc.pidx[0]], pc.dtab[2][pc.pidx[2]]
    tan = pc.dscale * np.einsum("i,j,k->ijk", *fac) + pc.scale * (np.einsum("i,j,k->ijk", d0, fac[1], fac[2]) +
                                                                 np.einsum("i,j,k->ijk", fac[0], fac[1], d2))
    assert np.allclose(pc.field(1)[0].astype(np.float64).reshape(full.shape), tan, rtol=1e-13, atol=1e-14)
    w = pc.w.reshape(full.shape)
    for which in range(3):
        others = [fac[i] for i in range(3) if i != which]
        want = pc.scale * np.einsum(("ijk,j,k->i", "ijk,i,k->j", "ijk,i,j->k")[which], w, *others)
        assert np.allclose(pc.marginal(which)[0].astype(np.float64), want, rtol=1e-13, atol=1e-13)
    x = rng.normal(size=(5, 4, 9))
    ref, bound = bc.mirror_reference(x, (0, 1, 1), 2, [0.5, 0.25, -1.0, 2.0], 1.0, 0.0, np.float64)
    f0 = np.roll(x[::-1], 1, axis=0)
    f1 = np.roll(np.roll(x[:, ::-1, ::-1], 1, axis=1), 1, axis=2)
    f01 = np.roll(np.roll(f0[:, ::-1, ::-1], 1, axis=1), 1, axis=2)
    assert np.allclose(ref.astype(np.float64), 0.5 * x + 0.25 * f0 - f1 + 2.0 * f01, rtol=1e-14) and np.all(bound >= 0)
    assert len(bc.mirror_groupings(3)) == 1 + 8 + 27
