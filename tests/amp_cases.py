"""Cases, long-double references and DERIVED error bounds for the amplitude kernels of nifty_amd/csrc/nk_amp.hip
(tests/test_amp_cases.py on the host, tests/test_amp_kernels_gpu.py on the device).

The model (header comment of nk_amp.hip, oracle/nifty_oracle.py amplitude_state / amplitude_jvp / amplitude_vjp), m = nb - 2:
    sig0 = flex sqrt(d) sqrt(d^2 / 12 + asp),  sig1 = flex sqrt(d);   x0 = sig0 xs0,  x1 = sig1 xs1
    c = cumsum(x1);  smooth[j + 2] = cumsum((c_j + c_{j-1}) / 2 d_j + x0_j)
    p = slope rel + smooth - smooth[-1] sc;  spec = exp(p);  S = sum mult spec;  ahat = sqrt(spec / S)
    amp[0] = V zm;  amp[b] = V fluct ahat[b]
`forward`, `jvp` and `vjp` evaluate this, its derivative and its transpose in the precision T they are given: np.longdouble is
the reference, np.float64 the plain restatement a device result is put beside.  Their inputs are the float64 arrays the
device gets, cast exactly.  A `mut` names ONE deliberate fault (MUTATIONS) the bounds have to catch.

Bounds.  u = 2^-53; a result whose rounding steps each have relative error <= u, k of them on the longest path from an input
to the output, differs from the exact one by at most about k u sum |terms| (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 3.1); `gamma(k)` is the rigorous k u / (1 - k u).  The "magnitude companions" are those sums of
absolute terms: the same recurrences run on |x0|, |x1| (|y| for the transpose) so that nothing cancels.  The step counts are
read off nk_amp.hip, with AMP_THREADS, EPT and MAXG parsed from its text (a retune moves the bounds with it):

  scan.  One seg_combine is (A, D, B) <- (Al + Ar, Dl + Dr, Bl + Br + Al Dr).  The longest chain of combines between an
  element and a scan output, `scan_depth`:
      EPT                 the thread's own elements (chunk_aggregate)
    + 6 + AMP_WAVES       the wavefront's shuffle steps 1 .. 32 and the walk over the wavefront totals (block_scan_seg)
    + tiles per chunk     carry <- combine(carry, total) over the tiles of the source workgroup
    + 6 + AMP_WAVES + 1   the scan of the <= MAXG = 256 workgroup aggregates (seg_prefix_total) and its wave prefix
    + tiles per chunk     the carry over the tiles of the emitting workgroup
    + 1 + EPT             combine(carry, excl) and the thread's running state (chunk_apply)
  A term B_i of an output passes 2 additions per combine; a term A_i D_k is formed where the groups of i and k meet, from
  sums A and D that took one addition per combine until then, by one product, and passes 2 additions per combine afterwards:
  at most c_scan = 2 scan_depth + 1 steps for every term of smooth (the B component) and scan_depth for a plain sum (the A
  component, the T of the transpose).  Neither depends on nb beyond the tiles per chunk.  A combine with the empty segment
  (0, 0, 0) is exact, and every other combine on the way to an output joins at least one more of the k elements the output
  holds: output number k of the scan order passes at most min(scan_depth, k - 1) of them (`output_depth`), which is what
  the first outputs and the sizes below one tile are held to.
  elements.  exp and sqrt of the device library are within 1 ulp = 2 u.  flex, asp, fluct, zm = exp(lm + ls xi): 2 |arg| u from
  the argument's two steps plus 2 u: E_HYP = 10 u for |arg| <= 4 (a condition on every case).  w0 = sqrt(d^2 / 12 + asp):
  (10 + 3) / 2 + 2 < 9 u.  x0 = flex sqrt(d) w0 xs0: 10 + 2 + 9 + 3 = 24, B = x1 d / 2 + x0 two more: E_FWD = 28 covers every
  element-wise expression of the forward pass and of the transpose's emit.  The JVP's dx0 = dsig0 xs0 + sig0 dxs0 with
  dsig0 = dflex sqrt(d) w0 + flex sqrt(d) (0.5 / w0) dasp, dflex = flex ls dxi (12 u): 10 + 2 + (9 + 1) + 12 + 3 = 39 for the
  second term, then the sum, the product with xs0, the sum with sig0 dxs0 and the two steps of B: E_JVP = 48.
  reductions.  block_sum is 6 shuffle steps and AMP_WAVES additions; amp_store_sums adds ceil(grid / AMP_THREADS) partials per
  thread and runs block_sum again.  Before that a thread adds its own terms in turn: EPT per tile and the two leading bins
  in the scan launches (`c_sum_scan`), ceil(nb / (grid AMP_THREADS)) in the grid-stride launches (`c_sum_grid`).
The bounds of spec, S, ahat, amp, of dS / S and of Q / S follow by propagating these through exp, sqrt and the quotients
(forward_bounds, jvp_bounds, vjp_bounds).
"""
import math
import os
import re
from functools import lru_cache

import numpy as np

from oracle.nifty_oracle import CFParams, lognormal_moments

LD = np.longdouble
U64 = 2.0 ** -53
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nifty_amd", "csrc")
NK_MAX_BATCH = 8  # include/niftyk.h


def _const(name):
    text = open(os.path.join(CSRC, "nk_amp.hip")).read()
    factors = re.search(r"constexpr int %s = ([\d *]+);" % name, text).group(1).split("*")
    return math.prod(int(f) for f in factors)


AMP_THREADS = _const("AMP_THREADS")
EPT = _const("EPT")
MAXG = _const("MAXG")
AMP_WAVES = AMP_THREADS // 64
TILE = AMP_THREADS * EPT
E_FWD, E_JVP = 28, 48  # rounding steps of one element-wise expression (docstring)
E_HYP = 10             # of flex, asp, fluct, zm


def gamma(k):
    return k * U64 / (1.0 - k * U64)


# ---- launch geometry (make_scan_geom, amp_grid of nk_amp.hip) -------------------------------------------------------------
def scan_geom(m):
    """(chunk, ngroups) of the scan over m elements"""
    ng = min(max((m + TILE - 1) // TILE, 1), MAXG)
    chunk = (m + ng - 1) // ng
    chunk = (chunk + TILE - 1) // TILE * TILE
    return chunk, max((m + chunk - 1) // chunk, 1)


def amp_grid(nb):
    return min(max((nb + AMP_THREADS - 1) // AMP_THREADS, 1), MAXG)


def state_used(nb):
    """doubles of the state the kernels may touch: 16 scalars, spec | ahat | tmp | one unused row, then 3 per scan workgroup
    (amp_segs: room for (nb + 1023) / 1024 + 1 of them) and 2 per workgroup of a reducing launch (amp_part)"""
    return 16 + 4 * nb + 3 * min((nb + 1023) // 1024 + 1, MAXG) + 2 * amp_grid(nb)


def scan_depth(nb):
    tiles = scan_geom(nb - 2)[0] // TILE
    return EPT + (6 + AMP_WAVES) + tiles + (6 + AMP_WAVES + 1) + tiles + 1 + EPT


def c_scan(nb):
    return 2 * scan_depth(nb) + 1


def output_depth(nb, reverse=False):
    """per element j of the m: combines that round on the way to the scan's output at j (docstring, "scan")"""
    held = np.arange(nb - 2)  # elements the output holds beside its own
    return np.minimum(scan_depth(nb), held[::-1] if reverse else held)


def c_sum_scan(nb, per_element=1):
    """additions of a sum a scan launch forms beside the scan (S, dS: one term per element; flex_bar: two)"""
    chunk, ng = scan_geom(nb - 2)
    return per_element * (EPT * (chunk // TILE) + 2) + 2 * (6 + AMP_WAVES) + -(-ng // AMP_THREADS)


def c_sum_grid(nb):
    """additions of a sum of the grid-stride launches (k_vjp_red1, k_vjp_red2)"""
    g = amp_grid(nb)
    return -(-nb // (g * AMP_THREADS)) + 2 * (6 + AMP_WAVES) + -(-g // AMP_THREADS)


# ---- geometries, hyper-parameters, latents ----------------------------------------------------------------------------------
def hyp_default():
    p = CFParams()
    return np.array([*lognormal_moments(*p.fluctuations), *lognormal_moments(*p.flexibility), *lognormal_moments(*p.asperity),
                     *lognormal_moments(*p.offset_std), float(p.loglogavgslope[0]), float(p.loglogavgslope[1]), 1.0])


def hyp_other():
    return np.array([*lognormal_moments(0.7, 0.3), *lognormal_moments(2.0, 0.5), *lognormal_moments(0.2, 0.1),
                     *lognormal_moments(0.05, 0.02), -2.2, 0.4, 3.75])


HYPS = {"default": hyp_default, "other": hyp_other}


def k_lengths(nb, family, seed=0):
    if family == "sqrt":  # small and decaying widths, like natural binning
        return np.sqrt(np.arange(nb, dtype=np.float64))
    steps = np.random.default_rng([11, nb, seed]).uniform(0.05, 0.6, nb - 2)  # wide bins: the d^2 / 12 term matters
    return np.concatenate([[0.0], np.exp(np.concatenate([[0.0], np.cumsum(steps)]))])


def make_geo(k, seed=0):
    """geo = rel | sc | mult | delta as FusedModel.__init__ builds it from the bins' k lengths, except that the two unused
    slots of delta hold NaN: a kernel that reads past the first nb - 2 shows"""
    nb = len(k)
    logk = np.log(k[1:])
    rel = np.insert(logk - logk[0], 0, 0.0)
    delta = np.concatenate([logk[1:] - logk[:-1], [np.nan, np.nan]])
    mult = np.random.default_rng([12, nb, seed]).integers(1, 50, nb).astype(np.float64)
    mult[0] = 0.0
    return np.concatenate([rel, rel / rel[-1], mult, delta])


class Problem:
    """the static arrays of one (nb, family, hyp) in float64 and, per precision, cast"""

    def __init__(self, nb, family="sqrt", hyp="default", geo=None, hyp_values=None):
        self.nb, self.m, self.family, self.hyp_name = nb, nb - 2, family, hyp
        self.geo = make_geo(k_lengths(nb, family)) if geo is None else np.asarray(geo, dtype=np.float64)
        self.hyp = HYPS[hyp]() if hyp_values is None else np.asarray(hyp_values, dtype=np.float64)
        self.nsmall = 5 + 2 * self.m
        self.chunk, self.ngroups = scan_geom(self.m)
        self._cast = {}

    def arrays(self, T):
        if T not in self._cast:
            g, nb = self.geo.astype(T), self.nb
            self._cast[T] = (g[:nb], g[nb:2 * nb], g[2 * nb:3 * nb], g[3 * nb:4 * nb - 2], self.hyp.astype(T))
        return self._cast[T]


def latents(pr, seed, extreme=False):
    rng = np.random.default_rng([13, pr.nb, seed])
    lat = rng.normal(size=pr.nsmall)
    if extreme:  # scalars at +-3, spectrum three times as wide
        lat[:5] = 3.0 * np.where(rng.random(5) < 0.5, -1.0, 1.0)
        lat[5:] *= 3.0
    return lat


def unit(n, i, value=1.0):
    v = np.zeros(n)
    v[i] = value
    return v


SPLIT_ROWS_UP_TO = 65537


def spectrum_positions(pr):
    """elements 0 and m - 1, both sides of the first tile boundary and of the first workgroup boundary"""
    pos = {0, pr.m - 1}
    if pr.m > TILE:
        pos |= {TILE - 1, TILE}
    if pr.ngroups > 1:
        pos |= {pr.chunk - 1, pr.chunk}
    return sorted(pos)


def tangents(pr, seed=0):
    """[(name, dlat)]: dense normal, the five scalar units, spectrum units at spectrum_positions: one per row, beyond
    SPLIT_ROWS_UP_TO bins one with both rows of the element set (the long-double side sets the run time there)"""
    out = [("dense", np.random.default_rng([14, pr.nb, seed]).normal(size=pr.nsmall))]
    out += [(f"scalar{i}", unit(pr.nsmall, i)) for i in range(5)]
    for j in spectrum_positions(pr):
        rows = [(f"xs0[{j}]", unit(pr.nsmall, 5 + j)), (f"xs1[{j}]", unit(pr.nsmall, 5 + pr.m + j))]
        out += rows if pr.nb <= SPLIT_ROWS_UP_TO else [(f"xs01[{j}]", rows[0][1] + rows[1][1])]
    return out


def cotangents(pr, seed=0):
    """[(name, abar)]: dense normal, units at bins 0, 1, 2 and nb - 1"""
    out = [("dense", np.random.default_rng([15, pr.nb, seed]).normal(size=pr.nb))]
    return out + [(f"bin{b}", unit(pr.nb, b)) for b in sorted({0, 1, 2, pr.nb - 1})]


# ---- the model in precision T ---------------------------------------------------------------------------------------------
MUTATIONS = ("drop_x0_tile2", "drop_carry_c", "drop_tile_carry_c", "delta_shift", "vjp_last_half", "no_sc_dot", "fl_bar_bin0")


def mutation_defined(mut, pr):
    return {"drop_x0_tile2": pr.m > TILE, "drop_carry_c": pr.ngroups > 1, "drop_tile_carry_c": pr.chunk > TILE, "delta_shift": pr.m > 1,
            "vjp_last_half": pr.m > 1, "no_sc_dot": True, "fl_bar_bin0": True}[mut]


def _cumsum(v):
    return np.cumsum(v, dtype=v.dtype)


def _rcumsum(v):
    return _cumsum(v[::-1])[::-1]


def twolog(pr, x0, x1, d, mut=None):
    """smooth (nb,) from the increments; faults: the x0 of the first element of the second tile dropped, workgroup 1 without
    its carry-in of c, the second tile of workgroup 0 without the c of its first, delta[1] for delta[0] in the B term of element 0"""
    T = x0.dtype.type
    c = _cumsum(x1)
    cprev = np.concatenate([[T(0)], c[:-1]])
    if mut in ("drop_carry_c", "drop_tile_carry_c"):
        lo, hi = (pr.chunk, min(2 * pr.chunk, pr.m)) if mut == "drop_carry_c" else (TILE, 2 * TILE)
        c, cprev = c.copy(), cprev.copy()
        c[lo:hi] -= cprev[lo]
        cprev[lo:hi] -= cprev[lo]
    inc = (c + cprev) / 2 * d + x0
    if mut == "drop_x0_tile2":
        inc[TILE] -= x0[TILE]
    if mut == "delta_shift":
        inc[0] = x1[0] / 2 * d[1] + x0[0]
    return np.concatenate([[T(0), T(0)], _cumsum(inc)])


def twolog_adj(y, d, mut=None):
    """transpose of twolog on y = smooth_bar[2:]: t_j = sum_{i >= j} y_i, g1_j = d_j t_j / 2 + sum_{i > j} d_i t_i; fault: the
    last element of the reversed scan (j = 0) without the delta[1] half of its width"""
    t = _rcumsum(y)
    w = d * t
    g1 = _rcumsum(w) - w / 2
    if mut == "vjp_last_half":
        g1 = g1.copy()
        g1[0] -= d[1] * t[1] / 2
    return t, g1


def hyper(hyp, lat):
    """flex, asp, fluct, zm, slope and the arguments of the four exponentials"""
    args = [hyp[2] + hyp[3] * lat[1], hyp[4] + hyp[5] * lat[0], hyp[0] + hyp[1] * lat[2], hyp[6] + hyp[7] * lat[4]]
    return [np.exp(a) for a in args] + [hyp[8] + hyp[9] * lat[3]], args


def forward(pr, lat, T=LD, mut=None):
    rel, sc, mult, d, hyp = pr.arrays(T)
    lat = np.asarray(lat, dtype=np.float64).astype(T)
    (flex, asp, fluct, zm, slope), args = hyper(hyp, lat)
    xs0, xs1 = lat[5:5 + pr.m], lat[5 + pr.m:]
    sq, w0 = np.sqrt(d), np.sqrt(d * d / 12 + asp)
    sig0, sig1 = flex * sq * w0, flex * sq
    x0, x1 = sig0 * xs0, sig1 * xs1
    smooth = twolog(pr, x0, x1, d, mut)
    p = slope * rel + smooth - smooth[-1] * sc
    spec = np.exp(p)
    S = np.sum(mult * spec)
    ahat = np.sqrt(spec / S)
    amp = hyp[10] * fluct * ahat
    amp[0] = hyp[10] * zm
    return dict(lat=lat, flex=flex, asp=asp, fluct=fluct, zm=zm, slope=slope, args=args, sq=sq, w0=w0, sig0=sig0, sig1=sig1,
                xs0=xs0, xs1=xs1, x0=x0, x1=x1, smooth=smooth, p=p, spec=spec, S=S, ahat=ahat, amp=amp, T=T)


def jvp(pr, st, dlat, mut=None, detail=False):
    T = st["T"]
    rel, sc, mult, d, hyp = pr.arrays(T)
    dlat = np.asarray(dlat, dtype=np.float64).astype(T)
    dflex, dasp = st["flex"] * hyp[3] * dlat[1], st["asp"] * hyp[5] * dlat[0]
    dfluct, dzm = st["fluct"] * hyp[1] * dlat[2], st["zm"] * hyp[7] * dlat[4]
    dslope = hyp[9] * dlat[3]
    dxs0, dxs1 = dlat[5:5 + pr.m], dlat[5 + pr.m:]
    sq, w0 = st["sq"], st["w0"]
    dsig0 = [dflex * sq * w0, st["flex"] * sq * (T(0.5) / w0) * dasp]
    dx0 = [dsig0[0] * st["xs0"], dsig0[1] * st["xs0"], st["sig0"] * dxs0]
    dx1 = [dflex * sq * st["xs1"], st["sig1"] * dxs1]
    dsm = twolog(pr, sum(dx0), sum(dx1), d, mut)
    dp = dslope * rel + dsm - dsm[-1] * sc
    w = mult * st["spec"]
    dS = np.sum(w * dp)
    dah = st["ahat"] * (dp - dS / st["S"]) / 2
    damp = hyp[10] * (dfluct * st["ahat"] + st["fluct"] * dah)
    damp[0] = hyp[10] * dzm
    if not detail:
        return damp
    dsm_abs = twolog(pr, sum(np.abs(v) for v in dx0), sum(np.abs(v) for v in dx1), d)  # magnitude companion
    return dict(damp=damp, dp=dp, dS=dS, dah=dah, dfluct=dfluct, dslope=dslope, dsm_abs=dsm_abs)


def vjp(pr, st, abar, mut=None, detail=False):
    T = st["T"]
    rel, sc, mult, d, hyp = pr.arrays(T)
    abar = np.asarray(abar, dtype=np.float64).astype(T)
    V, ahat = hyp[10], st["ahat"]
    lo = 0 if mut == "fl_bar_bin0" else 1
    fl_bar = V * np.sum(abar[lo:] * ahat[lo:])
    q = ahat * (V * st["fluct"] * abar) / 2
    q[0] = 0
    Q = np.sum(q)
    w = mult * st["spec"]
    pb = q - (Q / st["S"]) * w
    slope_bar, sc_dot = np.sum(pb * rel), np.sum(pb * sc)
    y = pb[2:].copy()
    if mut != "no_sc_dot":
        y[-1] -= sc_dot
    t, g1 = twolog_adj(y, d, mut)
    s0b, s1b = t * st["xs0"], g1 * st["xs1"]
    f_terms = [s0b * st["sq"] * st["w0"], s1b * st["sq"]]
    a_terms = s0b * st["flex"] * st["sq"] * T(0.5) / st["w0"]
    flex_bar, asp_bar = np.sum(f_terms[0] + f_terms[1]), np.sum(a_terms)
    latbar = np.concatenate([[asp_bar * st["asp"] * hyp[5], flex_bar * st["flex"] * hyp[3], fl_bar * st["fluct"] * hyp[1],
                              slope_bar * hyp[9], V * abar[0] * st["zm"] * hyp[7]], t * st["sig0"], g1 * st["sig1"]])
    if not detail:
        return latbar
    return dict(latbar=latbar, abar=abar, q=q, Q=Q, w=w, pb=pb, sc_dot=sc_dot, y=y, t=t, g1=g1, f_terms=f_terms, a_terms=a_terms,
                flex_bar=flex_bar, asp_bar=asp_bar, fl_bar=fl_bar, slope_bar=slope_bar)


# ---- bounds (all from the long-double state; float64 arrays come out) -------------------------------------------------------
def forward_bounds(pr, st):
    """bound of amp per bin and the relative bounds of spec, S and ahat the derivatives need"""
    rel, sc, mult, d, hyp = pr.arrays(LD)
    nb, u = pr.nb, LD(U64)
    sm_abs = twolog(pr, np.abs(st["x0"]), np.abs(st["x1"]), d)  # magnitude companion of smooth
    slope_mag = abs(hyp[8]) + abs(hyp[9] * st["lat"][3])
    p_mag = slope_mag * np.abs(rel) + sm_abs + sm_abs[-1] * sc
    cs = np.concatenate([[0, 0], 2 * output_depth(nb) + 1 + E_FWD])  # smooth[0] = smooth[1] = 0 exactly
    b_p = u * (cs * sm_abs + cs[-1] * sc * sm_abs[-1] + 4 * p_mag)  # 4: slope (2), its product, the two additions
    e_spec = np.expm1(b_p) + 2 * u
    w = mult * st["spec"]
    e_S = np.sum(w * e_spec) / st["S"] + gamma(c_sum_scan(nb) + 1)  # every term is >= 0: relative errors average
    e_ahat = np.sqrt((1 + e_spec) / (1 - e_S)) - 1 + 3 * u  # the quotient and the square root
    b_amp = np.abs(st["amp"]) * (e_ahat + (E_HYP + 2) * u)
    b_amp[0] = abs(st["amp"][0]) * (E_HYP + 2) * u
    return dict(amp=b_amp.astype(np.float64), e_spec=e_spec, e_S=e_S, e_ahat=e_ahat, sm_abs=sm_abs, p_mag=p_mag, b_p=b_p)


def jvp_bounds(pr, st, fb, dj, dlat):
    """bound of damp per bin (dj: jvp(..., detail=True) in long double) and its magnitude companion"""
    rel, sc, mult, d, hyp = pr.arrays(LD)
    nb, u, V = pr.nb, LD(U64), hyp[10]
    da = dj["dsm_abs"]
    dp_mag = abs(dj["dslope"]) * np.abs(rel) + da + da[-1] * sc
    cs = np.concatenate([[0, 0], 2 * output_depth(nb) + 1 + E_JVP])
    b_dp = u * (cs * da + cs[-1] * sc * da[-1] + 4 * dp_mag)
    w, adp = mult * st["spec"], np.abs(dj["dp"])
    b_dS = np.sum(w * (b_dp + adp * (fb["e_spec"] + 2 * u))) + gamma(c_sum_scan(nb)) * np.sum(w * adp)
    r = dj["dS"] / st["S"]
    b_r = (b_dS / st["S"] + abs(r) * (fb["e_S"] + u)) / (1 - fb["e_S"])
    ahat, e_ahat = st["ahat"], fb["e_ahat"]
    b_dah = np.abs(dj["dah"]) * (e_ahat + 4 * u) + ahat / 2 * (b_dp + b_r) * (1 + e_ahat + 4 * u)
    # dfluct = fluct ls dxi: E_HYP + 2, then the product with ahat, the addition and V; fluct dah: E_HYP + 3
    b = V * (abs(dj["dfluct"]) * ahat * (e_ahat + (E_HYP + 5) * u) + st["fluct"] * (b_dah * (1 + (E_HYP + 3) * u)
                                                                                 + np.abs(dj["dah"]) * (E_HYP + 3) * u))
    b[0] = abs(dj["damp"][0]) * (E_HYP + 4) * u
    mag = V * (abs(dj["dfluct"]) * ahat + st["fluct"] * ahat / 2 * (dp_mag + np.sum(w * dp_mag) / st["S"]))
    mag[0] = abs(dj["damp"][0])
    return b.astype(np.float64), mag


def vjp_bounds(pr, st, fb, dv):
    """bound of latbar per latent (dv: vjp(..., detail=True) in long double)"""
    rel, sc, mult, d, hyp = pr.arrays(LD)
    nb, u, V = pr.nb, LD(U64), hyp[10]
    ahat, e_ahat, e_spec, e_S = st["ahat"], fb["e_ahat"], fb["e_spec"], fb["e_S"]
    nred, depth = c_sum_grid(nb), output_depth(nb, reverse=True)
    a_fl = np.abs(dv["abar"][1:]) * ahat[1:]
    b_fl = V * (np.sum(a_fl * e_ahat[1:]) + gamma(nred + 2) * np.sum(a_fl))
    aq = np.abs(dv["q"])
    e_q = e_ahat + (E_HYP + 3) * u
    b_Q = np.sum(aq * e_q) + gamma(nred) * np.sum(aq)
    r = dv["Q"] / st["S"]
    b_r = (b_Q / st["S"] + abs(r) * (e_S + u)) / (1 - e_S)
    w, apb = dv["w"], np.abs(dv["pb"])
    b_pb = (aq * e_q + b_r * w + abs(r) * w * (e_spec + 2 * u) + u * apb) * (1 + e_spec.max() + 4 * u)
    b_sl = np.sum(b_pb * np.abs(rel)) + gamma(nred + 1) * np.sum(apb * np.abs(rel))
    b_scd = np.sum(b_pb * sc) + gamma(nred + 1) * np.sum(apb * sc)
    b_y, y_abs = b_pb[2:].copy(), apb[2:].copy()
    b_y[-1] += b_scd + u * abs(dv["y"][-1])
    y_abs[-1] += abs(dv["sc_dot"])
    t_abs, g1_abs = twolog_adj(y_abs, d)   # magnitude companions of t and g1
    t_by, g1_by = twolog_adj(b_y, d)       # what the errors of y become
    b_t = gamma(depth) * t_abs + t_by
    b_g1 = gamma(2 * depth + 1 + 3) * g1_abs + g1_by  # + 3: (d_j + d_{j+1}) / 2 and y d_j / 2 of vjp_elem
    e_el = E_FWD * u
    b_s0 = st["sig0"] * b_t * (1 + e_el) + np.abs(dv["t"] * st["sig0"]) * e_el
    b_s1 = st["sig1"] * b_g1 * (1 + e_el) + np.abs(dv["g1"] * st["sig1"]) * e_el
    axs0, axs1, sq, w0 = np.abs(st["xs0"]), np.abs(st["xs1"]), st["sq"], st["w0"]
    f_abs = np.sum(np.abs(dv["f_terms"][0]) + np.abs(dv["f_terms"][1]))
    b_flex = (np.sum(b_t * axs0 * sq * w0 + b_g1 * axs1 * sq) * (1 + e_el) + (gamma(c_sum_scan(nb, 2)) + e_el) * f_abs)
    b_asp = (np.sum(b_t * axs0 * st["flex"] * sq / (2 * w0)) * (1 + e_el) + (gamma(c_sum_scan(nb)) + e_el) * np.sum(np.abs(dv["a_terms"])))
    tail = (E_HYP + 3) * u
    lb = dv["latbar"]
    head = [st["asp"] * abs(hyp[5]) * b_asp * (1 + tail) + abs(lb[0]) * tail,
            st["flex"] * abs(hyp[3]) * b_flex * (1 + tail) + abs(lb[1]) * tail,
            st["fluct"] * abs(hyp[1]) * b_fl * (1 + tail) + abs(lb[2]) * tail,
            abs(hyp[9]) * b_sl * (1 + u) + abs(lb[3]) * u,
            abs(lb[4]) * (E_HYP + 4) * u]
    return np.concatenate([np.array(head, dtype=LD), b_s0, b_s1]).astype(np.float64)


# ---- cases ------------------------------------------------------------------------------------------------------------------
# sizes that mark a branch of the launch geometry: nb -> (chunk, ngroups, amp_grid); asserted by tests/test_amp_cases.py
GEOMETRY = {
    3: (1024, 1, 1), 4: (1024, 1, 1), 5: (1024, 1, 1), 6: (1024, 1, 1), 7: (1024, 1, 1),  # m = 1 .. EPT + 1
    256: (1024, 1, 1), 257: (1024, 1, 2),           # amp_grid 1 -> 2
    258: (1024, 1, 2), 259: (1024, 1, 2),           # m = 256, 257: the scan reaches the second wavefront (64 EPT elements)
    1026: (1024, 1, 5), 1027: (1024, 2, 5),         # one full tile; a second workgroup holding one element
    2050: (1024, 2, 9), 2051: (1024, 3, 9),
    65536: (1024, 64, 256), 65537: (1024, 64, 256),  # amp_grid at its cap, the grid-stride loops start
    262146: (1024, 256, 256),                       # 256 workgroups of one tile
    262147: (2048, 129, 256),                       # chunks of two tiles, a partial last workgroup
    300003: (2048, 147, 256),                       # the size the comment of seg_prefix_total names
    524291: (3072, 171, 256),                       # chunks of three tiles
}
LOG_SIZES = (3, 4, 5, 6, 7, 67, 259)   # the wide-bin family, small nb only
EXTREME_SIZES = (7, 259, 2051, 65537, 262147)   # one per size class: scalars at +-3, spectrum x 3
OTHER_HYP_SIZES = (6, 1027, 262147)


def case_table():
    """[(id, nb, family, hyp, extreme)]"""
    out = [(f"{nb}-sqrt", nb, "sqrt", "default", False) for nb in GEOMETRY]
    out += [(f"{nb}-log", nb, "log", "default", False) for nb in LOG_SIZES]
    out += [(f"{nb}-sqrt-extreme", nb, "sqrt", "default", True) for nb in EXTREME_SIZES]
    out += [(f"{nb}-sqrt-otherhyp", nb, "sqrt", "other", False) for nb in OTHER_HYP_SIZES]
    return out


CASES = {c[0]: c for c in case_table()}


class Case:
    """everything a test needs about one case: the problem, the point, the long-double state and its bounds"""

    def __init__(self, cid, seed=0):
        _, nb, family, hyp, extreme = CASES[cid]
        self.id, self.pr = cid, Problem(nb, family, hyp)
        self.lat = latents(self.pr, seed, extreme)
        self.st = forward(self.pr, self.lat)
        self.fb = forward_bounds(self.pr, self.st)
        self.tangents, self.cotangents = tangents(self.pr), cotangents(self.pr)
        self._refs = None

    def well_conditioned(self):
        """finite everywhere, |p| < 600 (exp far from over- and underflow), |arguments of the hyper exponentials| <= 4"""
        st = self.st
        return bool(np.all(np.isfinite(st["amp"])) and np.all(np.isfinite(st["p"])) and np.max(np.abs(st["p"])) < 600
                    and max(abs(a) for a in st["args"]) <= 4 and st["S"] > 0)

    def jvp(self, dlat):
        """(damp, bound, magnitude) in long double / float64"""
        dj = jvp(self.pr, self.st, dlat, detail=True)
        b, mag = jvp_bounds(self.pr, self.st, self.fb, dj, dlat)
        return dj["damp"], b, mag

    def vjp(self, abar):
        """(latbar, bound)"""
        dv = vjp(self.pr, self.st, abar, detail=True)
        return dv["latbar"], vjp_bounds(self.pr, self.st, self.fb, dv)

    def references(self):
        """([(name, dlat, damp, bound)], [(name, abar, latbar, bound)]) of self.tangents and self.cotangents, computed once
        (on a few threads: numpy's long-double loops release the interpreter lock) and to be left unchanged"""
        if self._refs is None:
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(8) as ex:
                fj = [ex.submit(self.jvp, d) for _, d in self.tangents]
                fv = [ex.submit(self.vjp, a) for _, a in self.cotangents]
                self._refs = ([(n, d) + f.result()[:2] for (n, d), f in zip(self.tangents, fj)],
                              [(n, a) + f.result() for (n, a), f in zip(self.cotangents, fv)])
        return self._refs


@lru_cache(maxsize=2)
def get_case(cid):
    return Case(cid)


def worst(got, exact, bound):
    """(ratio, err, bound, |exact|) at the element with the largest |got - exact| / bound; a zero bound needs a zero error"""
    got = np.asarray(got)
    err = np.abs(got.astype(LD) - exact).astype(np.float64)
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    return float(ratio[i]), float(err[i]), float(bound[i]), float(abs(exact[i]))
