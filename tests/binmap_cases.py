"""Geometry, exact restatements, long-double references and DERIVED bounds for the bin-map kernels: nk_octant_expand(_k2),
nk_octant_scatter(_k2), nk_fold_copies, nk_segment_sum, nk_pindex_from_k2, nk_scatter_add of nifty_amd/csrc/nk_vec.hip and the
product-spectrum kernels of nk_prod.hip (tests/test_binmap_cases.py on the host, tests/test_binmap_kernels_gpu.py on the device).
numpy and Python integers only.

Geometry.  A grid of 1..3 axes is seen right-aligned as [A][M][NL]; the octant holds the points a <= A/2, b <= M/2, c <= NL/2
(extents Ah, Mh, Ch = n/2 + 1, odd lengths included).  The bins are the distinct integer k^2 = a^2 + b^2 + c^2 of the folded
coordinates in ascending order (`bin_k2`), `pidx` the bin of every grid point, `pidx8` of every octant point: PowerSpace's
natural binning wherever the harmonic distances are equal.

Shell walk (k_octant_scatter_k2 and its fixed-point twin).  Workgroup (shell j, split s) owns the bins [j NK_SHELL_BINS,
(j + 1) NK_SHELL_BINS) = the k^2 range [klo, khi) and the first-axis lines a = s (mod NK_SHELL_SPLITS).  `shell_walk` lists
the (a, b, c) it visits from klo, khi, hc2 = (Ch - 1)^2, b_lo = ceil sqrt(klo - hc2 - ra), b_hi = ceil sqrt(khi - ra) and
the two ceiling roots per line, in the kernel's own trip structure (16 groups x NK_SHELL_NU lines, the first 16 points of a
run, then the tail loop) with EXACT integer square roots.

Fixed point (`fixed_point_scatter`), the contract of include/niftyk.h.  e = max(frexp exponent of w8max, E_MIN = -979),
q = 2^(e - 44).  Every point adds rne(v / q) (ties to even) as an integer to the sum of its (bin, split = a mod 16); every
such sum becomes a double once (round to nearest) and is multiplied by q (exact); the 16 splits are added in split order
starting from 0.0.  No step depends on the order of the atomics, so the device result is these bits.  v / q = v 2^(44 - e)
is exact in fp64 unless it is subnormal, and then it rounds to the integer 0 with or without the intermediate rounding:
`fixed_rn` (vectorised, fp64 scaling + rint) equals `fixed_rn_exact` (Python integers) -- the host test holds one to the other.
On every grid used here a bin holds at most 165 octant points, so its sums stay below 165 * 2^44 < 2^53 quanta: the
conversions and the fold happen to be exact and their order shows only in nk_fold_copies' own test (data whose sums round).

Bounds.  u = 2^-53, gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1),
m_b = points (or atomic terms) of bin b, all in long double so that a bound of subnormal data does not underflow to zero:
  floating-point shell scatter   gamma(m_b - 1 + 15) sum |w_i|: any order of the m_b - 1 LDS additions inside the workgroups,
                                 then at most 15 rounding additions of the fold (0.0 + x is exact)
  fixed point against the sum    m_b q / 2 (one rounding to the quantum per point) + 16 u sum |partial| (one conversion per
                                 split) + gamma(15) sum |partial| (the fold), partial = the 16 split doubles of the bin
  global atomics (nk_octant_scatter, nk_scatter_add)
                                 gamma(m_b) (|abar0| + sum |terms|): m_b additions in any order onto abar0; a merged pair
                                 l0 + l1 is one term with one rounding of its own, u |term| (1 + gamma(m_b))
  product marginal               gamma(A C + chunks + 5) sum |w others s| per output.  A term passes at most 1 rounding in the
                                 product of the tables behind `which`, 1 in w * that, ceil(C / 64) - 1 additions of its lane
                                 and up to 6 of the shuffle tree, 2 in the factors in front, 1 in the scale, at most
                                 min(A, MARG_ROWS) - 1 additions of its chunk and chunks - 1 of the fold (factors of 1.0 and
                                 additions onto 0.0 are exact): `marginal_steps` counts them per case and the host test
                                 asserts the count is at most A C + chunks + 5; a multiply-add contracted into one
                                 instruction only removes a rounding
  product field / tangent        gamma(6) sum |terms| (ds t0 t1 t2 + s (dt0 t1 t2 + ...): two products, two sums, the factor
                                 s and the last sum on the longest path) + 2^-24 |ref| for a float32 store
  mirror combine                 gamma(2^nsub + 2) (|scale| sum |coef in| + |offset|) + the store rounding
"""
import math
import os
import re

import numpy as np

LD = np.longdouble
U64 = LD(2.0) ** -53
U32 = LD(2.0) ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nifty_amd", "csrc")
VEC_SRC = open(os.path.join(CSRC, "nk_vec.hip")).read()
PROD_SRC = open(os.path.join(CSRC, "nk_prod.hip")).read()


def _define(name):
    return int(re.search(r"^#define %s (\d+)$" % name, VEC_SRC, re.M).group(1))


def _constexpr(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, PROD_SRC).group(1))


NK_SHELL_BINS = _define("NK_SHELL_BINS")
NK_SHELL_SPLITS = _define("NK_SHELL_SPLITS")
NK_SHELL_NU = _define("NK_SHELL_NU")
NG = int(re.search(r"constexpr int NG = (\d+), NU = NK_SHELL_NU;", VEC_SRC).group(1))  # lanes of a group = lines per step
MARG_ROWS = _constexpr("MARG_ROWS")
PROD_THREADS = _constexpr("PROD_THREADS")
E_MIN = -979            # 2^(44 - e) <= 2^1023 stays finite (k_octant_scatter_k2_fx, include/niftyk.h)
K2_LIMIT = 1 << 24      # nk_octant_scatter_k2 / nk_octant_expand_k2 refuse (Ah-1)^2 + (Mh-1)^2 + (Ch-1)^2 >= 2^24
INT_MAX = 0x7FFFFFFF

# the shapes of the shell scatter tests: (bins, shells) as the issue's table states them, recomputed by the host test
SHELL_SHAPES = {
    (64, 64, 64): (1914, 1),
    (16, 16, 256): (4720, 2),      # Ah = 9 < NK_SHELL_SPLITS: 7 of 16 workgroups per shell own no line
    (33, 31, 255): (10010, 3),     # all lengths odd
    (32, 32, 256): (10153, 3),
    (128, 128, 128): (8041, 2),
    (8191,): (4096, 1),            # exactly one full shell
    (129, 255): (4419, 2),         # two-dimensional with a second shell: Ah = 1, split 0 owns every line
}
SCATTER_SHAPES = [(1,), (7,), (600,), (5, 6), (3, 700), (4, 6, 10), (5, 7, 9), (8, 8, 12), (64, 64, 64)]
EXPAND_K2_SHAPES = [(16, 16, 256), (33, 31, 255), (255,)]
PINDEX_SHAPES = [(9,), (6, 7), (5, 8, 6)]


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * U64 / (1 - k * U64)


# ---- geometry -------------------------------------------------------------------------------------------------------------
class Geometry:
    def __init__(self, shape):
        self.shape = tuple(int(n) for n in shape)
        self.ndim = len(self.shape)
        assert 1 <= self.ndim <= 3 and min(self.shape) >= 1
        self.A, self.M, self.NL = (1,) * (3 - self.ndim) + self.shape
        self.Ah, self.Mh, self.Ch = self.A // 2 + 1, self.M // 2 + 1, self.NL // 2 + 1
        self.oshape = tuple(n // 2 + 1 for n in self.shape)
        self.osl = tuple(slice(0, n) for n in self.oshape)
        k2 = None
        for n in self.shape:
            ax = np.arange(n, dtype=np.int64)
            ax = np.minimum(ax, n - ax) ** 2
            k2 = ax if k2 is None else np.add.outer(k2, ax)
        self.k2 = k2                                     # integer k^2 of every grid point
        self.bin_k2 = np.unique(k2).astype(np.int32)     # ascending distinct k^2
        self.nb = len(self.bin_k2)
        flags = np.zeros(int(self.bin_k2[-1]) + 1, dtype=bool)
        flags[self.bin_k2] = True
        self.k2table = (np.cumsum(flags) - 1).astype(np.int32)  # PowerSpace._compute: the table nk_pindex_from_k2 reads
        self.pidx = np.ascontiguousarray(self.k2table[k2], dtype=np.int32)
        self.pidx8 = np.ascontiguousarray(self.pidx[self.osl])
        self.n8 = self.pidx8.size
        self.count8 = np.bincount(self.pidx8.ravel(), minlength=self.nb)     # m_b of the octant
        self.rho = np.bincount(self.pidx.ravel(), minlength=self.nb)
        self.shells = -(-self.nb // NK_SHELL_BINS)
        a = np.arange(self.Ah).reshape(-1, 1, 1)
        self.a8 = np.broadcast_to(a, (self.Ah, self.Mh, self.Ch)).reshape(-1)  # first (right-aligned) coordinate per octant point
        self.split8 = self.a8 % NK_SHELL_SPLITS
        self.k2_supported = (self.Ah - 1) ** 2 + (self.Mh - 1) ** 2 + (self.Ch - 1) ** 2 < K2_LIMIT

    def line_order(self):
        """octant lines a * Mh + b sorted by a^2 + b^2 (the optional argument of nk_octant_expand_k2)"""
        a, b = np.divmod(np.arange(self.Ah * self.Mh), self.Mh)
        return np.argsort(a * a + b * b, kind="stable").astype(np.int32)

    def scratch_doubles(self):
        return 64 * (self.nb + 32)  # include/niftyk.h


_GEO = {}


def geometry(shape):
    shape = tuple(shape)
    if shape not in _GEO:
        _GEO[shape] = Geometry(shape)
    return _GEO[shape]


# ---- the shell walk restated ----------------------------------------------------------------------------------------------
def isqrt_ceil(x):
    """smallest n >= 0 with n n >= x (nk_isqrt_ceil), exactly"""
    return 0 if x <= 0 else math.isqrt(x - 1) + 1


def isqrt_floor(x):
    return 0 if x <= 0 else math.isqrt(x)


WALK_FAULTS = ("floor_root_lower_c", "no_tail_loop", "b_lo_without_hc2", "split_mod_8")


def shell_walk(geo, j, s, mut=None):
    """the flat octant indices (a Mh + b) Ch + c workgroup (shell j, split s) adds, in the order of its trips"""
    bin0 = j * NK_SHELL_BINS
    klo = int(geo.bin_k2[bin0])
    last = bin0 + NK_SHELL_BINS >= geo.nb
    khi = INT_MAX if last else int(geo.bin_k2[bin0 + NK_SHELL_BINS])
    hc2 = (geo.Ch - 1) ** 2
    lower_c = isqrt_floor if mut == "floor_root_lower_c" else isqrt_ceil
    out = []
    for a in range(s, geo.Ah, 8 if mut == "split_mod_8" else NK_SHELL_SPLITS):
        ra = a * a
        if ra >= khi:
            break
        b_hi = geo.Mh if last else min(geo.Mh, isqrt_ceil(khi - ra))            # b^2 < khi - ra
        b_lo = isqrt_ceil(klo - (0 if mut == "b_lo_without_hc2" else hc2) - ra)  # b^2 + hc2 >= klo - ra
        for grp in range(NG):
            for b0 in range(b_lo + grp, b_hi, NG * NK_SHELL_NU):
                for u in range(NK_SHELL_NU):
                    b = b0 + u * NG
                    if b >= b_hi:  # `on` is false: ce = 0
                        continue
                    r2 = ra + b * b
                    cl = lower_c(klo - r2)
                    ce = geo.Ch if last else min(geo.Ch, isqrt_ceil(khi - r2))
                    line = (a * geo.Mh + b) * geo.Ch
                    for l16 in range(NG):
                        c = cl + l16
                        if c < ce:
                            out.append(line + c)          # the first 16 points of the run
                        if mut != "no_tail_loop":
                            out.extend(range(line + c + 16, line + ce, 16))  # "rare: runs longer than 16 points"
    return np.asarray(out, dtype=np.int64)


def walk_coverage(geo, mut=None):
    """(failures, visits): the workgroups (j, s) whose walk is not exactly {points with pidx8 in shell j and a mod 16 == s},
    each once; and how often every octant point is visited by all workgroups together"""
    shell8 = geo.pidx8.ravel() // NK_SHELL_BINS
    visits = np.zeros(geo.n8, dtype=np.int64)
    failures = []
    for j in range(geo.shells):
        for s in range(NK_SHELL_SPLITS):
            pts = shell_walk(geo, j, s, mut)
            if len(pts) and (pts.min() < 0 or pts.max() >= geo.n8):
                failures.append((j, s, "outside the octant"))
                continue
            mine = np.bincount(pts, minlength=geo.n8)
            visits += mine
            if not np.array_equal(mine, ((shell8 == j) & (geo.split8 == s)).astype(np.int64)):
                failures.append((j, s, "set"))
    return failures, visits


def walk_counts(geo):
    """points per workgroup [shell][split] and the longest run of one line inside one shell"""
    shell8 = geo.pidx8.ravel() // NK_SHELL_BINS
    per = np.zeros((geo.shells, NK_SHELL_SPLITS), dtype=np.int64)
    np.add.at(per, (shell8, geo.split8), 1)
    sh = shell8.reshape(-1, geo.Ch)
    longest = max(int(np.bincount(row, minlength=geo.shells).max()) for row in sh)  # a shell's cut with a line is one run
    return per, longest


# ---- fixed point restated -------------------------------------------------------------------------------------------------
ARITH_FAULTS = ("ties_away", "e_too_small_at_pow2", "reversed_fold", "truncate", "fold_drops_last_split", "convert_after_fold")


def fixed_exponent(w8max, mut=None):
    e = 0
    if np.isfinite(w8max) and w8max > 0:
        m, e = math.frexp(float(w8max))
        if mut == "e_too_small_at_pow2" and m == 0.5:
            e -= 1
    return max(e, E_MIN)


def fixed_rn_exact(v, shift):
    """rne(v 2^shift) for one double, in Python integers"""
    m, ex = math.frexp(float(v))
    mant = int(m * 2 ** 53)  # exact: |m| < 1 has 53 bits
    k = ex - 53 + shift
    if k >= 0:
        return mant << k
    quo, rem = divmod(mant, 1 << -k)  # floor division: 0 <= rem
    half = 1 << (-k - 1)
    return quo + (1 if rem > half or (rem == half and quo & 1) else 0)


def fixed_rn(v, shift, mut=None):
    x = np.ldexp(np.asarray(v, dtype=np.float64), shift)
    assert np.all(np.abs(x) < 2.0 ** 51)
    if mut == "truncate":
        r = np.trunc(x)
    elif mut == "ties_away":
        r = np.where(np.abs(x - np.trunc(x)) == 0.5, x + np.copysign(0.5, x), np.rint(x))
    else:
        r = np.rint(x)  # ties to even
    return r.astype(np.int64)


def fixed_point_scatter(geo, w8, w8max, mut=None):
    """(abar, partial[16][nb], e): the bits nk_octant_scatter_k2 with a w8max has to return"""
    S = NK_SHELL_SPLITS
    if not (np.isfinite(w8max) and w8max >= 0):
        return np.full(geo.nb, np.nan), np.full((S, geo.nb), np.nan), 0
    e = fixed_exponent(w8max, mut)
    ints = fixed_rn(np.asarray(w8).reshape(-1), 44 - e, mut)
    acc = np.zeros((S, geo.nb), dtype=np.int64)
    np.add.at(acc, (geo.split8, geo.pidx8.ravel()), ints)
    assert np.bincount(geo.pidx8.ravel() // NK_SHELL_BINS * S + geo.split8).max() < 1 << 18  # the kernel's overflow guard
    if mut == "convert_after_fold":
        return np.ldexp(acc.sum(axis=0).astype(np.float64), e - 44), None, e
    partial = np.ldexp(acc.astype(np.float64), e - 44)  # int -> double rounds to nearest; the power of two is exact
    rows = range(S - 1) if mut == "fold_drops_last_split" else (reversed(range(S)) if mut == "reversed_fold" else range(S))
    abar = np.zeros(geo.nb)
    for s in rows:
        abar = abar + partial[s]  # k_fold_copies: s = 0.0; s += src[c]
    return abar, partial, e


def fold_copies_host(src, n, copies, stride):
    out = np.zeros(n)
    for c in range(copies):
        out = out + src[c * stride:c * stride + n]
    return out


def fold_data(n, copies):
    """(src, n, copies, stride): stride > n; whatever lies between the copies is NaN and must not be read"""
    stride = n + 5
    rng = np.random.default_rng([23, n, copies])
    src = np.full(copies * stride, np.nan)
    for c in range(copies):
        src[c * stride:c * stride + n] = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)
    return src, n, copies, stride


def segment_data():
    """(rowptr, perm, src): an empty first segment, an empty one in the middle, one of 5000 entries, an empty last one"""
    rng = np.random.default_rng(29)
    lengths = [0, 3, 1, 0, 5000, 17, 64, 0] + [int(k) for k in rng.integers(0, 9, size=300)] + [0]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    nsrc = int(rowptr[-1]) + 11
    perm = rng.integers(0, nsrc, size=int(rowptr[-1])).astype(np.int32)  # with repeats: a gather, not a permutation
    return rowptr, perm, rng.normal(size=nsrc) * 10.0 ** rng.uniform(-3, 3, size=nsrc)


def segment_sum_host(rowptr, perm, src, dst0, accumulate):
    out = np.empty(len(rowptr) - 1)
    for s in range(len(out)):
        v = 0.0
        for i in perm[rowptr[s]:rowptr[s + 1]]:
            v = v + float(src[i])
        out[s] = (float(dst0[s]) + v) if accumulate else v
    return out


# ---- long-double references and bounds ------------------------------------------------------------------------------------------
def bin_sums(index, values, nb):
    out = np.zeros(nb, dtype=LD)
    np.add.at(out, np.asarray(index).reshape(-1), np.asarray(values, dtype=LD).reshape(-1))
    return out


def shell_reference(geo, w8):
    """(sum, sum of magnitudes) per bin of the octant array, long double"""
    w = np.asarray(w8, dtype=LD).reshape(-1)
    return bin_sums(geo.pidx8, w, geo.nb), bin_sums(geo.pidx8, np.abs(w), geo.nb)


def float_shell_bound(geo, mag):
    return gamma(geo.count8 - 1 + 15) * mag


def fixed_bound(geo, partial, e):
    q = LD(2.0) ** (e - 44)
    pabs = np.abs(partial.astype(LD)).sum(axis=0)
    return geo.count8 * q / 2 + 16 * U64 * pabs + gamma(15) * pabs


def atomic_scatter_reference(geo, pidx, w8, abar0, merged, nb):
    """nk_octant_scatter: (ref, bound).  merged: the launcher honours merge_swapped_lines (3-D, A == M)"""
    w = np.asarray(w8, dtype=LD).reshape(geo.Ah, geo.Mh, geo.Ch)
    p8 = np.asarray(pidx).reshape(geo.A, geo.M, geo.NL)[:geo.Ah, :geo.Mh, :geo.Ch]
    if merged:
        a, b = np.arange(geo.Ah)[:, None, None], np.arange(geo.Mh)[None, :, None]
        pair = np.broadcast_to(a < b, w.shape)
        keep = np.broadcast_to(a <= b, w.shape)
        terms = np.where(pair, w + w.transpose(1, 0, 2), w)
        terms, bins, pair = terms[keep], p8[keep], pair[keep]
    else:
        terms, bins, pair = w.reshape(-1), p8.reshape(-1), np.zeros(w.size, dtype=bool)
    m = np.bincount(bins, minlength=nb)
    a0 = np.asarray(abar0, dtype=LD)
    ref = a0 + bin_sums(bins, terms, nb)
    g = gamma(m)
    bound = g * (np.abs(a0) + bin_sums(bins, np.abs(terms), nb)) + U64 * (1 + g) * bin_sums(bins[pair], np.abs(terms[pair]), nb)
    return ref, bound


def scatter_add_reference(pidx, values, nb):
    v = np.asarray(values, dtype=LD)
    return bin_sums(pidx, v, nb), gamma(np.bincount(pidx, minlength=nb)) * bin_sums(pidx, np.abs(v), nb)


def worst(got, exact, bound):
    """(ratio, err, bound, index) at the largest err / bound; a NaN or an infinity in `got` is an infinite ratio"""
    got = np.asarray(got).reshape(-1)
    exact, bound = np.asarray(exact, dtype=LD).reshape(-1), np.asarray(bound, dtype=LD).reshape(-1)
    bad = ~np.isfinite(got)
    if bad.any():
        i = int(np.argmax(bad))
        return math.inf, LD(np.inf), bound[i], i
    err = np.abs(got.astype(LD) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, LD(0), LD(np.inf)))
    i = int(np.argmax(ratio))
    return float(ratio[i]), err[i], bound[i], i


def record(kernel, shape, dtype, variant, w):
    """`ERR kernel shape dtype variant err bound ratio`"""
    line = "ERR %s %s %s %s err=%.3e bound=%.3e ratio=%.3e" % (kernel, "x".join(str(n) for n in shape), dtype, variant,
                                                            w[1], w[2], w[0])
    print(line)
    return line


# ---- data sets of the shell scatter -------------------------------------------------------------------------------------------
def scatter_datasets(geo):
    """[(name, w8, w8max, fixed_only)]: w8max is what the fixed-point variant is given (always >= max |w8|); fixed_only marks the
    sets that differ from an earlier one in w8max alone"""
    rng = np.random.default_rng([17, *geo.shape])
    n = geo.n8

    def top(w):
        return float(np.max(np.abs(w)))

    normal = rng.normal(size=n)
    out = [("normal_wmax_true", normal, top(normal), False)]
    lu = 10.0 ** rng.uniform(-12.0, 0.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    out.append(("loguniform_12_decades", lu, top(lu), False))
    neg = -np.abs(rng.normal(size=n)) - 2.0 ** -30
    out.append(("all_negative", neg, top(neg), False))
    outlier = rng.normal(size=n)
    outlier[int(rng.integers(n))] = -1.37 * 2.0 ** 30
    out.append(("outlier_2^30", outlier, top(outlier), False))
    # exact ties (k + 1/2) q for w8max = 1.0: frexp gives e = 1, q = 2^-43
    k = rng.integers(-(1 << 42), 1 << 42, size=n)
    k[:4] = [0, -1, 1, -2]  # +-q/2 and +-3q/2: the two neighbours of a tie differ in parity
    ties = (2.0 * k + 1.0) * 2.0 ** -44
    out.append(("ties", ties, 1.0, False))
    out.append(("wmax_next_pow2", normal, 2.0 ** math.ceil(math.log2(top(normal))), True))
    out.append(("wmax_times_2^10", normal, top(normal) * 1024.0, True))
    pow2 = np.clip(rng.normal(size=n), -7.5, 7.5)
    pow2[int(rng.integers(n))] = -8.0
    out.append(("wmax_pow2_is_max", pow2, 8.0, False))
    base = normal / 1024.0  # keeps every bin sum of the 1e307 set inside the fp64 range (asserted by the host test)
    for name, f in (("scaled_1e-200", 1e-200), ("scaled_1e307", 1e307), ("scaled_1e-300", 1e-300)):
        w = base * f
        out.append((name, w, top(w), False))
    sub = np.ldexp(rng.integers(-(1 << 20), 1 << 20, size=n).astype(np.float64), -1074)
    sub[0] = np.ldexp(float(1 << 20), -1074)
    out.append(("subnormal_max", sub, top(sub), False))
    return [(name, np.ascontiguousarray(w.reshape(geo.oshape)), wmax, fo) for name, w, wmax, fo in out]


# ---- product spectra --------------------------------------------------------------------------------------------------------
PRODUCT_SIZES = [(600,), (257,), (128, 255), (257, 256), (128, 1, 64), (5, 255, 63), (129, 257, 65), (3, 600, 200)]


class ProductCase:
    """sizes of the sub-spaces, bin indices, tables, tangents (dtab[null_dtab] is NULL) and the scale (dscale may be NULL)"""

    def __init__(self, sizes, null_dtab=None, null_dscale=False, seed=3):
        rng = np.random.default_rng([seed, *sizes])
        self.sizes, self.nsub = tuple(sizes), len(sizes)
        self.nbs = [max(1, min(s, 3 + s // 7)) for s in sizes]
        self.pidx = [rng.integers(0, nb, size=s).astype(np.int32) for s, nb in zip(sizes, self.nbs)]
        self.tab = [rng.uniform(0.5, 2.0, size=nb) * rng.choice([-1.0, 1.0], size=nb) for nb in self.nbs]
        self.dtab = [None if i == null_dtab else rng.normal(size=nb) for i, nb in enumerate(self.nbs)]
        self.scale = 1.7
        self.dscale = None if null_dscale else -0.3
        self.n = int(np.prod(sizes))
        self.w = rng.normal(size=self.n)

    def _outer(self, parts):
        out = parts[0]
        for p in parts[1:]:
            out = np.multiply.outer(out, p)
        return out.reshape(-1)

    def field(self, tangent):
        """(ref, bound of the fp64 chain), long double, flat"""
        fac = [t.astype(LD)[p] for t, p in zip(self.tab, self.pidx)]
        if not tangent:
            ref = LD(self.scale) * self._outer(fac)
            return ref, gamma(6) * np.abs(ref)
        ds = LD(0.0 if self.dscale is None else self.dscale)
        terms = [ds * self._outer(fac)]
        for i in range(self.nsub):
            if self.dtab[i] is not None:
                dfac = self.dtab[i].astype(LD)[self.pidx[i]]
                terms.append(LD(self.scale) * self._outer([dfac if j == i else fac[j] for j in range(self.nsub)]))
        return sum(terms), gamma(6) * sum(np.abs(t) for t in terms)

    def abc(self, which):
        A = int(np.prod(self.sizes[:which], dtype=np.int64))
        C = int(np.prod(self.sizes[which + 1:], dtype=np.int64))
        return A, self.sizes[which], C

    def marginal_steps(self, which):
        """(roundings on the longest path of a term, the k of the bound's gamma)"""
        A, _, C = self.abc(which)
        chunks = -(-A // MARG_ROWS)
        n_before, n_after = which, self.nsub - which - 1
        row = (max(n_after - 1, 0) + 1 if n_after else 0)                 # the tables behind `which`, w * that (w * 1.0 is exact)
        row += -(-C // 64) - 1 + min(6, (min(C, 64) - 1).bit_length())    # a lane's additions (0.0 + x is exact), the shuffle tree
        front = (max(n_before - 1, 0) + 1 if n_before else 0) + 1         # the tables in front, s * that, * scale
        return row + front + min(A, MARG_ROWS) - 1 + chunks - 1, A * C + chunks + 5

    def marginal(self, which):
        A, Bn, C = self.abc(which)
        fac = [t.astype(LD)[p] for t, p in zip(self.tab, self.pidx)]
        before = self._outer(fac[:which]) if which else np.ones(1, dtype=LD)
        after = self._outer(fac[which + 1:]) if which + 1 < self.nsub else np.ones(1, dtype=LD)
        terms = self.w.astype(LD).reshape(A, Bn, C) * (LD(self.scale) * before)[:, None, None] * after[None, None, :]
        ref, mag = terms.sum(axis=(0, 2)), np.abs(terms).sum(axis=(0, 2))
        return ref, gamma(self.marginal_steps(which)[1]) * mag


def store_rounding(ref, dtype):
    return U32 * np.abs(ref) if np.dtype(dtype) == np.float32 else LD(0.0) * np.abs(ref)


MIRROR_SHAPES = [(7,), (5, 6), (5, 4, 9), (1, 8, 3)]


def mirror_groupings(ndim):
    """every (nsub, group): each axis in any of the nsub sub-spaces"""
    out = []
    for nsub in (1, 2, 3):
        out += [(nsub, g) for g in np.ndindex(*(nsub,) * ndim)]
    return out


def mirror_reference(x, group, nsub, coef, scale, offset, dtype):
    """out[k] = scale sum_s coef[s] in[flip_s(k)] + offset, summed directly in long double; (ref, bound)"""
    xl = np.asarray(x, dtype=LD)
    acc, mag = np.zeros(x.shape, dtype=LD), np.zeros(x.shape, dtype=LD)
    for s in range(1 << nsub):
        ix = np.ix_(*[(-np.arange(n)) % n if (s >> g) & 1 else np.arange(n) for n, g in zip(x.shape, group)])
        acc += LD(coef[s]) * xl[ix]
        mag += np.abs(LD(coef[s]) * xl[ix])
    ref = LD(scale) * acc + LD(offset)
    return ref, gamma((1 << nsub) + 2) * (abs(LD(scale)) * mag + abs(LD(offset))) + store_rounding(ref, dtype)
