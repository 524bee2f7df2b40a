"""Long-double references, derived error bounds and comparators for the Hartley transforms and their fused prologues /
epilogues (tests/test_fused_transforms_gpu.py on the device, tests/test_transform_cases.py for this module itself and for
the host emulation).

REFERENCE.  The T-valued operands are cast to np.longdouble (eps 1.1e-19), the prologue is evaluated in long double, the
transform is scipy.fft.fftn on the long-double array (complex256), Re +- Im gives the two conventions, the epilogue is
evaluated in long double.  The sandwich reference is the same thing applied twice.

BOUNDS.  u = unit roundoff of T (2^-24, 2^-53), gamma_k = k u / (1 - k u).  Nothing below is fitted to a measured error.

* One radix-2 level of a Cooley-Tukey transform (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 24.2):
  a butterfly a +- w b with a stored twiddle |w^ - w| <= mu costs eta = mu + gamma_4 relative to the 2-norm of the level's
  output, and t levels give ||y^ - y||_2 <= t eta / (1 - t eta) ||y||_2.  The radix-4 / 8 / 64 stages of the kernels are
  radix-2 levels with exact (+-1, +-i) or once-rounded ((1 +- i)/sqrt 2) inner constants and ONE general twiddle product
  per level at most, so log2 R levels bound a radix-R stage.
    mu = u            every table (cos / sin evaluated in long double, rounded to double and then to T: (1 + 2^-29) u for
                      fp32, covered by the factor SLACK) and every compile-time constant
    mu = 2 u + sqrt2 gamma_2 (= 4.83 u)
                      MidCfg::TWO, the composed twiddle w^(8 floor(r/8)) w^(r mod 8): two rounded factors (2 u) and one
                      complex product (sqrt2 gamma_2, Higham (3.13))
  eta_table = 5 u, eta_composed = 8.83 u.
* Radix 3 / 5 / 7 of the generic kernels (ButterflyOdd, nk_core.h): a direct R-point DFT, every output an inner product
  of R terms with once-rounded constants c, s: 2 products and R additions per component and one rounding of the constant,
  componentwise gamma_(R+3) sum_r (|x_r||c| + |y_r||s|) <= gamma_(R+3) sum_r |v_r|.  A complex output errs by at most
  sqrt2 gamma_(R+3) sqrt R ||v||_2, the R outputs together by sqrt2 R gamma_(R+3) ||v||_2 = sqrt2 sqrt R gamma_(R+3) ||o||_2
  (||o||_2 = sqrt R ||v||_2).  The stage's twiddle product adds mu + sqrt2 gamma_2:
    eta_R = sqrt(2 R) gamma_(R+3) + mu + sqrt2 gamma_2   = 18.5 u, 29.1 u, 41.2 u  for R = 3, 5, 7.
* One more radix-2 level (eta_table) for the real-pair untangle with the Hartley combination Re +- Im (one table twiddle
  product and additions), and one more for the inter-level twiddle of the two-level first-axis pass.
  The real last axis of n points is a complex transform of n/2 points plus the untangle; counting ceil(log2 n) levels for
  it AND the extra level stays an upper bound.
  => transform_rel_bound(shape) = SLACK * sum of the eta of every stage of every axis (+ the extra levels).
  SLACK = 1.01 covers the second-order terms (1 / (1 - t eta), t eta < 2e-3) and the double rounding of the fp32 tables.
* The transform is linear with ||H||_2 = sqrt N (N = number of grid points): an element-wise prologue error dx reaches
  the output as sqrt N ||dx||_2 at most.  Prologues (nk_core.h, nk_prologue_pair): at most two products and one addition
  in T, and a double table entry rounded to T: |dx| <= gamma_3 (|a in| + |da in2|) = gamma_3 x_abs;  PLAIN: 0.
* Epilogues run in fp64 on the T-valued transform output and round ONCE to T (nk_epilogue): |d out| <= Lip |dt| +
  (u + 8 u64) |out|, Lip = the epilogue's Lipschitz constant in t: 1 (AFFINE), |mul_scalar mul| (MUL), |amp| (VJP), g' and
  the derivatives of dE/ds, g'^2 M (NONLIN, LIKELIHOOD; taken at the reference point, the second-order term is below
  SLACK).  exp / tanh / log of the device library: <= 2 ulp in fp64 (OCML), i.e. 4 u64 relative: inside the 8 u64.
* Reductions (`value` of LIKELIHOOD and of the VJP curvature, the sandwich's included): an fp64 summation tree errs by
  gamma_h(u64) sum |term| with h = the number of additions on the longest path from a term to the result (Higham (4.4)).
  On the device (nk_flush_energy, nk_fold_value_slots):
    a thread adds its own terms one after the other        <= 128  (register-resident final pass: E = 16 coefficients x 2
                                                                   lines x 2 for a couple = 64; 1-D k2_contig: E <= 32
                                                                   coefficients = 64 outputs; generic pass C: <= 19456
                                                                   complex of 152 KiB LDS over 512 threads = 38 -> 76
                                                                   outputs; k_pass1d: <= 9216 complex over 256 threads =
                                                                   36 -> 72 outputs)
    six shuffle steps join the wavefront                      6
    -> one slot per wavefront; k_fold_slots_a: 256 workgroups of 256 threads over n_slots slots, a thread adds
       ceil(ceil(n_slots / 256) / 256) slots in order, six shuffle steps, the four wavefront partials in order   s + 6 + 4
    k_fold_slots_b: 256 partials, six shuffle steps, four partials in order, `*value += s`                       6 + 4 + 1
    the term itself: <= 4 fp64 operations behind the fp64 conversion of the output                               4
  h_device = 128 + 6 + s + 10 + 11 + 4 = 159 + s;  n_slots is not exported: its area is 2 (n_slots + 256) doubles of the
  workspace, so n_slots <= nk_plan_workspace_bytes / 16 (s = 4 for 64^3 fp64, where the N = 262144 of a sequential sum
  would be 1600 times looser).  Without a workspace (1-D calls) a workgroup joins its <= 16 wavefront partials in LDS and
  issues ONE atomic: h = 128 + 6 + 16 + (number of workgroups = atomic contributions) + 4.
  The host emulation adds every term to one running sum: h = the number of terms there (reduction_depth(None)).
  The atomically accumulated abar has no fixed order: h = the number of contributions to the bin.
  Inherited error: sum |weight| |dt| <= ||weight||_2 ||dt||_2 (Cauchy-Schwarz, worst case -- in fp32 this term, not
  gamma_h, sets the bound of `value`).

IMPULSES.  A unit impulse at p gives scale * cas(2 pi sum_d k_d p_d / n_d).  Every stage then multiplies ONE non-zero
value of modulus 1 by a twiddle (additions of zero are exact; a radix-R odd stage multiplies by one constant and one
twiddle: 2 (mu + sqrt2 gamma_2) <= 2 eta_table), the untangle adds two values of modulus <= 1 (its level counted twice), so a
complex coefficient errs by (levels + 2) eta_table and Re +- Im by sqrt2 times that, per ELEMENT.

COMPLEX TRANSFORMS (nk_fftn; tests/test_complex_transforms_gpu.py).  Reference: scipy.fft on complex256 (fft_ld), checked
against a direct mpmath DFT (fft_direct_mp).  k_c2c_contig / k_c2c_strided run the generic stages of nk_core.h
(nk_dif_stage) on every axis at FULL length: no real-pair untangle, no two-level pass.
  => c2c_rel_bound(shape) = SLACK * sum of eta(p) over the prime factors p of every axis + u,
the u for the one product with (T)scale (the tests use scales that T represents exactly).
  Written down, not hidden: a radix-4 / radix-8 stage of nk_dif_stage reads ONE table entry w and forms w^2 .. w^(R-1) by
  repeated products, |w^r^ - w^r| <= r u + (r - 1) sqrt2 gamma_2.  Over the R outputs of a butterfly that is 5.0 u (R = 4)
  and 13.7 u (R = 8) in the root mean square against the mu = u of a table entry, so the worst case of a radix-8 stage on
  paper is about 20 u where its three levels are counted with 15 u (radix 4: 9.8 u against 10 u).  The bound is kept as
  the table-twiddle rule gives it -- the tighter figure -- and is not widened for this.
* c2c_impulse_elem_bound: a unit impulse passes ONE non-zero value of modulus 1 through every stage (additions of zero
  are exact): one twiddle product per level (an odd stage: a constant and a twiddle, 2 eta_table), no untangle, and the
  complex coefficient itself is compared (no Re +- Im, no sqrt2): (levels + 2 #odd) eta_table + u per ELEMENT.

CHIRP-Z (nk_bluestein_rows, one launch; backend._fft_last_axis_any, three native transforms).  n points, padded to m = 2^L.
With w_j = exp(-+ i pi j^2 / n) and the cyclic filter b_j = conj(w)_|j|:  X_k = w_k (a * b)_k,  a = x . w zero-padded.
Tables (backend._bluestein_tables / _chirp): angles from j^2 mod 2n in integers, evaluated in DOUBLE on the host:
    theta^ = fl(fl(j^2 mod 2n) fl(pi / n)): relative 2.4 u64 (pi, the quotient, the product) of theta <= 2 pi -> 15 u64,
    cos / sin <= 1 ulp each -> sqrt2 u64;            mu_w  = 17 u64 (+ u when rounded to fp32)
    exp(-2 pi i k / m), k / m exact, theta <= pi:    mu_tw = 5 u64  (+ u when rounded to fp32)
  so in fp64 the level of the one-launch kernel costs eta_b = mu_tw + gamma_4 = 9 u, not the 5 u of a long-double table
  (fp32: 5 u as before).  Its radix-4 butterflies read BOTH levels' twiddles from the table (tw[j s1], tw[j s2]); the +-i
  rotations and the conjugation of the inverse levels are exact.
  The filter spectrum bhat the kernel multiplies with is itself a product of a transform (numpy's, in double, for the
  one-launch kernel; nk_fftn in T for the composition).  Its error is a property of the TABLE handed to the kernel, not
  of the kernel: table_err = max_k |bhat^_k - bhat_k| / Bmax, Bmax = max_k |bhat_k|, both from the filter spectrum built
  here in long double (bluestein_filter_ld, bluestein_table_error); a table rounded once has table_err <= u.  The tests
  measure it on the table they pass and hand it to the bound; tests/test_transform_cases.py pins it for the host tables.
Chain, first order, absolute, P = sqrt2 gamma_2 one complex product:
    a^ = fl(x w^)                       ||da||  <= (mu_w + P) ||x||                           (||a|| = ||x||)
    A^ = DIF levels                     ||dA||  <= (L eta_b + mu_w + P) sqrt m ||x||
    p^ = fl(A^ bhat^)                   ||dp||  <= Bmax (L eta_b + mu_w + 2 P + table_err) sqrt m ||x||
    c^ = DIT levels (unnormalised)      ||dc||  <= m Bmax (2 L eta_b + mu_w + 2 P + table_err) ||x||
    crop to n (no larger), times w^, times (T)(scale / m) (m a power of two: exact when scale is; one product, and one
    more u for a scale T does not represent)
    ||X^ - X||_2 <= |scale| Bmax E_conv ||x||_2,   E_conv = 2 L eta_b + 2 mu_w + table_err + 3 P + 2 u
  ||p|| <= Bmax ||A|| and Parseval carry the norms; a real input row only saves roundings in the first product.
  Relative to ||X||_2 = |scale| sqrt n ||x||_2 of the COMPLEX transform (the tests bound the absolute error by that norm
  row by row, because Re X +- Im X of a complex row can be much smaller than X):
    bluestein_rel_bound = SLACK E_conv Bmax / sqrt n          (Bmax = 2.0 .. 2.3 sqrt n; 310 u at m = 8192 in fp32)
  Hartley end Re X + s Im X: |d Re| + |d Im| <= sqrt2 |dX|, one addition and the product with scale: sqrt2 (E + 2 u).
  composition_rel_bound: the same chain with each run of L levels replaced by nk_fftn on (m,), c2c_rel_bound((m,)) (its
  + u is the product with scale = 1 / m), and the three nk_cplx_rows products (scale = 1: exact):
    E_conv = 2 c2c_rel_bound((m,)) + 2 mu_w + table_err + 3 P.
  Axes compose: every axis transform has norm sqrt n_axis, so relative errors ADD over the axes of the seam's N-D walk
  (seam_rel_bound; one more SLACK for the cross terms, one u for a separate scale launch).
* nk_cplx_rows per ELEMENT: scale (re wr - im wi) is two products, one subtraction, one product: gamma_3 times the sum
  of the absolute terms (a contraction into fma only removes roundings); mode 2, scale (re + sgn im): gamma_2.
"""
import functools
import math

import numpy as np
import scipy.fft

LD = np.longdouble
SLACK = 1.01
U64 = 2.0 ** -53


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def gamma(k, u):
    return k * u / (1.0 - k * u)


def factor(n):
    out = []
    for p in (2, 3, 5, 7):
        while n % p == 0:
            out.append(p)
            n //= p
    assert n == 1, "axis lengths factor into 2, 3, 5, 7"
    return out


def eta(radix, u, composed=False):
    """Relative 2-norm error of one stage (radix 2: one level) -- module docstring."""
    mu = 2.0 * u + math.sqrt(2.0) * gamma(2, u) if composed else u
    if radix == 2:
        return mu + gamma(4, u)
    return math.sqrt(2.0 * radix) * gamma(radix + 3, u) + mu + math.sqrt(2.0) * gamma(2, u)


def transform_levels(shape, route=None):
    """(radix-2 levels incl. the extra ones, list of odd radices) of a real transform over `shape` on `route` (nk_plan_route)."""
    twos, odd = 1, []  # the untangle / Hartley level
    for n in shape:
        for p in factor(n):
            if p == 2:
                twos += 1
            else:
                odd.append(p)
    if route is not None and route[3] == 2:
        twos += 1  # inter-level twiddle of the two-level pass
    return twos, odd


def transform_rel_bound(shape, dtype, route=None, composed_axis=None):
    """E with ||H^(x) - H(x)||_2 <= E ||H(x)||_2 for the kernels' transform in `dtype`.  composed_axis: the axis whose pass
    composes its twiddles (MidCfg::TWO of the sandwich's fused first-axis pass)."""
    u = unit_roundoff(dtype)
    twos, odd = transform_levels(shape, route)
    e = twos * eta(2, u) + sum(eta(p, u) for p in odd)
    if composed_axis is not None:
        e += sum(eta(2, u, True) - eta(2, u) for p in factor(shape[composed_axis]) if p == 2)
    return SLACK * e


def sandwich_composed_axis(shape, dtype, field_diagonal):
    """The axis whose pass of a sandwich may compose its twiddles, or None.  MidCfg::TWO (nk_fft.hip) is a compile-time
    property of the fused first-axis kernel and no plan query reports it; its necessary conditions can be read off the
    code: fp32, a scalar diagonal (no `mul` field) and the 32-element schedule, which Sched<float, N> has from N = 512
    on.  Everywhere else the pass reads whole table entries."""
    if np.dtype(dtype) == np.float32 and not field_diagonal and shape[0] >= 512:
        return 0
    return None


def impulse_elem_bound(shape, dtype, route=None):
    u = unit_roundoff(dtype)
    twos, odd = transform_levels(shape, route)
    return SLACK * math.sqrt(2.0) * (twos + 1 + 2 * len(odd)) * eta(2, u)


# ---- references ------------------------------------------------------------------------------------------------------
def hartley_ld(x, ndim, sign=1):
    """Re F + sign Im F over the last `ndim` axes, in long double."""
    x = np.asarray(x).astype(LD)
    F = scipy.fft.fftn(x, axes=tuple(range(x.ndim - ndim, x.ndim)))
    assert F.dtype == np.complex256
    return F.real + sign * F.imag


def hartley_same_precision(x, ndim, sign=1):
    """scipy.fft run in the dtype of x: what a sound transform in T does (the record's third column)."""
    F = scipy.fft.fftn(x, axes=tuple(range(x.ndim - ndim, x.ndim)))
    assert F.dtype == (np.complex64 if x.dtype == np.float32 else np.complex128)
    return (F.real + sign * F.imag).astype(x.dtype)


def hartley_direct_mp(x, sign=1):
    """Direct cas sum with mpmath (50 digits) -- grids of <= 64 points."""
    import mpmath

    mpmath.mp.dps = 50
    x = np.asarray(x)
    assert x.size <= 64
    out = np.empty(x.shape, dtype=LD)
    for k in np.ndindex(*x.shape):
        acc = mpmath.mpf(0)
        for p in np.ndindex(*x.shape):
            th = 2 * mpmath.pi * sum(mpmath.mpf(int(a) * int(b)) / n for a, b, n in zip(k, p, x.shape))
            acc += mpmath.mpf(float(x[p])) * (mpmath.cos(th) - sign * mpmath.sin(th))
        out[k] = LD(mpmath.nstr(acc, 30))
    return out


def impulse_theta(shape, p):
    """2 pi sum k_d p_d / n_d for every k in long double, the argument reduced in integers (modulo the common denominator)."""
    M = 1
    for n in shape:
        M = M * n // math.gcd(M, n)
    m = np.zeros(shape, dtype=np.int64)
    for d, n in enumerate(shape):
        k = np.arange(n, dtype=np.int64).reshape([-1 if e == d else 1 for e in range(len(shape))])
        m = (m + k * (int(p[d]) * (M // n) % M)) % M
    two_pi = LD(2) * np.arctan(LD(1)) * 4
    return two_pi * m.astype(LD) / LD(M)


def impulse_reference(shape, p, sign=1):
    """cas(2 pi sum k_d p_d / n_d) for every k."""
    th = impulse_theta(shape, p)
    return np.cos(th) - sign * np.sin(th)  # Re F + sign Im F of exp(-i theta)


def impulse_positions(shape):
    """The origin, the last and the Nyquist index of every axis, an odd and an even column of the last axis."""
    nd = len(shape)
    pos = [tuple([0] * nd)]
    for d, n in enumerate(shape):
        for v in (n - 1, n // 2):
            p = [0] * nd
            p[d] = v
            pos.append(tuple(p))
    mid = [min(1, n - 1) for n in shape]
    for col in (min(3, shape[-1] - 1) | 1, (shape[-1] // 2) & ~1):
        p = list(mid)
        p[-1] = min(col, shape[-1] - 1)
        pos.append(tuple(p))
    return sorted(set(pos))


def pindex_powerspace(shape):
    """(PowerSpace.pindex of the default-distance grid as int32, number of bins)"""
    import nifty_amd as ift

    ps = ift.PowerSpace(ift.RGSpace(shape).get_default_codomain())
    return np.ascontiguousarray(np.array(ps.pindex).astype(np.int32)), int(ps.shape[0])


def pindex_from_k2(shape):
    """The same index without a PowerSpace: the harmonic partner of a default-distance grid has unit distances on every
    axis, so |k|^2 = sum_d min(i_d, n_d - i_d)^2 is an integer, distinct integers have distinct square roots, and the
    natural binning (one bin per distinct |k|, in ascending order) is the rank of k^2 among its distinct values.
    tests/test_transform_cases.py holds it against pindex_powerspace."""
    k2 = np.zeros((), dtype=np.int64)
    for n in shape:
        ax = np.arange(n, dtype=np.int64)
        k2 = np.add.outer(k2, np.minimum(ax, n - ax) ** 2)
    uniq, inv = np.unique(k2.ravel(), return_inverse=True)
    return np.ascontiguousarray(inv.reshape(shape).astype(np.int32)), int(uniq.size)


# the index of one shape is shared by every case on it; tests/test_batched_transforms_gpu.py alone walks seven shapes
@functools.lru_cache(maxsize=32)
def real_pindex(shape):
    """PowerSpace.pindex of the grid as int32 and the number of bins (computed from the integer k^2: pindex_from_k2), with
    the properties the VJP's mirror merging and the tests rely on checked: symmetric under every single-axis flip, a
    single-member bin, a Nyquist-only bin."""
    pidx, nb = pindex_from_k2(tuple(shape))
    pidx.setflags(write=False)  # cached: shared by every case of the shape
    idx = np.indices(shape)
    for d in range(len(shape)):
        flip = tuple((-idx[e]) % shape[e] if e == d else idx[e] for e in range(len(shape)))
        assert np.array_equal(pidx, pidx[flip])
    counts = np.bincount(pidx.ravel(), minlength=nb)
    assert counts.min() > 0 and counts[pidx[tuple([0] * len(shape))]] == 1
    on_nyq = np.zeros(shape, dtype=bool)
    for d, n in enumerate(shape):
        on_nyq |= idx[d] == n // 2
    # a bin all of whose members lie on a Nyquist plane: as many members on the planes as members (one pass over the
    # grid instead of one per bin)
    assert np.any(np.bincount(pidx.ravel(), weights=on_nyq.ravel(), minlength=nb) == counts)
    return pidx, nb


# ---- fused calls: long-double reference and bounds -------------------------------------------------------------------
def nonlin_ld(kind, s):
    """g, g', g'' of NK_NL_ID / EXP / SIGMOID (0.5 + 0.5 tanh) in long double."""
    if kind == 1:
        e = np.exp(s)
        return e, e, e
    if kind == 2:
        th = np.tanh(s)
        gp = LD(0.5) - LD(0.5) * th * th
        return LD(0.5) + LD(0.5) * th, gp, -2 * th * gp
    return s, np.ones_like(s), np.zeros_like(s)


def prologue_ld(pro, a):
    """x fed into the transform and x_abs = the sum of the absolute terms; a: dict of T-valued (or fp64 table) arrays,
    amp / damp already gathered to the grid (a['a'], a['da'])."""
    x_in = a["in"].astype(LD)
    if pro == 0:
        return x_in, None
    if pro == 3:
        x = x_in * a["in2"].astype(LD)
        return x, np.abs(x)
    t1 = a["a"].astype(LD) * x_in
    if pro == 1:
        return t1, np.abs(t1)
    t2 = a["da"].astype(LD) * a["in2"].astype(LD)
    return t1 + t2, np.abs(t1) + np.abs(t2)


def l2(x):
    return float(np.sqrt(np.sum(np.asarray(x, dtype=LD) ** 2)))


def transform_abs_bound(x, x_abs, shape, dtype, scale_abs, rel, pro_ops=3):
    """||t^ - t||_2 for t = scale H(PRO(...)): the transform part and the prologue's roundings through ||H||_2 = sqrt N."""
    n = float(np.prod(shape))
    u = unit_roundoff(dtype)
    e = rel * math.sqrt(n) * l2(x)
    if x_abs is not None:
        e += (1.0 + rel) * math.sqrt(n) * gamma(pro_ops, u) * l2(x_abs)
    return scale_abs * e


def store_term(out, dtype):
    """the single rounding of an fp64 epilogue result to T"""
    return (unit_roundoff(dtype) + 8 * U64) * l2(out)


TERMS_PER_THREAD, WAVE_STEPS, FOLD_BLOCKS = 128, 6, 256


def reduction_depth(workspace_bytes, atomics=None):
    """h of the device's energy / curvature sum (module docstring, Reductions).  workspace_bytes: the plan's
    nk_plan_workspace_bytes when the call got a workspace (slots and folds); None with atomics = the number of workgroups
    on the no-workspace path."""
    if workspace_bytes is None:
        return TERMS_PER_THREAD + WAVE_STEPS + 16 + int(atomics) + 4
    n_slots = workspace_bytes // 16
    per_thread = -(-(-(-n_slots // FOLD_BLOCKS)) // 256)
    return TERMS_PER_THREAD + WAVE_STEPS + per_thread + (WAVE_STEPS + 4) + (WAVE_STEPS + 4 + 1) + 4


def sum_bound(terms, weight_l2, et, depth=None):
    """|sum^ - sum| of an fp64 reduction over `terms` of summation depth `depth` (None: one running sum over all terms,
    what the host emulation does) whose inputs inherit ||dt||_2 <= et through weights of 2-norm weight_l2."""
    terms = np.asarray(terms, dtype=LD).ravel()
    h = terms.size + 4 if depth is None else depth
    return float(gamma(h, U64) * np.sum(np.abs(terms)) * SLACK + weight_l2 * et)


# ---- comparators -----------------------------------------------------------------------------------------------------
def err_l2(got, ref):
    return l2(np.asarray(got).astype(LD) - ref)


def within_l2(got, ref, bound):
    """(ok, error): 2-norm comparator; a NaN anywhere fails."""
    e = err_l2(got, ref)
    return bool(np.isfinite(e) and e <= bound), e


def within_elem(got, ref, bound):
    """(ok, worst error / bound): element-wise comparator; bound a scalar or an array."""
    d = np.abs(np.asarray(got).astype(LD) - ref)
    worst = float(np.max(d / bound)) if d.size else 0.0
    return bool(np.isfinite(worst) and worst <= 1.0), worst


# ---- the routes of nk_run_hartley and the smallest shapes that reach them --------------------------------------------
# (shape, route of the fp64 plan, route of the fp32 plan) -- route = (pipe, last, mid, first) as nk_plan_route reports it
GEN1, REG1 = (0, 0, -1, -1), (0, 1, -1, -1)
ROUTES = [
    ((2,), GEN1, GEN1), ((30,), GEN1, GEN1), ((500,), GEN1, GEN1),
    ((128,), REG1, REG1), ((8192,), REG1, REG1),
    ((10, 12), (1, 0, -1, 0), (1, 0, -1, 0)), ((12, 250), (1, 0, -1, 0), (1, 0, -1, 0)),
    ((6, 5, 14), (1, 0, 0, 0), (1, 0, 0, 0)), ((9, 25, 28), (1, 0, 0, 0), (1, 0, 0, 0)),
    # contiguous-first hybrids: register-resident pass A and / or pass B beside the generic pass C
    ((30, 128), (1, 1, -1, 0), (1, 1, -1, 0)), ((64, 8192), (1, 1, -1, 0), (1, 1, -1, 0)),
    ((6, 10, 128), (1, 1, 0, 0), (1, 1, 0, 0)), ((6, 64, 128), (1, 1, 1, 0), (1, 1, 1, 0)),
    ((6, 64, 96), (1, 0, 1, 0), (1, 0, 1, 0)),
    ((6, 64, 48), (1, 0, 1, 0), (1, 0, 0, 0)),  # rows of 24 columns: whole tiles of the strided kernel in fp64 only
    # strided-first
    ((64, 64), (2, 1, -1, 1), (2, 1, -1, 1)), ((64, 128), (2, 1, -1, 1), (2, 1, -1, 1)),
    ((2048, 64), (2, 1, -1, 1), (2, 1, -1, 1)), ((64, 4096), (2, 1, -1, 1), (2, 1, -1, 1)),
    ((4096, 64), (2, 1, -1, 2), (2, 1, -1, 1)),  # two-level first axis in fp64 only
    ((64, 64, 64), (2, 1, 1, 1), (2, 1, 1, 1)), ((128, 64, 256), (2, 1, 1, 1), (2, 1, 1, 1)),
    ((64, 64, 1024), (2, 1, 1, 1), (2, 1, 1, 1)),
]
# the shapes the fused classes run on: the smallest of every route, every hybrid but the largest (+ the single-pair VJP
# final pass of (64, 4096) fp64)
CLASS_SHAPES = [(30,), (128,), (10, 12), (6, 5, 14), (30, 128), (6, 10, 128), (6, 64, 128), (6, 64, 96), (6, 64, 48), (64, 64),
                (64, 128), (64, 4096), (4096, 64), (64, 64, 64)]
SANDWICH = [((64, 128), None), ((64, 64, 128), None), ((64, 64, 1024), None), ((1024, 64, 128), np.float32),
            ((64, 1024, 128), np.float32)]  # (shape, the only dtype it runs in or None = both)


# nk_hartley_fused_batch (tests/test_batched_transforms_gpu.py): the batched twins of the first and the final pass exist for
# axis lengths 512 .. 4096 and need both axes >= 512 -- the smallest grid of every twin instantiation, same columns as ROUTES
SF1, SF2 = (2, 1, -1, 1), (2, 1, -1, 2)
BATCH_SHAPES = [
    ((512, 512), SF1, SF1),
    ((1024, 512), SF1, SF1), ((512, 1024), SF1, SF1),
    ((2048, 512), SF1, SF1), ((512, 2048), SF1, SF1),  # final pass of 2048 fp64 points: the single-pair VJP build
    ((4096, 512), SF2, SF1),  # two-level first axis in fp64 only
    ((512, 4096), SF1, SF1),  # final pass of 4096 points: the single-pair VJP build in both dtypes
]


def final_single_pair_vjp(shape, dtype):
    """2-D VJP final pass on single line pairs instead of the couple tile (nk_final_single_2d, nk_fft2.h): lines whose
    couple tile exceeds 60 KiB of LDS -- 2048 and 4096 points in fp64, 4096 in fp32"""
    return len(shape) == 2 and shape[-1] >= (4096 if np.dtype(dtype) == np.float32 else 2048)


def route_of(shape, dtype):
    for s, r64, r32 in ROUTES + BATCH_SHAPES:
        if s == tuple(shape):
            return r32 if np.dtype(dtype) == np.float32 else r64
    raise KeyError(shape)


PROLOGUES = ["plain", "mul", "amp_table", "amp_afield", "jvp_tables", "jvp_afield_dampT", "jvp_afield_dafield"]
PROLOGUES_OCTANT = ["amp_afield_oct", "jvp_dafield_oct"]  # field_octant: plans with nk_plan_octant_vjp != 0 only
EPILOGUES = (["mul_field", "mul_scalar"] + [f"nonlin_{n}" for n in ("id", "exp", "sigmoid")] +
             [f"lh_{k}_{n}" for k in ("gauss", "gaussf", "poisson") for n in ("id", "exp", "sigmoid")])
VJPS = ["vjp_atomic", "vjp_copies8", "vjp_addend_acc", "vjp_carry"]  # + vjp_w8 (octant plans) / vjp_wfull (the others)
NL = {"id": 0, "exp": 1, "sigmoid": 2}


def octant_slices(shape):
    return tuple(slice(0, n // 2 + 1) for n in shape)


def fold_to_octant(a, shape):
    """sum of a over the sign-flip images of every octant point (what w8 holds for a = xi t)"""
    idx = np.indices(shape)
    folded = tuple(np.minimum(idx[d], (shape[d] - idx[d]) % shape[d]) for d in range(len(shape)))
    out = np.zeros(tuple(n // 2 + 1 for n in shape), dtype=a.dtype)
    np.add.at(out, folded, a)
    return out


class FusedCase:
    """Operands (numpy, T-valued), the nk_fuse record and the long-double reference with its bounds of ONE nk_hartley_fused
    call.  `inputs`: name -> array the call only reads; `outputs`: name -> initial array the call writes (or must leave
    alone); fill(fuse, ptr) sets the record from ptr(name) -> address; reference(sign) -> name -> (ref, kind, bound),
    kind 'l2' (2-norm), 'elem' (per element) or 'same' (bit-wise unchanged)."""

    def __init__(self, shape, dtype, pro, epi, octant_plan, seed=0, sandwich=None, io32=False):
        """sandwich = (scale_first, mul_scalar, field diagonal?): the call is nk_hartley_sandwich, t = scale H(D H(x)).
        io32: nk_fuse.io32 -- float arrays at both ends of an fp64 plan (AMP prologue with an fp64 octant field, LIKELIHOOD)."""
        self.shape, self.dtype, self.pro, self.epi, self.octant_plan = tuple(shape), np.dtype(dtype), pro, epi, octant_plan
        self.sandwich, self.io_dtype, self.pro_ops = sandwich, np.dtype(np.float32 if io32 else dtype), 3
        rng = np.random.default_rng(seed)
        T = self.dtype
        n = int(np.prod(shape))
        self.n = n
        normal = lambda: rng.normal(size=shape).astype(T)  # noqa: E731
        self.inputs, self.outputs, self.set = {}, {}, {}
        self.scale, self.offset = 0.3 / math.sqrt(n), 0.0
        I, O, S = self.inputs, self.outputs, self.set
        I["in"] = normal()
        need_bins = pro != "plain" and pro != "mul" or epi.startswith("vjp")
        if need_bins:
            pidx, nb = real_pindex(shape)
            self.pidx, self.nb = pidx, nb
            # one more bin than the grid uses: NaN amplitudes behind the table's end show a gather past `pidx`
            I["pidx"] = pidx
            I["amp"] = np.append(rng.uniform(0.5, 1.5, size=nb) * rng.choice([-1.0, 1.0], size=nb), np.nan)
            I["damp"] = np.append(rng.normal(size=nb), np.nan)
        sl = octant_slices(shape)
        # ---- prologue
        if pro == "mul":
            I["in2"] = normal()
            S["pro"] = 3
        elif pro.startswith("amp"):
            S["pro"] = 1
            if pro != "amp_table":
                af = I["amp"][pidx].astype(T)
                I["afield"] = np.ascontiguousarray(af[sl]) if pro.endswith("_oct") else af
        elif pro.startswith("jvp"):
            S["pro"] = 2
            I["in2"] = normal()
            if pro != "jvp_tables":
                af, daf = I["amp"][pidx].astype(T), I["damp"][pidx].astype(T)
                octf = pro.endswith("_oct")
                I["afield"] = np.ascontiguousarray(af[sl]) if octf else af
                if pro == "jvp_pidxoct_oct":  # da gathered from its T table through the OCTANT bin index (sandwich)
                    I["dampT"], I["pidx_octant"] = I["damp"].astype(T), np.ascontiguousarray(pidx[sl])
                elif pro == "jvp_afield_dampT":
                    I["dampT"] = I["damp"].astype(T)
                else:
                    I["dafield"] = np.ascontiguousarray(daf[sl]) if octf else daf
        else:
            S["pro"] = 0
        if pro.endswith("_oct"):
            S["field_octant"] = 1
        if pro == "jvp_cg_oct":
            # the pending CG direction update rides in the prologue: in <- max(0, s[2] / s[0]) in + cg_r, written back
            I["cg_r"], I["cg_scal"] = normal(), np.array([2.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0])
            O["in"] = I.pop("in")
            self.pro_ops = 5  # two more roundings in front of the products
        if sandwich is not None:
            S["mul_scalar"] = sandwich[1]
            if sandwich[2]:
                I["mul"] = normal()
        # ---- epilogue
        O["out"] = np.full(shape, np.nan, dtype=T)
        if epi == "affine":
            S["epi"], self.scale, self.offset = 0, 0.7, -1.25
        elif epi.startswith("mul"):
            S["epi"], S["mul_scalar"] = 1, -1.5
            if epi == "mul_field":
                I["mul"] = normal()
        elif epi.startswith("nonlin"):
            S["epi"], S["nonlin"], self.offset = 4, NL[epi.split("_")[1]], 0.3
            O["out2"] = np.full(shape, np.nan, dtype=T)
        elif epi.startswith("lh"):
            _, kind, nl = epi.split("_")
            S["epi"], S["nonlin"], S["lh_kind"] = 3, NL[nl], 1 if kind == "poisson" else 0
            self.offset = 3.0 if (kind == "poisson" and nl == "id") else 0.3
            O["out2"] = np.full(shape, np.nan, dtype=T)
            O["value"] = np.array([0.625])  # the call ADDS its energy
            if kind == "poisson":
                I["data"] = rng.poisson(3.0, size=shape).astype(np.int64)
            else:
                I["data"] = normal()
                S["icov_scalar"] = 2.5
                if kind == "gaussf":
                    I["icov"] = rng.uniform(0.5, 1.5, size=shape).astype(T)
        elif epi.startswith("vjp"):
            S["epi"] = 2
            I["xi"] = normal()
            O["abar"] = np.append(rng.normal(size=self.nb), 7.0)  # the call ADDS to abar; the extra bin stays
            if octant_plan and epi in ("vjp_addend_acc", "vjp_w8"):
                I.setdefault("afield", np.ascontiguousarray(I["amp"][self.pidx].astype(T)[sl]))
                S["field_octant"] = 1
            if epi == "vjp_copies8":
                self.stride = (self.nb + 1 + 31) // 32 * 32
                O["abar"] = np.zeros(8 * self.stride)
                S["abar_copies"], S["abar_stride"] = 8, self.stride
            if epi in ("vjp_addend_acc", "vjp_carry", "vjp_w8"):
                I["addend"], S["addend_scale"], S["accumulate"] = normal(), 2.0, 1
                O["out"] = normal()
            if epi == "vjp_addend_acc" and octant_plan:
                O["value"] = np.array([-0.375])
            if epi == "vjp_carry":
                I["carry1"], I["carry2"] = normal(), normal()
            if epi == "vjp_w8":
                O["w8"] = np.full(tuple(m // 2 + 1 for m in shape), np.nan)
                if len(shape) == 3:
                    O["w8max"] = np.array([np.nan])
            if epi == "vjp_wfull":
                O["wfull"] = np.full(shape, np.nan)
        else:
            raise KeyError(epi)
        S["scale"], S["offset"] = self.scale, self.offset
        if io32:
            S["io32"] = 1
            for d in (I, O):
                for k in ("in", "data", "icov", "out", "out2"):
                    if k in d and d[k].dtype == T:
                        d[k] = d[k].astype(np.float32)

    def fill(self, f, ptr):
        for k, v in self.set.items():
            setattr(f, k, v)
        for k in self.inputs:
            setattr(f, "in_" if k == "in" else k, ptr(k))
        for k in self.outputs:
            setattr(f, "in_" if k == "in" else k, ptr(k))
        return f

    def transform_part(self, sign, rel):
        I = self.inputs
        a = dict(I)
        if "pidx" in I:
            # the amplitude factor as the prologue reads it: the T-valued field, or the double table
            a["a"] = I["amp"][self.pidx].astype(self.dtype) if "afield" in I else I["amp"][self.pidx]
            if "dampT" in I:
                a["da"] = I["dampT"][self.pidx]
            elif "dafield" in I:
                a["da"] = I["damp"][self.pidx].astype(self.dtype)
            else:
                a["da"] = I["damp"][self.pidx]
        if "cg_r" in I:
            beta = max(0.0, I["cg_scal"][2] / I["cg_scal"][0])
            a["in"] = LD(beta) * self.outputs["in"].astype(LD) + I["cg_r"].astype(LD)
            self._in_new = a["in"]
            self._in_abs = LD(beta) * np.abs(self.outputs["in"].astype(LD)) + np.abs(I["cg_r"].astype(LD))
        x, x_abs = prologue_ld(self.set["pro"], a)
        self._x = x
        nd, n = len(self.shape), float(self.n)
        if self.sandwich is None:
            # both conventions are Re F +- Im F of ONE long-double spectrum; a case asked for both (the batched tests)
            # transforms once.  The operands of a case are fixed once a reference has been taken.
            if getattr(self, "_spectrum", None) is None:
                self._spectrum = scipy.fft.fftn(x)
                assert self._spectrum.dtype == np.complex256
            t = LD(self.scale) * (self._spectrum.real + sign * self._spectrum.imag)
            return t, transform_abs_bound(x, x_abs, self.shape, self.dtype, abs(self.scale), rel, self.pro_ops)
        sf, ms, _ = self.sandwich
        s1 = LD(sf) * hartley_ld(x, nd, sign)
        e1 = transform_abs_bound(x, x_abs, self.shape, self.dtype, abs(sf), rel, self.pro_ops)
        d = LD(ms) * (I["mul"].astype(LD) if "mul" in I else LD(1))
        mid = d * s1
        e_mid = float(np.max(np.abs(d))) * e1 + gamma(3, unit_roundoff(self.dtype)) * l2(mid)
        t = LD(self.scale) * hartley_ld(mid, nd, sign)
        return t, abs(self.scale) * math.sqrt(n) * ((1.0 + rel) * e_mid + rel * l2(mid))

    def transform_input(self, sign=1):
        """the prologue's output rounded to T: the array the transform itself sees"""
        self.transform_part(sign, 0.0)
        return self._x.astype(self.dtype)

    def reference(self, sign, rel, depth=None):
        """rel: transform_rel_bound of the plan's route; depth: reduction_depth of the call on the device (None: the
        emulation's single running sum)"""
        I, O, S, T = self.inputs, self.outputs, self.set, self.io_dtype
        u = unit_roundoff(T)
        t, et = self.transform_part(sign, rel)
        epi, ref = self.epi, {}
        if "cg_r" in I:  # the written-back direction: one fp64 expression rounded to T
            ref["in"] = (self._in_new, "elem", (unit_roundoff(T) + 4 * U64) * self._in_abs + np.finfo(np.float64).tiny)
        if epi == "affine":
            out = t + LD(self.offset)
            ref["out"] = (out, "l2", et + store_term(out, T))
        elif epi.startswith("mul"):
            m = LD(S["mul_scalar"]) * (I["mul"].astype(LD) if "mul" in I else LD(1))
            out = t * m
            ref["out"] = (out, "l2", float(np.max(np.abs(m))) * et + store_term(out, T))
        elif epi.startswith("nonlin"):
            g, gp, gpp = nonlin_ld(S["nonlin"], t + LD(self.offset))
            ref["out"] = (g, "l2", SLACK * float(np.max(np.abs(gp))) * et + store_term(g, T))
            ref["out2"] = (gp, "l2", SLACK * float(np.max(np.abs(gpp))) * et + store_term(gp, T))
        elif epi.startswith("lh"):
            s = t + LD(self.offset)
            g, gp, gpp = nonlin_ld(S["nonlin"], s)
            if S["lh_kind"] == 0:
                ic = I["icov"].astype(LD) if "icov" in I else LD(S["icov_scalar"])
                r = g - I["data"].astype(LD)
                e, gs, w = LD(0.5) * ic * r * r, gp * ic * r, gp * gp * ic
                dgs, dw = ic * (gpp * r + gp * gp), 2 * gp * gpp * ic
            else:
                d = I["data"].astype(LD)
                e, gs, w = g - d * np.log(g), gp * (1 - d / g), gp * gp / g
                dgs, dw = gpp * (1 - d / g) + gp * gp * d / (g * g), 2 * gp * gpp / g - gp ** 3 / (g * g)
            ref["out"] = (gs, "l2", SLACK * float(np.max(np.abs(dgs))) * et + store_term(gs, T))
            ref["out2"] = (w, "l2", SLACK * float(np.max(np.abs(dw))) * et + store_term(w, T))
            # dE/dt = gs: first order ||gs||_2 et, second order 1/2 max |dgs| et^2
            vb = sum_bound(e, l2(gs), et, depth) + 0.5 * float(np.max(np.abs(dgs))) * et * et + 4 * U64 * abs(float(O["value"][0]))
            ref["value"] = (np.array([LD(O["value"][0]) + np.sum(e)]), "elem", vb)
        else:
            pidx = self.pidx
            amp_at = (I["amp"][pidx].astype(self.dtype) if "afield" in I else I["amp"][pidx]).astype(LD)  # field (T) or double table
            xi = I["xi"].astype(LD)
            own = amp_at * t
            b_own = float(np.max(np.abs(amp_at))) * et
            if "addend" in I:
                own = own + LD(S["addend_scale"]) * I["addend"].astype(LD)
            out, b_out = own, b_own + store_term(own, T)
            for k in ("carry1", "carry2"):
                if k in I:
                    out = out + I[k].astype(LD)
                    b_out += u * l2(out)
            if S.get("accumulate"):
                out = out + O["out"].astype(LD)
                b_out += u * l2(out)
            ref["out"] = (out, "l2", SLACK * b_out)
            xt = xi * t
            if "w8" in O or "wfull" in O:
                w8 = fold_to_octant(xt, self.shape)
                wl2 = math.sqrt(float(np.max(fold_to_octant(xi * xi, self.shape))))
                bw = gamma(12, U64) * l2(fold_to_octant(np.abs(xt), self.shape)) + wl2 * et
                ref["w8" if "w8" in O else "wfull_folded"] = (w8, "l2", SLACK * bw)
                ref["abar"] = (O["abar"].astype(LD), "same", 0.0)
                if "w8max" in O:
                    ref["w8max"] = (w8, "w8max", 0.0)
            else:
                nbp = self.nb + 1
                flat = pidx.ravel()
                order = np.argsort(flat, kind="stable")
                cuts = np.searchsorted(flat[order], np.arange(self.nb))
                assert np.all(np.diff(np.append(cuts, flat.size)) > 0)  # every bin of a PowerSpace has members
                sums = np.append(np.add.reduceat(xt.ravel()[order], cuts), LD(0))  # every bin summed on its own, in long double
                cnt = np.bincount(flat, minlength=nbp).astype(np.float64)
                sabs = np.bincount(flat, weights=np.abs(xt).astype(np.float64).ravel(), minlength=nbp)
                sxi2 = np.bincount(flat, weights=(xi * xi).astype(np.float64).ravel(), minlength=nbp)
                copies = S.get("abar_copies", 0) == 8
                init = np.zeros(nbp, dtype=LD) if copies else O["abar"].astype(LD)
                bound = SLACK * ((cnt + 12) * U64 * 1.0000001 * (sabs + np.abs(init.astype(np.float64))) + np.sqrt(sxi2) * et)
                bound[self.nb] = 0.0  # the extra bin: untouched
                ref["abar_bins"] = (init + sums, "elem_bins", bound)
            if "value" in O:
                terms = I["addend"].astype(LD) * out  # *value += sum addend * out
                ref["value"] = (np.array([LD(O["value"][0]) + np.sum(terms)]), "elem",
                                sum_bound(terms, l2(I["addend"]), SLACK * b_out, depth) + 4 * U64 * abs(float(O["value"][0])))
        return ref


def compare(case, ref, got):
    """Check every output of a fused call against reference(): rows (name, error, bound, ok).  got: name -> array after
    the call (the names of case.outputs)."""
    rows = []
    for name, (r, kind, bound) in ref.items():
        if kind == "l2":
            g = fold_to_octant(got["wfull"].astype(LD), case.shape) if name == "wfull_folded" else got[name]
            ok, e = within_l2(g, r, bound)
        elif kind == "elem":
            ok, worst = within_elem(got[name], r, bound)
            e, bound = float(np.max(np.abs(np.asarray(got[name]).astype(LD) - r))), float(np.max(bound))
        elif kind == "same":
            ok = np.array_equal(got[name].view(np.uint64), np.asarray(r, dtype=np.float64).view(np.uint64))
            e, bound = (0.0 if ok else np.inf), 0.0
        elif kind == "elem_bins":
            a = got["abar"]
            if case.set.get("abar_copies", 0) == 8:  # what nk_fold_copies computes
                a = a.reshape(8, case.stride).sum(0)[:case.nb + 1]
            d = np.abs(a.astype(LD) - r)
            ok = bool(np.all(np.isfinite(a)) and np.all(d <= bound))
            e, bound = float(np.max(d)), float(np.max(bound))
        elif kind == "w8max":  # the header's promise: an upper bound of max |w8| tight to fp32 rounding
            m, w = float(got["w8max"][0]), float(np.max(np.abs(got["w8"])))
            ok = w <= m <= w * (1.0 + 2.0 ** -23)
            e, bound = m - w, w * 2.0 ** -23
        else:
            raise KeyError(kind)
        rows.append((name, float(e), float(bound), bool(ok)))
    return rows


# ---- complex transforms: nk_fftn, nk_bluestein_rows, the chirp-z composition (module docstring) ----------------------
CLD = np.clongdouble


def complex_dtype(dtype):
    return np.complex64 if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.complex128


def normal_complex(shape, dtype, seed):
    """seeded complex normal data in T: the inputs the device tests and the host tests of the bounds share"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(complex_dtype(dtype))


def fft_ld(x, ndim, inverse=False):
    """Unnormalised c2c transform over the last `ndim` axes in long double (exp(+i ..) for inverse)."""
    x = np.asarray(x).astype(CLD)
    axes = tuple(range(x.ndim - ndim, x.ndim))
    F = scipy.fft.ifftn(x, axes=axes, norm="forward") if inverse else scipy.fft.fftn(x, axes=axes)
    assert F.dtype == np.complex256
    return F


def fft_same_precision(x, ndim, inverse=False):
    """scipy.fft run in the dtype of x: what a sound transform in T does"""
    axes = tuple(range(x.ndim - ndim, x.ndim))
    F = scipy.fft.ifftn(x, axes=axes, norm="forward") if inverse else scipy.fft.fftn(x, axes=axes)
    assert F.dtype == x.dtype
    return F


def fft_direct_mp(x, inverse=False):
    """Direct DFT sum with mpmath (50 digits) -- grids of <= 64 points."""
    import mpmath

    mpmath.mp.dps = 50
    x = np.asarray(x)
    assert x.size <= 64
    out = np.empty(x.shape, dtype=CLD)
    for k in np.ndindex(*x.shape):
        acc = mpmath.mpc(0)
        for p in np.ndindex(*x.shape):
            th = 2 * mpmath.pi * sum(mpmath.mpf(int(a) * int(b)) / n for a, b, n in zip(k, p, x.shape))
            acc += mpmath.mpc(float(x[p].real), float(x[p].imag)) * mpmath.expj(th if inverse else -th)
        out[k] = LD(mpmath.nstr(acc.real, 30)) + 1j * LD(mpmath.nstr(acc.imag, 30))
    return out


def impulse_reference_c2c(shape, p, inverse=False):
    """exp(-+ 2 pi i sum k_d p_d / n_d): the transform of a unit impulse at p"""
    th = impulse_theta(shape, p)
    return np.cos(th) + (1j if inverse else -1j) * np.sin(th)


def l2c(x):
    """2-norm of a real or complex array in long double"""
    return float(np.sqrt(np.sum(np.abs(np.asarray(x).astype(CLD)) ** 2)))


def err_l2c(got, ref):
    return l2c(np.asarray(got).astype(CLD) - ref)


def within_l2c(got, ref, bound):
    e = err_l2c(got, ref)
    return bool(np.isfinite(e) and e <= bound), e


def within_elem_c(got, ref, bound):
    """(ok, worst error / bound): element-wise comparator of complex (or real) arrays; a NaN anywhere fails"""
    d = np.abs(np.asarray(got).astype(CLD) - ref)
    worst = float(np.max(d / bound)) if d.size else 0.0
    return bool(np.isfinite(worst) and worst <= 1.0), worst


def c2c_levels(shape):
    fs = [p for n in shape for p in factor(n)]
    return fs.count(2), [p for p in fs if p != 2]


def c2c_rel_bound(shape, dtype):
    """E with ||F^(x) - F(x)||_2 <= E ||F(x)||_2 for nk_fftn in `dtype` (scale exactly representable in T)."""
    u = unit_roundoff(dtype)
    twos, odd = c2c_levels(shape)
    return SLACK * (twos * eta(2, u) + sum(eta(p, u) for p in odd)) + u


def c2c_impulse_elem_bound(shape, dtype):
    u = unit_roundoff(dtype)
    twos, odd = c2c_levels(shape)
    return SLACK * (twos + 2 * len(odd)) * eta(2, u) + u


# the c2c set-up of nk_plan_create restated (nk_fft.hip; nk_pick_strided_tile of nk_plan.h without its environment knobs)
def pick_strided_tile(n, inner, csize, outer):
    def grow(t, budget):
        while 2 * t <= inner and n * 2 * t * csize <= budget and 2 * t * csize <= 256:
            t *= 2
        return t

    t = grow(1, 128 * 1024)
    if t * csize < 64:
        t = grow(t, 152 * 1024)
    while t > 4 and outer * -(-inner // t) < 256:
        t //= 2
    return t


def c2c_lds_bytes(shape, dtype, batch=1):
    """dynamic LDS of (k_c2c_contig, k_c2c_strided middle axis, k_c2c_strided first axis); 0 = no such pass"""
    csize = 8 if np.dtype(dtype) == np.float32 else 16
    nl = shape[-1]
    na = shape[0] if len(shape) >= 2 else 1
    nm = shape[1] if len(shape) == 3 else 1
    line = (nl + nl // 16 + 1) * csize
    tile = max(1, min(32 * 1024 // line, -(-2048 // nl)))
    tile = min(tile, batch * na * nm)
    mid = nm * pick_strided_tile(nm, nl, csize, batch * na) * csize if len(shape) == 3 else 0
    first = na * pick_strided_tile(na, nm * nl, csize, batch) * csize if len(shape) >= 2 else 0
    return tile * line, mid, first


def c2c_line_limit(dtype):
    """complex values of one padded line the contiguous c2c pass keeps in LDS: 144 KiB"""
    return 144 * 1024 // (8 if np.dtype(dtype) == np.float32 else 16)


def is_smooth(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def c2c_longest(dtype):
    """the largest even 7-smooth nl with nl + nl / 16 + 1 <= 9216 (fp64) / 18432 (fp32)"""
    lim = c2c_line_limit(dtype)
    for nl in range(lim, 1, -1):
        if nl % 2 == 0 and nl + nl // 16 + 1 <= lim:
            r = nl
            for p in (2, 3, 5, 7):
                while r % p == 0:
                    r //= p
            if r == 1:
                return nl
    raise AssertionError


C2C_SHAPES = [(2,), (6,), (30,), (500,), (1024,), (4096,), (6, 10), (15, 14), (64, 64), (7, 500), (1000, 8), (6, 5, 14), (9, 25, 28),
              (64, 6, 128)]
# one shape per dtype whose strided (first-axis) pass needs more than 64 KiB of LDS: tile 4 (rows of 64 B / 32 B), n * 4 * csize
C2C_BIG_LDS = {np.dtype(np.float64): ((1280, 8), 81920), np.dtype(np.float32): ((2560, 8), 81920)}
# two fp64 plans that both need more than 64 KiB in k_c2c_strided<double>, the first more than the second
C2C_TWO_PLANS = (((2048, 8), 131072), ((1280, 8), 81920))


def c2c_shapes(dtype):
    return C2C_SHAPES + [C2C_BIG_LDS[np.dtype(dtype)][0], (c2c_longest(dtype),)]


# ---- chirp-z ------------------------------------------------------------------------------------------------------------
MU_W64, MU_TW64 = 17.0, 5.0  # host evaluation of the chirp / of the level twiddles in double, in units of u64


def smallest_m(n):
    return 1 << max(2, (2 * n - 2).bit_length())


def bit_reverse(m):
    bits = m.bit_length() - 1
    rev = np.zeros(m, dtype=np.int64)
    for bit in range(bits):
        rev |= ((np.arange(m) >> bit) & 1) << (bits - 1 - bit)
    return rev


@functools.lru_cache(maxsize=64)
def bluestein_filter_ld(n, m, inverse=False):
    """(chirp w[n], spectrum bhat[m] of the cyclic filter in natural order, Bmax = max |bhat|) in long double"""
    k = np.arange(n, dtype=np.int64)
    ang = (LD(4) * np.arctan(LD(1))) * (k * k % (2 * n)).astype(LD) / LD(n)
    w = np.cos(ang) + (1j if inverse else -1j) * np.sin(ang)
    b = np.zeros(m, dtype=CLD)
    b[:n] = w.conj()
    b[m - n + 1:] = w.conj()[1:][::-1]
    bhat = scipy.fft.fft(b)
    assert bhat.dtype == np.complex256
    for a in (w, bhat):
        a.setflags(write=False)
    return w, bhat, float(np.max(np.abs(bhat)))


def bluestein_table_error(bhat_used, n, m, inverse=False):
    """max_k |bhat_used_k - bhat_k| / Bmax of a filter spectrum in NATURAL order as a kernel is handed it"""
    _, bhat, bmax = bluestein_filter_ld(n, m, inverse)
    return float(np.max(np.abs(np.asarray(bhat_used).astype(CLD) - bhat))) / bmax


def host_table_error_ceiling(n, m, dtype, inverse=False):
    """ceiling of bluestein_table_error for the tables backend._bluestein_tables builds on the host: rounded once in fp32
    (the double transform behind it is far below u); in fp64 the norm-wise bound of a double transform of L levels on the
    filter built from the perturbed chirp (every entry within mu_w), taken per element"""
    if np.dtype(dtype) == np.float32:
        return 1.001 * 2.0 ** -24
    L = m.bit_length() - 1
    bmax = bluestein_filter_ld(n, m, inverse)[2]
    return (SLACK * L * eta(2, U64) * math.sqrt(m * (2.0 * n - 1)) + MU_W64 * U64 * (2 * n - 1)) / bmax


def device_filter_l2_bound(n, m, dtype, inverse=False):
    """||fb^ - bhat||_2 of the filter spectrum the composition transforms ON THE DEVICE with nk_fftn: the filter's entries are
    the conjugate chirp rounded to T (each within mu_w, ||db|| <= mu_w ||b||, carried by the transform as mu_w ||bhat||) and
    the transform itself errs by c2c_rel_bound((m,))"""
    bhat = bluestein_filter_ld(n, m, inverse)[1]
    return (c2c_rel_bound((m,), dtype) + _table_mu(dtype, MU_W64)) * l2c(bhat)


def _table_mu(dtype, host_u64):
    return (2.0 ** -24 if np.dtype(dtype) == np.float32 else 0.0) + host_u64 * U64


def _chirp_tail(e_conv, n, m, dtype, hartley, inverse):
    u = unit_roundoff(dtype)
    e = SLACK * e_conv * bluestein_filter_ld(n, m, inverse)[2] / math.sqrt(n)
    return math.sqrt(2.0) * (e + 2 * u) if hartley else e


def bluestein_rel_bound(n, m, dtype, real_in=False, hartley=False, inverse=False, table_err=None):
    """E with ||X^ - X||_2 <= E |scale| sqrt n ||x||_2 for one row of nk_bluestein_rows (module docstring, CHIRP-Z).
    real_in saves roundings only; table_err: bluestein_table_error of the table in use (None: rounded once, u)."""
    u = unit_roundoff(dtype)
    L = m.bit_length() - 1
    assert m == 1 << L and m >= max(4, 2 * n - 1)
    level = _table_mu(dtype, MU_TW64) + gamma(4, u)
    prod = math.sqrt(2.0) * gamma(2, u)
    tab = u if table_err is None else table_err
    e_conv = 2 * L * level + 2 * _table_mu(dtype, MU_W64) + tab + 3 * prod + 2 * u
    return _chirp_tail(e_conv, n, m, dtype, hartley, inverse)


def composition_rel_bound(n, m, dtype, hartley=False, inverse=False, table_err=None):
    """the same for the three-transform composition of backend._fft_last_axis_any (nk_fftn on (m,) twice, nk_cplx_rows)"""
    u = unit_roundoff(dtype)
    prod = math.sqrt(2.0) * gamma(2, u)
    tab = u if table_err is None else table_err
    e_conv = 2 * c2c_rel_bound((m,), dtype) + 2 * _table_mu(dtype, MU_W64) + tab + 3 * prod
    return _chirp_tail(e_conv, n, m, dtype, hartley, inverse)


def seam_rel_bound(axis_bounds, dtype, separate_scale=False):
    """relative errors of the axis transforms add (every one has norm sqrt n_axis; a Hartley end is part of the last axis'
    own bound), one more SLACK for their cross terms; separate_scale: one more launch that multiplies by scale"""
    return SLACK * sum(axis_bounds) + (unit_roundoff(dtype) if separate_scale else 0.0)


def bluestein_host_tables(n, m, dtype, inverse=False):
    """(w[n], bhat[m] in natural order) in T as backend._bluestein_tables builds them: angles and the filter's transform
    in double on the host, rounded to T"""
    k = np.arange(n, dtype=np.int64)
    ang = (k * k % (2 * n)).astype(np.float64) * (np.pi / n)
    w = np.exp(1j * ang if inverse else -1j * ang)
    b = np.zeros(m, dtype=np.complex128)
    b[:n] = w.conj()
    b[m - n + 1:] = w.conj()[1:][::-1]
    cdt = complex_dtype(dtype)
    return w.astype(cdt), np.fft.fft(b).astype(cdt)


def bluestein_same_precision(x, n, m, w, bhat, scale=1.0, hartley=0):
    """The chirp-z restated with numpy in T = the dtype of the tables, every intermediate cast to T: what a sound
    implementation does.  x: rows x n (real or complex); w[n], bhat[m] (natural order) in T."""
    cdt = w.dtype
    rdt = np.float32 if cdt == np.complex64 else np.float64
    x = np.asarray(x)
    a = np.zeros(x.shape[:-1] + (m,), dtype=cdt)
    a[..., :n] = (x.astype(cdt) * w).astype(cdt)
    A = scipy.fft.fft(a).astype(cdt)
    P = (A * bhat).astype(cdt)
    c = scipy.fft.ifft(P).astype(cdt)
    v = (c[..., :n] * w).astype(cdt)
    if hartley:
        return (rdt(scale) * (v.real + rdt(hartley) * v.imag)).astype(rdt)
    return (v * rdt(scale)).astype(cdt)


def row_errors(got, ref, x, n, scale=1.0):
    """per row: ||got - ref||_2 / (|scale| sqrt n ||x||_2) -- the quantity the chirp-z bounds limit (0 for a zero row that
    comes out as zeros, inf for one that does not)"""
    d = np.abs(np.asarray(got).astype(CLD) - ref) ** 2
    e = np.sqrt(np.sum(d.reshape(-1, n), axis=1).astype(LD))
    nx = np.sqrt(np.sum((np.abs(np.asarray(x).astype(CLD)) ** 2).reshape(-1, n), axis=1).astype(LD)) * LD(abs(scale) * math.sqrt(n))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(nx > 0, e / nx, np.where(e > 0, np.inf, 0.0))
    return np.asarray(r, dtype=np.float64)


def structured_rows(n, dtype, real=False):
    """impulses at 0, n / 2 and n - 1, the constant and one exponential exp(2 pi i q j / n) (real: its cosine), rounded to T"""
    pos = sorted({0, n // 2, n - 1})
    x = np.zeros((len(pos) + 2, n), dtype=np.complex128)
    for r, p in enumerate(pos):
        x[r, p] = 1.0
    x[len(pos)] = 1.0 if real else 1.0 - 0.5j
    q = min(3, n - 1)
    x[len(pos) + 1] = np.exp(2j * np.pi * ((q * np.arange(n)) % n) / n)
    return np.ascontiguousarray(x.real.astype(dtype) if real else x.astype(complex_dtype(dtype)))


# (n, m, only dtype or None): nk_bluestein_rows lengths -- the smallest m, both parities of log2 m, m = 2 n, the LDS limits
# of both dtypes, twice and four times the smallest m
BLUESTEIN_LENGTHS = [(1, 4, None), (2, 4, None), (3, 8, None), (5, 16, None), (11, 32, None), (17, 64, None), (32, 64, None),
                     (33, 128, None), (211, 512, None), (1009, 2048, None), (2048, 4096, None), (4096, 8192, np.float32),
                     (11, 64, None), (11, 128, None)]
BLUESTEIN_ROW_SWEEPS = [(11, 32), (211, 512)]
BLUESTEIN_GRID_STRIDE = (1500, 4096, 2051)  # more than 2048 row groups of R = 1 row
# rejected lengths the array seam is tested at, with the path each takes (per dtype): the hand-over at the 64 KiB row, the
# longest the composition serves (4095: m = 8192, the longest c2c line in fp64; 8191: m = 16384 = the seam's own cap)
SEAM_LENGTHS = {np.dtype(np.float64): [(2047, "one-launch"), (2049, "composition"), (4095, "composition")],
                np.dtype(np.float32): [(4095, "one-launch"), (4097, "composition"), (8191, "composition")]}
SEAM_SHAPES = [(63,), (63, 54), (10, 11), (13, 17, 6)]
