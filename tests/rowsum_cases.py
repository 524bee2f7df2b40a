"""Matrices, data, restatements, long-double references and DERIVED bounds for the sparse and index-movement kernels at the end
of nifty_amd/csrc/nk_vec.hip: nk_csr_rowsum / nk_spmv / nk_csr_rowsum_batch (k_csr_rowsum, k_csr_rowsum_b, k_csr_rowsum_staged),
nk_spmv_t, nk_roll and nk_cumsum (tests/test_rowsum_cases.py on the host, tests/test_rowsum_kernels_gpu.py on the device).
numpy and Python integers only.

Geometry, parsed from the source.  k_csr_rowsum runs workgroups of 256 threads, L = 1, 4, 16 or 64 lanes per row.  The staged
short-row kernel gives a workgroup NkStaged<MB>::ROWS = 256 RPT consecutive rows and walks THEIR entries [e0, e1) in windows of W
entries counted from e0: MB = 1 (single calls) and MB = 4 (batched calls, one grid row per four members).  k_roll runs at most
ROLL_MAX_BLOCKS blocks of ROLL_THREADS threads in a grid-stride loop; k_cumsum is ONE workgroup of CUMSUM_TILE threads =
CUMSUM_TILE / WAVE wavefronts.

Order of a row sum (include/niftyk.h), `rowsum_in_order`.  Lane l starts from 0.0 and adds the entries l, l + L, ... of the row in
ascending order; then the shuffle-down tree off = L/2 ... 1 runs, a[l] += a[l + off] for l < off; lane 0 is the row.  The staged
kernel adds a row's entries in the order of L = 1.

Data kinds.
  exact    integers in x and y, weights k / 4: every product and every partial sum is representable (|sum| < 2^17 quarters), so any
           order gives the same bits and a dropped, doubled or misplaced entry fails deterministically
  ordered  float32-representable values (twelve decades) in an array of the field dtype, float32 weights (four decades): a product
           has at most 48 bits and is exact in fp64, so a fused and an unfused multiply-add agree and `rowsum_in_order` is the
           device's bits whatever the compiler contracts; the sums themselves round, so the ORDER shows
  normal   full-precision normals, float32 normal weights: held to the bound

Bounds.  u = 2^-53, gamma(k) = k u / (1 - k u) (binmap_cases.gamma, Higham section 3.1), long double; + 2^-24 |ref| where the result
is stored as float32 (`store_rounding`).
  row sums   gamma(ceil(len / L) + log2 L + 1) sum |w x| per row.  A term passes 1 rounding of its product (none if fused), at
             most ceil(len / L) additions of its lane (the first, onto 0.0, is exact) and log2 L additions of the tree.
  nk_spmv_t  gamma(m_c + 1) (|x0_c| + sum |terms|) per column, m_c = atomic terms of column c: 1 rounding of the product and m_c
             additions in any order onto the prefill x0_c.
  nk_cumsum  gamma(22 ceil((i + 1) / 1024)) sum_{j <= i} |x_j| per element.  Inside a tile an element passes at most 6 steps of
             the wavefront scan (log2 64), at most 15 additions of `pre` -- carry + wsum[0] + ... + wsum[14] for the last wavefront,
             the carry being the first operand, not an addition of its own -- and the final v + pre: 22.  The carry handed to the
             next tile is thread 1023's v + pre, again 22 deep, so after t whole tiles a term has passed at most 22 (t + 1)
             roundings.  (Counting "15 wave sums and one carry addition" separately gives 23; the kernel's loop makes 15.)
The long-double references themselves carry at most (len + 1) 2^-64 sum |terms| against a bound of at least
(ceil(len / L) + log2 L + 1) 2^-53 sum |terms|: a fraction below 2^-11 (len + 1) / (ceil(len / L) + log2 L + 1) < 2^-11 L, at most
2^-5 = 3 % of the bound (L = 64).
"""
import math
import os
import re

import numpy as np

from tests.binmap_cases import LD, ROOT, U32, U64, VEC_SRC, gamma, worst  # noqa: F401  (re-exported for the tests)

HEADER = open(os.path.join(ROOT, "include", "niftyk.h")).read()

_m = re.search(r"static constexpr int RPT = MB == 1 \? (\d+) : (\d+), W = MB == 1 \? (\d+) : (\d+), ROWS = (\d+) \* RPT;", VEC_SRC)
WG_THREADS = int(_m.group(5))  # threads of a row-sum workgroup
STAGED = {1: {"RPT": int(_m.group(1)), "W": int(_m.group(3)), "ROWS": WG_THREADS * int(_m.group(1))},
          4: {"RPT": int(_m.group(2)), "W": int(_m.group(4)), "ROWS": WG_THREADS * int(_m.group(2))}}
assert "__launch_bounds__(%d) k_csr_rowsum(" % WG_THREADS in VEC_SRC
_m = re.search(r"std::min<int64_t>\(\(total \+ 255\) / (\d+), (\d+) \* (\d+)\)", VEC_SRC)
ROLL_THREADS, ROLL_MAX_BLOCKS = int(_m.group(1)), int(_m.group(2)) * int(_m.group(3))
_CUMSUM_SRC = VEC_SRC[VEC_SRC.index("k_cumsum(int64_t n"):VEC_SRC.index('extern "C" int nk_cumsum')]
CUMSUM_TILE = int(re.search(r"base \+= (\d+)\)", _CUMSUM_SRC).group(1))
WAVE = int(re.search(r"for \(int off = 1; off < (\d+); off <<= 1\)", _CUMSUM_SRC).group(1))
assert "threadIdx.x & %d," % (WAVE - 1) in _CUMSUM_SRC and "wsum[%d]" % (CUMSUM_TILE // WAVE) in _CUMSUM_SRC
NK_MAX_BATCH = int(re.search(r"^#define NK_MAX_BATCH (\d+)$", HEADER, re.M).group(1))

LANES = (1, 4, 16, 64)
DTYPES = (np.float64, np.float32)
KINDS = ("exact", "ordered", "normal")
NCOLS = 97
# every (lanes, weighted, dtype, kind) of the edge matrix: both tests run all of them
ROWSUM_CASES = [(L, w, dt, kind) for L in LANES for w in (True, False) for dt in DTYPES for kind in KINDS]
BATCH_COUNTS = tuple(range(1, NK_MAX_BATCH + 1))
STAGED_BATCH_COUNTS = (1, 3, 4, 5, 8)  # ragged and full slices of four: one and two grid rows
CUMSUM_STEPS = int(math.log2(WAVE)) + (CUMSUM_TILE // WAVE - 1) + 1  # scan + pre + final = 22 per tile


def store_rounding(ref, dtype):
    return (U32 if np.dtype(dtype) == np.float32 else LD(0.0)) * np.abs(ref)


class Csr:
    def __init__(self, name, lengths, ncols, rng, weighted, allowed=None):
        self.name, self.ncols = name, ncols
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.rowptr = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.nrows, self.nnz = len(self.lengths), int(self.rowptr[-1])
        pool = np.arange(ncols) if allowed is None else np.asarray(allowed)
        self.col = pool[rng.integers(0, len(pool), size=self.nnz)].astype(np.int32)  # with repetition
        self.rng, self.weighted = rng, weighted

    def weights(self, kind):
        """float32 weights of the data kind, or None"""
        if not self.weighted:
            return None
        rng = np.random.default_rng([71, self.nnz, KINDS.index(kind)])
        if kind == "exact":
            return (rng.integers(-8, 9, size=self.nnz) / 4.0).astype(np.float32)
        if kind == "ordered":
            return (rng.normal(size=self.nnz) * 10.0 ** rng.uniform(-2, 2, size=self.nnz)).astype(np.float32)
        return rng.normal(size=self.nnz).astype(np.float32)


def operand(kind, n, dtype, seed=0):
    """x (or y of nk_spmv_t) of the data kind"""
    rng = np.random.default_rng([73, n, KINDS.index(kind), seed])
    if kind == "exact":
        return rng.integers(-8, 9, size=n).astype(dtype)
    if kind == "ordered":
        return (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(np.float32).astype(dtype)
    return rng.normal(size=n).astype(dtype)


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def edge_lengths(L):
    nrows = 3 * WG_THREADS // L + 3
    fixed = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 5 * L + 3, 0, 0, 300]
    rng = np.random.default_rng([61, L])
    return fixed + [int(k) for k in rng.integers(0, 3 * L + 2, size=nrows - len(fixed) - 1)] + [L + 2]


def edge_matrix(L, weighted):
    """every row length around the lane count, three workgroups and a ragged fourth, an empty first row, a last row of L + 2"""
    return Csr(f"edge{L}", edge_lengths(L), NCOLS, np.random.default_rng([67, L]), weighted)


STAGED_NAMES = ("a", "b-", "b+", "edge")


def staged_lengths(name, MB):
    """(a) one window exactly in one row, an empty workgroup, a last workgroup of one row of two windows and one entry;
    (b-/b+) ROWS -+ 1 rows of 0..5 entries and one of 3000; (edge) a row that ENDS on a window edge, an empty one behind it, then one
    that straddles the next edge"""
    rows, W = STAGED[MB]["ROWS"], STAGED[MB]["W"]
    rng = np.random.default_rng([79, MB, STAGED_NAMES.index(name)])
    if name == "a":
        lengths = np.zeros(2 * rows + 1, dtype=np.int64)
        lengths[5], lengths[-1] = W, 2 * W + 1
    elif name in ("b-", "b+"):
        lengths = rng.integers(0, 6, size=rows + (1 if name == "b+" else -1))
        lengths[100] = 3000
    else:
        lengths = rng.integers(0, 6, size=rows + 7)
        lengths[:4] = [W - 24, 24, 0, W + W // 2]
    return lengths


def staged_matrix(name, MB, weighted):
    return Csr(f"staged{MB}{name}", staged_lengths(name, MB), NCOLS, np.random.default_rng([83, MB, STAGED_NAMES.index(name)]), weighted)


def staged_windows(rowptr, MB):
    """per workgroup of k_csr_rowsum_staged<T, MB>: (first row, rows, entries, windows)"""
    rows, W = STAGED[MB]["ROWS"], STAGED[MB]["W"]
    nrows = len(rowptr) - 1
    out = []
    for r0 in range(0, nrows, rows):
        r1 = min(r0 + rows, nrows)
        e = int(rowptr[r1] - rowptr[r0])
        out.append((r0, r1 - r0, e, -(-e // W)))
    return out


def rows_on_window_edges(rowptr, MB):
    """(rows that end exactly on an inner window edge of their workgroup, rows that straddle one)"""
    rows, W = STAGED[MB]["ROWS"], STAGED[MB]["W"]
    ends, straddles = [], []
    for r in range(len(rowptr) - 1):
        r0 = r // rows * rows
        e0, e1 = int(rowptr[r0]), int(rowptr[min(r0 + rows, len(rowptr) - 1)])
        lo, hi = int(rowptr[r]) - e0, int(rowptr[r + 1]) - e0
        if hi > lo and hi % W == 0 and hi < e1 - e0:
            ends.append(r)
        if hi > lo and (lo // W) != ((hi - 1) // W):
            straddles.append(r)
    return ends, straddles


# ---- row sums: reference, restatement, bound --------------------------------------------------------------------------------
def terms_of(m, wgt, x, kind=np.float64):
    xv = np.asarray(x).astype(kind)[m.col]
    return xv if wgt is None else np.asarray(wgt).astype(kind) * xv


def rowsum_ld(m, wgt, x):
    """(sum, sum of magnitudes) per row, long double"""
    t = terms_of(m, wgt, x, LD)
    ref, mag = np.zeros(m.nrows, dtype=LD), np.zeros(m.nrows, dtype=LD)
    rows = np.repeat(np.arange(m.nrows), m.lengths)
    np.add.at(ref, rows, t)
    np.add.at(mag, rows, np.abs(t))
    return ref, mag


def rowsum_bound(m, mag, ref, lanes, dtype):
    steps = -(-m.lengths // lanes) + int(math.log2(lanes)) + 1
    return gamma(steps) * mag + store_rounding(ref, dtype)


ROWSUM_FAULTS = ("drop_entry", "drop_tail", "half_tree", "tree_stops_at_2")


def rowsum_in_order(rowptr, col, wgt, x, lanes, mut=None):
    """the documented order in fp64: lane l adds the entries l, l + lanes, ... from 0.0 (np.cumsum adds strictly in sequence), the
    tree off = lanes / 2 ... 1 joins a[l] += a[l + off], lane 0 is the row.  mut: a row loses its last entry / every lane its last
    trip / the tree its first step (the upper half of the lanes) / the tree its last step (off > 1)"""
    xv = np.asarray(x).astype(np.float64)[col]
    t = xv if wgt is None else np.asarray(wgt).astype(np.float64) * xv  # exact for `exact` and `ordered` data
    out = np.zeros(len(rowptr) - 1)
    offs = [o for o in (32, 16, 8, 4, 2, 1) if o < lanes]
    if mut == "half_tree":
        offs = offs[1:]
    if mut == "tree_stops_at_2":
        offs = offs[:-1]
    for r in range(len(out)):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if mut == "drop_entry" and hi > lo:
            hi -= 1
        if mut == "drop_tail" and hi > lo:
            hi = lo + (-(-(hi - lo) // lanes) - 1) * lanes
        a = np.zeros(lanes)
        for l in range(min(lanes, hi - lo)):
            a[l] = np.cumsum(t[lo + l:hi:lanes])[-1]
        for off in offs:
            a[:off] = a[:off] + a[off:2 * off]
        out[r] = a[0]
    return out


# ---- nk_spmv_t ------------------------------------------------------------------------------------------------------------------
SPMV_T_ROWS = (1, 4, 5, 9)
SPMV_T_NCOLS = 50
SPMV_T_UNTOUCHED = (7, 49)
_SPMV_T_LENGTHS = [200, 0, 1, 63, 64, 65, 200, 1, 65]  # one lane, a wavefront less one / exactly / plus one, four trips


def spmv_t_matrix(nrows):
    allowed = [c for c in range(SPMV_T_NCOLS) if c not in SPMV_T_UNTOUCHED]
    return Csr(f"spmvt{nrows}", _SPMV_T_LENGTHS[:nrows], SPMV_T_NCOLS, np.random.default_rng([89, nrows]), True, allowed)


def spmv_t_prefill(nrows):
    return np.random.default_rng([97, nrows]).integers(-5, 6, size=SPMV_T_NCOLS).astype(np.float64)


def spmv_t_reference(m, wgt, y, x0):
    """(ref, bound, m_c): x0 + the column sums of wgt[j] y[row of j], long double"""
    rows = np.repeat(np.arange(m.nrows), m.lengths)
    t = np.asarray(wgt).astype(LD) * np.asarray(y).astype(LD)[rows]
    ref, mag = np.asarray(x0, dtype=LD).copy(), np.abs(np.asarray(x0, dtype=LD))
    np.add.at(ref, m.col, t)
    np.add.at(mag, m.col, np.abs(t))
    mc = np.bincount(m.col, minlength=m.ncols)
    return ref, gamma(mc + 1) * mag, mc


# ---- nk_roll --------------------------------------------------------------------------------------------------------------------
ROLL_DTYPES = (np.float32, np.float64, np.complex64, np.complex128)  # 4, 8, 8 and 16 bytes
ROLL_SHAPES = [(1,), (7,), (256,), (257,), (5, 1, 6), (2, 3, 1, 4, 1, 5), (3, 4, 5, 2, 3, 2)]
ROLL_LONG = (ROLL_MAX_BLOCKS * ROLL_THREADS + 777,)  # the grid-stride loop takes a second trip for 777 elements
_MIXED = (1, -2, 7, 0, -1, 40)


def roll_shifts(shape):
    """zero, FFTShift and its inverse, n - 1, n, 2 n + 1, -3 n - 2 on every axis, and one mixed vector"""
    per_axis = [lambda n: 0, lambda n: n // 2, lambda n: -(n // 2), lambda n: n - 1, lambda n: n, lambda n: 2 * n + 1,
                lambda n: -3 * n - 2]
    return [tuple(f(n) for n in shape) for f in per_axis] + [tuple(_MIXED[d] for d in range(len(shape)))]


def c_rem(a, n):
    """a % n as C computes it: truncation towards zero, the sign of a"""
    assert abs(a) < 1 << 52 and 0 < n < 1 << 52  # exact in fmod's doubles
    return int(math.fmod(a, n))


def reduced_shift(s, n):
    """nk_roll's own arithmetic: ((shift % n) + n) % n with C's %"""
    return c_rem(c_rem(s, n) + n, n)


def roll_payload(shape, dtype):
    """a counter pattern: every element distinct (exact in float32 below 2^24 elements)"""
    total = int(np.prod(shape))
    assert total < 1 << 24
    k = np.arange(1, total + 1, dtype=np.float64)
    if np.dtype(dtype).kind == "c":
        return (k - 1j * (k + 0.5)).astype(dtype).reshape(shape)
    return (k + (0.25 if dtype == np.float64 else 0.0)).astype(dtype).reshape(shape)


def roll_reference(a, shift):
    """out[(i_d + shift_d) mod n_d ...] = in[i ...] from the reduced shifts, as a gather: out[k] = in[(k - shift) mod n]"""
    idx = [(np.arange(n) - reduced_shift(s, n)) % n for n, s in zip(a.shape, shift)]
    return np.ascontiguousarray(a[np.ix_(*idx)])


# ---- nk_cumsum ------------------------------------------------------------------------------------------------------------------
CUMSUM_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)


def cumsum_data(kind, n, dtype):
    rng = np.random.default_rng([101, n, KINDS.index(kind)])
    if kind == "exact":
        return rng.integers(-100, 101, size=n).astype(dtype)  # |sums| <= 5e5 < 2^24
    return rng.normal(size=n).astype(dtype)


def cumsum_exact(x, reverse):
    k = np.asarray(x).astype(np.int64)
    return (np.cumsum(k[::-1])[::-1] if reverse else np.cumsum(k)).astype(np.asarray(x).dtype)


def cumsum_reference(x, reverse, dtype):
    """(ref, bound) per element, long double"""
    v = np.asarray(x).astype(LD)
    if reverse:
        v = v[::-1]
    ref, mag = np.cumsum(v), np.cumsum(np.abs(v))
    tiles = np.arange(len(v)) // CUMSUM_TILE + 1
    bound = gamma(CUMSUM_STEPS * tiles) * mag + store_rounding(ref, dtype)
    return (ref[::-1], bound[::-1]) if reverse else (ref, bound)


def cumsum_in_order(x, reverse, mut=None):
    """k_cumsum addition by addition in fp64, stored in the dtype of x: per tile the shuffle-up scan of every wavefront,
    pre = carry + wsum[0] + ... in sequence, v + pre; the last thread's v + pre is the next carry.  mut `lane_gt_off`: the scan
    tests lane > off"""
    x = np.asarray(x)
    n = len(x)
    src = x[::-1] if reverse else x
    out = np.empty(n, dtype=np.float64)
    waves = CUMSUM_TILE // WAVE
    carry = 0.0
    for base in range(0, n, CUMSUM_TILE):
        v = np.zeros(CUMSUM_TILE)
        k = min(CUMSUM_TILE, n - base)
        v[:k] = src[base:base + k].astype(np.float64)
        v = v.reshape(waves, WAVE)
        off = 1
        while off < WAVE:
            first = off + 1 if mut == "lane_gt_off" else off
            nxt = v.copy()
            nxt[:, first:] = v[:, first:] + v[:, first - off:WAVE - off]
            v = nxt
            off <<= 1
        pre = np.empty(waves)
        p = carry
        for w in range(waves):
            pre[w] = p
            p = p + v[w, WAVE - 1]
        res = (v + pre[:, None]).reshape(-1)
        out[base:base + k] = res[:k]
        carry = res[-1]
    out = out.astype(x.dtype)
    return out[::-1] if reverse else out


def record(kernel, case, dtype, lanes, variant, w):
    """`ERR kernel case dtype lanes variant err bound ratio`"""
    line = "ERR %s %s %s lanes=%s %s err=%.3e bound=%.3e ratio=%.3e" % (kernel, case, np.dtype(dtype).name, lanes, variant,
                                                                       w[1], w[2], w[0])
    print(line)
    return line
