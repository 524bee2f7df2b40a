"""tests/rowsum_cases.py held to itself on the host: the restatements stay inside their own bounds, the bounds are tight enough
that a dropped entry, a dropped lane tail or half a shuffle tree breaks them (and the bits of exact and ordered data), the staged
matrices have the window properties they claim, the roll reference is np.roll, and the constants parsed from nk_vec.hip are the ones
the cases were laid out for.  No GPU.  Every case the module lists is run: nothing is filtered."""
import numpy as np
import pytest

from tests import rowsum_cases as rc

LD = rc.LD
RATIOS = {}  # (lanes, weighted, dtype name, kind) -> the restatement's worst err / bound


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_parsed_constants_and_case_lists():
    assert rc.STAGED == {1: {"RPT": 4, "W": 2048, "ROWS": 1024}, 4: {"RPT": 1, "W": 1024, "ROWS": 256}}
    assert (rc.WG_THREADS, rc.ROLL_THREADS, rc.ROLL_MAX_BLOCKS) == (256, 256, 256 * 64)
    assert (rc.CUMSUM_TILE, rc.WAVE, rc.CUMSUM_STEPS, rc.NK_MAX_BATCH) == (1024, 64, 22, 8)
    assert len(rc.ROWSUM_CASES) == len(set(rc.ROWSUM_CASES)) == 4 * 2 * 2 * 3
    assert rc.ROLL_LONG == (256 * 64 * 256 + 777,) and 4 * rc.ROLL_LONG[0] < 17 << 20
    assert [np.dtype(d).itemsize for d in rc.ROLL_DTYPES] == [4, 8, 8, 16]


@pytest.mark.parametrize("L", rc.LANES)
def test_edge_matrix_has_the_stated_rows(L):
    m = rc.edge_matrix(L, True)
    assert m.nrows == {1: 771, 4: 195, 16: 51, 64: 15}[L] == 3 * 256 // L + 3
    assert m.nrows * L > 3 * 256 and (m.nrows * L) % 256 != 0      # three workgroups and a ragged one: lanes of rows >= nrows
    assert m.lengths[0] == 0 and m.lengths[-1] == L + 2
    assert list(m.lengths[:12]) == [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 5 * L + 3, 0, 0, 300]
    assert m.lengths[12:-1].min() >= 0 and m.lengths[12:-1].max() <= 3 * L + 1
    assert 1000 < m.nnz < 2500 and m.col.min() >= 0 and m.col.max() < rc.NCOLS == 97
    assert len(np.unique(m.col)) < m.nnz                            # columns repeat
    assert m.weights("normal").dtype == np.float32 and rc.edge_matrix(L, False).weights("normal") is None
    assert np.array_equal(m.rowptr, rc.edge_matrix(L, False).rowptr)


def _row_medians(m, t):
    return np.array([np.median(np.abs(t[m.rowptr[r]:m.rowptr[r + 1]])) if m.lengths[r] else np.inf for r in range(m.nrows)])


def _check_matrix(m, L, dtype, kind, key=None):
    """the restatement against the long-double reference and its bound; the three faults break the bound (normal) or the bits"""
    wgt, x = m.weights(kind), rc.operand(kind, m.ncols, dtype)
    ref, mag = rc.rowsum_ld(m, wgt, x)
    bound = rc.rowsum_bound(m, mag, ref, L, dtype)
    want = rc.rowsum_in_order(m.rowptr, m.col, wgt, x, L).astype(dtype)
    w = rc.worst(want, ref, bound)
    assert w[0] <= 1, (m.name, kind, w)
    if key is not None:
        RATIOS[key] = w[0]
    if kind == "exact":  # any order gives the exact sum
        assert np.array_equal(want.astype(LD), ref) and not mag[m.lengths == 0].any()
    if kind == "normal":  # the bound is tight: one missing term of typical size breaks it, in every row
        full = rc.rowsum_bound(m, mag, ref, L, np.float64)
        has = m.lengths > 0
        assert (full[has] < _row_medians(m, rc.terms_of(m, wgt, x))[has]).all(), (m.name, float(full.max()))
    faults = rc.ROWSUM_FAULTS if L > 1 else ("drop_entry", "drop_tail")  # one lane has no tree
    for mut in faults:
        bad = rc.rowsum_in_order(m.rowptr, m.col, wgt, x, L, mut).astype(dtype)
        if kind == "normal":
            assert rc.worst(bad, ref, bound)[0] > 1, (m.name, mut)
        else:
            assert not np.array_equal(bits(bad), bits(want)), (m.name, kind, mut)
    return w


@pytest.mark.parametrize("L,weighted,dtype,kind", rc.ROWSUM_CASES,
                         ids=[f"L{L}-{'w' if w else 'u'}-{np.dtype(d).name}-{k}" for L, w, d, k in rc.ROWSUM_CASES])
def test_edge_restatement_inside_its_bound_and_faults_outside(L, weighted, dtype, kind):
    _check_matrix(rc.edge_matrix(L, weighted), L, dtype, kind, key=(L, weighted, np.dtype(dtype).name, kind))


def test_every_edge_case_ran_and_the_bound_is_within_a_decade_of_the_restatement():
    """(runs after the parametrised test above: same module, file order).  The largest err / bound of the restatement itself: a
    bound ten times looser would put it below 0.1 -- short weighted rows (one product rounding u |t| against gamma(3) |t|) and the
    float32 store (up to 2^-24 |ref| against just that) come close to theirs."""
    if len(RATIOS) != len(rc.ROWSUM_CASES):  # run alone: fill the table here
        for L, weighted, dtype, kind in rc.ROWSUM_CASES:
            _check_matrix(rc.edge_matrix(L, weighted), L, dtype, kind, key=(L, weighted, np.dtype(dtype).name, kind))
    assert set(RATIOS) == {(L, w, np.dtype(d).name, k) for L, w, d, k in rc.ROWSUM_CASES}
    for dt in ("float64", "float32"):
        for kind in ("ordered", "normal"):
            top = max(v for (L, w, d, k), v in RATIOS.items() if d == dt and k == kind)
            print(f"HOST rowsum {dt} {kind} worst ratio {top:.3f}")
            assert 0.1 <= top <= 1, (dt, kind, top)


@pytest.mark.parametrize("weighted", [True, False], ids=["w", "u"])
@pytest.mark.parametrize("MB", [1, 4])
@pytest.mark.parametrize("name", rc.STAGED_NAMES)
def test_staged_matrices_have_their_window_properties(name, MB, weighted):
    rows, W = rc.STAGED[MB]["ROWS"], rc.STAGED[MB]["W"]
    m = rc.staged_matrix(name, MB, weighted)
    wg = rc.staged_windows(m.rowptr, MB)
    ends, straddles = rc.rows_on_window_edges(m.rowptr, MB)
    if name == "a":
        assert m.nrows == 2 * rows + 1 and len(wg) == 3
        assert wg[0][2:] == (W, 1) and m.lengths[:rows].max() == W      # exactly one window, all of it in one row
        assert wg[1][1:] == (rows, 0, 0)                                # a workgroup whose rows are all empty
        assert wg[2][1:] == (1, 2 * W + 1, 3) and m.lengths[-1] == 2 * W + 1
    elif name in ("b-", "b+"):
        assert m.nrows == rows + (1 if name == "b+" else -1) and len(wg) == (2 if name == "b+" else 1)
        assert m.lengths[100] == 3000 and 100 in straddles and np.delete(m.lengths, 100).max() <= 5
        assert wg[-1][1] == (1 if name == "b+" else rows - 1)
    else:
        assert 1 in ends and m.lengths[2] == 0 and 3 in straddles
        assert m.rowptr[2] == W and m.rowptr[4] > 2 * W > m.rowptr[3]
        assert len(wg) == 2 and wg[1][1] == 7
    for dtype in rc.DTYPES:
        for kind in rc.KINDS:
            _check_matrix(m, 1, dtype, kind)


@pytest.mark.parametrize("weighted", [True, False], ids=["w", "u"])
def test_one_lane_restatement_is_the_fused_multiply_add_chain(weighted):
    """on ordered data every product is exact, so rounding the product first or not at all is the same chain"""
    from tests.test_los_response import _fma_rowsum

    for m in (rc.edge_matrix(1, weighted), rc.staged_matrix("b+", 1, weighted)):
        wgt = m.weights("ordered")
        for dtype in rc.DTYPES:
            x = rc.operand("ordered", m.ncols, dtype)
            assert np.array_equal(x.astype(np.float32).astype(dtype), x)
            got = rc.rowsum_in_order(m.rowptr, m.col, wgt, x, 1)
            assert np.array_equal(bits(got), bits(_fma_rowsum(m.rowptr, m.col, wgt, x.astype(np.float64))))
    # and the order shows on this data: another lane count gives other bits
    m = rc.edge_matrix(4, weighted)
    x = rc.operand("ordered", m.ncols, np.float64)
    assert not np.array_equal(rc.rowsum_in_order(m.rowptr, m.col, m.weights("ordered"), x, 4),
                              rc.rowsum_in_order(m.rowptr, m.col, m.weights("ordered"), x, 1))


@pytest.mark.parametrize("nrows", rc.SPMV_T_ROWS)
def test_spmv_t_reference_bounds_a_sequential_scatter(nrows):
    m = rc.spmv_t_matrix(nrows)
    assert (nrows + 3) // 4 == {1: 1, 4: 1, 5: 2, 9: 3}[nrows] and set(m.lengths) <= {0, 1, 63, 64, 65, 200}
    assert not np.isin(m.col, rc.SPMV_T_UNTOUCHED).any() and m.col.max() < rc.SPMV_T_NCOLS == 50
    x0 = rc.spmv_t_prefill(nrows)
    rows = np.repeat(np.arange(m.nrows), m.lengths)
    for dtype in rc.DTYPES:
        for kind in ("exact", "normal"):
            wgt, y = m.weights(kind), rc.operand(kind, nrows, dtype)
            ref, bound, mc = rc.spmv_t_reference(m, wgt, y, x0)
            assert mc.sum() == m.nnz and not mc[list(rc.SPMV_T_UNTOUCHED)].any() and mc.max() > 1  # columns collide
            for order in (np.arange(m.nnz), np.arange(m.nnz)[::-1]):
                got = x0.copy()
                for j in order:
                    got[m.col[j]] += float(wgt[j]) * float(y[rows[j]])
                assert rc.worst(got, ref, bound)[0] <= 1
                if kind == "exact":
                    assert np.array_equal(got.astype(LD), ref)
            lost = x0.copy()  # the last entry of every row never arrives
            for j in np.setdiff1d(np.arange(m.nnz), m.rowptr[1:][m.lengths > 0] - 1):
                lost[m.col[j]] += float(wgt[j]) * float(y[rows[j]])
            if kind == "normal":
                assert rc.worst(lost, ref, bound)[0] > 1


def test_roll_reference_is_numpy_roll_for_every_case():
    seen = 0
    for shape in rc.ROLL_SHAPES + [(40000,)]:
        shifts = rc.roll_shifts(shape)
        assert len(shifts) == 8 and shifts[0] == (0,) * len(shape)
        for shift in shifts:
            for s, n in zip(shift, shape):
                assert rc.reduced_shift(s, n) == s % n and 0 <= rc.reduced_shift(s, n) < n
            for dtype in rc.ROLL_DTYPES:
                a = rc.roll_payload(shape, dtype)
                assert len(np.unique(a)) == a.size and a.dtype == dtype
                want = np.roll(a, shift, axis=tuple(range(len(shape))))
                assert np.array_equal(rc.roll_reference(a, shift), want)
                seen += 1
    assert seen == 8 * 8 * 4
    assert rc.c_rem(-7, 3) == -1 and rc.c_rem(7, 3) == 1 and rc.reduced_shift(-7, 3) == 2  # C's remainder keeps the sign
    a = rc.roll_payload(rc.ROLL_LONG, np.float32)
    assert len(np.unique(a)) == a.size
    assert np.array_equal(rc.roll_reference(a, (12345,)), np.roll(a, 12345))


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", rc.CUMSUM_N)
def test_cumsum_restatement_inside_its_bound(n, dtype):
    for reverse in (0, 1):
        x = rc.cumsum_data("exact", n, dtype)
        want = rc.cumsum_exact(x, reverse)
        assert np.abs(want).max() < 1 << 24
        assert np.array_equal(bits(rc.cumsum_in_order(x, reverse)), bits(want))
        assert np.array_equal(want[::-1] if reverse else want, np.cumsum(x[::-1] if reverse else x, dtype=np.float64).astype(dtype))
        x = rc.cumsum_data("normal", n, dtype)
        ref, bound = rc.cumsum_reference(x, reverse, dtype)
        got = rc.cumsum_in_order(x, reverse)
        assert rc.worst(got, ref, bound)[0] <= 1
        if n >= 3:  # lane > off loses lane `off` of every step: elements 1, 2, 4, ... of a wavefront miss their neighbour
            bad = rc.cumsum_in_order(x, reverse, mut="lane_gt_off")
            assert rc.worst(bad, ref, bound)[0] > 1
            xe = rc.cumsum_data("exact", n, dtype)
            assert not np.array_equal(rc.cumsum_in_order(xe, reverse, mut="lane_gt_off"), rc.cumsum_exact(xe, reverse))
        if n > 1:  # the bound is tight: below the median term wherever a term could go missing
            b64 = rc.cumsum_reference(x, reverse, np.float64)[1]
            assert b64.max() < np.median(np.abs(x.astype(np.float64)))
