"""Nufft and Gridder on host fields (reference library/nft.py:40-141, test_nft.py): the gridding approximation against direct
sums in both directions, exact adjointness, argument errors, the Cartesian identity, and the spreading plan of the device
kernels (nk_nufft_spread) walked in numpy against the host's spread grid."""
import numpy as np
import pytest

import nifty_amd as ift
from nifty_amd import nufft

EPS = [1e-2, 1e-4, 1e-7, 1e-10, 1e-12, 2e-13]
SHAPES = [((32,), (0.2,)), ((127,), (0.3,)), ((27,), (1.0,)), ((128,), (0.2,)), ((32, 48), (0.2, 1.12)), ((54, 27), (0.5, 2.0)),
          ((128, 128), (0.2, 1.12)), ((10, 27, 32), (0.2, 1.12, 0.7)), ((32, 48, 54), (1.0, 0.3, 0.5))]


def _l2(ref, x):
    return np.sqrt(np.sum(np.abs(ref - x) ** 2) / np.sum(np.abs(ref) ** 2))


def _points(rng, m, dst):
    """m points in inverse units of dst, two of them at 0 and 1e-5 and one outside the principal interval"""
    dst = np.asarray(dst)
    pos = (rng.random((m, len(dst))) - 0.5) / dst
    if m > 2:
        pos[-1] = 0.0
        pos[-2] = 1e-5 / dst
        pos[0] += 3.0 / dst
    return pos


def direct_matrix(shape, dst, pos):
    """E[i..., j] = exp(+2 pi i sum_d k_d dst_d pos_jd), k_d = i_d - N_d // 2"""
    ks = np.meshgrid(*[np.arange(n) - n // 2 for n in shape], indexing="ij")
    phase = sum(k[..., None] * (pos[:, d] * dst[d])[None] for d, k in enumerate(ks))
    return np.exp(2j * np.pi * phase)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape,dst", SHAPES)
@pytest.mark.parametrize("m", [1, 10, 100])
def test_nufft_against_direct_sum(shape, dst, m, eps):
    rng = np.random.default_rng(len(shape) * 1000 + m)
    pos = _points(rng, m, dst)
    op = ift.Nufft(ift.RGSpace(shape, dst), pos, eps)
    e = direct_matrix(shape, dst, pos)
    v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    res = op(ift.makeField(op.domain, v)).asnumpy()
    assert res.dtype == np.float64 and res.shape == shape
    assert _l2((e @ v).real, res) < 10 * eps
    g = rng.standard_normal(shape)
    y = op.adjoint(ift.makeField(op.target, g)).asnumpy()
    assert y.dtype == np.complex128 and y.shape == (m,)
    ref = np.tensordot(g, np.conj(e), axes=(list(range(len(shape))), list(range(len(shape)))))
    assert _l2(ref, y) < 10 * eps


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", [(32, 32), (32, 48), (128, 48), (54, 128)])
@pytest.mark.parametrize("m", [1, 10, 100])
def test_gridder_reaches_eps(shape, m, eps):
    rng = np.random.default_rng(7 + m)
    dst = (0.2, 1.12)
    uv = _points(rng, m, dst)
    op = ift.Gridder(ift.RGSpace(shape, dst), uv=uv, eps=eps)
    e = direct_matrix(shape, dst, uv)
    v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    assert _l2((e @ v).real, op(ift.makeField(op.domain, v)).asnumpy()) < eps
    g = rng.standard_normal(shape)
    ref = np.tensordot(g, np.conj(e), axes=([0, 1], [0, 1]))
    assert _l2(ref, op.adjoint(ift.makeField(op.target, g)).asnumpy()) < eps


@pytest.mark.parametrize("eps", [1e-2, 1e-6, 2e-13])
@pytest.mark.parametrize("space", [ift.RGSpace(128), ift.RGSpace([32, 64]), ift.RGSpace([10, 27, 32]), ift.RGSpace(27)])
def test_exact_adjointness(space, eps):
    rng = np.random.default_rng(3)
    pos = rng.random((100, len(space.shape))) - 0.5
    ift.extra.check_linear_operator(ift.Nufft(space, pos, eps), np.complex128, np.float64, only_r_linear=True, rtol=1e-12,
                                    atol=1e-12)
    if len(space.shape) == 2:
        ift.extra.check_linear_operator(ift.Gridder(space, pos, eps), np.complex128, np.float64, only_r_linear=True,
                                        rtol=1e-12, atol=1e-12)


def test_host_path_in_chunks_of_points(monkeypatch):
    """the host path evaluates the (point, footprint cell) weights a chunk of points at a time: any chunking, same result"""
    rng = np.random.default_rng(5)
    sp = ift.RGSpace((32, 48), (0.3, 0.7))
    pos = rng.random((500, 2)) - 0.5
    v = ift.makeField(ift.UnstructuredDomain(500), rng.standard_normal(500) + 1j * rng.standard_normal(500))
    g = ift.makeField(sp, rng.standard_normal(sp.shape))
    whole = ift.Nufft(sp, pos, 1e-9)
    ref_t, ref_a = whole(v).asnumpy(), whole.adjoint(g).asnumpy()
    monkeypatch.setattr(nufft, "HOST_ENTRIES", 1000)  # 8 points per chunk at w = 11
    small = ift.Nufft(sp, pos, 1e-9)
    assert len(small.plan._host_chunks()) > 50
    np.testing.assert_allclose(small(v).asnumpy(), ref_t, rtol=0, atol=1e-13 * np.abs(ref_t).max())
    np.testing.assert_array_equal(small.adjoint(g).asnumpy(), ref_a)


def test_chunk_length_follows_the_list_lengths():
    """uniform coverage keeps every tile's list whole; a dense core is split"""
    rng = np.random.default_rng(6)
    uniform = nufft.NufftPlan((256, 256), (1.0, 1.0), rng.random((1 << 20, 2)) - 0.5, 1e-6)
    assert uniform.max_list > nufft.CHUNK and uniform.n_slabs == 0 and uniform.chunk >= uniform.max_list
    core = np.concatenate([rng.random((1 << 16, 2)) - 0.5, 0.01 * rng.random((1 << 16, 2))])
    dense = nufft.NufftPlan((256, 256), (1.0, 1.0), core, 1e-6)
    assert dense.n_slabs > 0 and dense.max_list > dense.chunk


def test_argument_errors():
    pos = np.zeros((4, 2))
    with pytest.raises(TypeError):
        ift.Nufft(ift.UnstructuredDomain(5), np.zeros((4, 1)))
    with pytest.raises(ValueError):
        ift.Nufft(ift.RGSpace((4, 4, 4, 4)), np.zeros((4, 4)))
    with pytest.raises(TypeError):
        ift.Nufft(ift.RGSpace((8, 8)), np.zeros(4))
    with pytest.raises(ValueError):
        ift.Gridder(ift.RGSpace((8, 7)), pos)
    with pytest.raises(ValueError):
        ift.Gridder(ift.RGSpace(8), np.zeros((4, 1)))
    with pytest.raises(ValueError):
        ift.Gridder(ift.RGSpace((8, 8, 8)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        ift.Gridder(ift.RGSpace((8, 8)), np.zeros(4))
    with pytest.raises(ValueError):
        ift.Gridder(ift.RGSpace((8, 8)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        ift.Nufft(ift.RGSpace(8), pos, eps=0.0)


def test_cartesian_points_are_the_fft():
    nx, ny = 32, 42
    dom = ift.RGSpace((nx, ny), (0.3, 0.2))
    uu, vv = np.meshgrid(np.fft.fftfreq(nx, 0.3), np.fft.fftfreq(ny, 0.2))
    uv = np.transpose(np.vstack([uu[None, :], vv[None, :]]), (2, 1, 0)).reshape(-1, 2)
    op = ift.Gridder(dom, uv=uv).adjoint
    arr = np.random.default_rng(11).standard_normal(dom.shape)
    res = op(ift.makeField(dom, np.roll(arr, (nx // 2, ny // 2), axis=(0, 1)))).asnumpy().reshape(nx, ny)
    fft = ift.FFTOperator(dom.get_default_codomain(), target=dom).adjoint
    vol = ift.full(dom, 1.0).s_integrate()
    np.testing.assert_allclose(res, fft(ift.makeField(dom, arr)).asnumpy() * vol)


def test_kernel_parameters():
    assert [nufft.kernel_params(e)[0] for e in (1e-2, 1e-4, 1e-6, 1e-7, 1e-10, 1e-12, 2e-13, 1e-16)] == [4, 6, 8, 9, 12, 14, 15, 16]
    assert nufft.kernel_params(1e-6)[1] == pytest.approx(2.30 * 8)
    assert nufft.oversampled_length(27, 9) == 54 and nufft.oversampled_length(127, 9) == 256
    assert nufft.oversampled_length(5, 16) == 32 and nufft.oversampled_length(31, 4) == 63
    w, beta = nufft.kernel_params(1e-8)
    z = np.linspace(-w / 2, w / 2, 200001)
    for xi in (0.0, 0.1, 0.25):
        ref = np.trapezoid(nufft.es_kernel(z, w, beta) * np.cos(2 * np.pi * xi * z), z)
        assert nufft.kernel_ft([xi], w, beta)[0] == pytest.approx(ref, rel=1e-8)


def spread_like_the_device(plan, v):
    """nk_nufft_spread's walk in numpy: for every item the tile's neighbour bins in C order, every cell adds the points
    whose footprint covers it, in list order; split lists through the slabs.  Returns the oversampled grid."""
    nd, w = plan.ndim, plan.w
    grid = np.full(plan.n, np.nan + 0j)
    slabs = np.zeros((plan.n_slabs, 256), dtype=np.complex128)
    for tile, lo, hi, slab in plan.item:
        tc = np.unravel_index(tile, plan.ntiles)
        axes = []
        for d in range(nd):
            span = 2 * plan.reach[d] + 1
            b0 = 0 if span >= plan.ntiles[d] else tc[d] - plan.reach[d]
            axes.append([(b0 + o) % plan.ntiles[d] for o in range(min(span, plan.ntiles[d]))])
        bins = [np.ravel_multi_index(b, plan.ntiles) for b in np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, nd)]
        lst = np.concatenate([np.arange(plan.bin_start[b], plan.bin_start[b + 1]) for b in bins])[lo:hi]
        cells = np.stack(np.meshgrid(*[tc[d] * plan.tile[d] + np.arange(plan.tile[d]) for d in range(nd)], indexing="ij"),
                         -1).reshape(-1, nd)
        acc = np.zeros(256, dtype=np.complex128)
        for s in lst:
            u = plan.u[s]
            l0 = np.ceil(u - 0.5 * w)
            dd = (cells - l0[None, :]) % np.array(plan.n)[None, :]
            ker = np.prod(np.where(dd < w, nufft.es_kernel(l0[None, :] - u[None, :] + dd, w, plan.beta), 0.0), axis=1)
            acc += ker * v[plan.perm[s]]
        inside = np.all(cells < np.array(plan.n)[None, :], axis=1)
        if slab >= 0:
            slabs[slab] = acc
        else:
            grid[tuple(cells[inside].T)] = acc[inside]
    for k, tile in enumerate(plan.split_tile):
        tc = np.unravel_index(tile, plan.ntiles)
        cells = np.stack(np.meshgrid(*[tc[d] * plan.tile[d] + np.arange(plan.tile[d]) for d in range(nd)], indexing="ij"),
                         -1).reshape(-1, nd)
        inside = np.all(cells < np.array(plan.n)[None, :], axis=1)
        grid[tuple(cells[inside].T)] = slabs[plan.split_slab[k]:plan.split_slab[k + 1]].sum(axis=0)[inside]
    return grid


@pytest.mark.parametrize("shape,eps,chunk", [((100,), 1e-6, 8192), ((300,), 1e-12, 7), ((24, 30), 1e-4, 8192),
                                             ((24, 30), 1e-12, 5), ((6, 10, 9), 1e-6, 8192), ((6, 10, 9), 1e-13, 11)])
def test_device_spreading_plan_covers_every_footprint(shape, eps, chunk, monkeypatch):
    """Every cell of the oversampled grid is written once and gets every point whose footprint covers it -- partial tiles,
    wrapping, few tiles per axis, and split lists (a small CHUNK) included."""
    monkeypatch.setattr(nufft, "CHUNK", chunk)
    monkeypatch.setattr(nufft, "CHUNK_MEDIANS", 0)
    rng = np.random.default_rng(2)
    m = 60
    pos = np.concatenate([rng.random((m - 20, len(shape))) - 0.5, 1e-3 * rng.random((20, len(shape)))])
    plan = nufft.NufftPlan(shape, [1.0] * len(shape), pos, eps)
    assert (plan.n_slabs > 0) == (chunk < 100)
    v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    grid = spread_like_the_device(plan, v)
    assert not np.any(np.isnan(grid))
    flat, wgt = plan._host_weights(0, plan.m)
    size = int(np.prod(plan.n))
    ref = (np.bincount(flat.reshape(-1), (wgt * v.real[:, None]).reshape(-1), size)
           + 1j * np.bincount(flat.reshape(-1), (wgt * v.imag[:, None]).reshape(-1), size)).reshape(plan.n)
    np.testing.assert_allclose(grid, ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())


def test_plan_sorts_points_by_tile():
    rng = np.random.default_rng(4)
    plan = nufft.NufftPlan((64, 48), (1.0, 1.0), rng.random((500, 2)) - 0.5, 1e-6)
    assert sorted(plan.perm.tolist()) == list(range(500))
    b = (plan.u // np.array(plan.tile)).astype(int)
    flat = np.ravel_multi_index(tuple(b.T), plan.ntiles)
    assert np.all(np.diff(flat) >= 0)
    assert plan.bin_start[-1] == 500 and np.array_equal(np.bincount(flat, minlength=len(plan.bin_start) - 1), np.diff(plan.bin_start))
    assert np.all(plan.u >= 0) and np.all(plan.u < np.array(plan.n))
