"""Nufft and Gridder on device fields (nk_nufft.hip + nk_fftn): the same approximation as the host path to roundoff, fp32,
bit reproducibility with and without split spreading lists, a large grid spot-checked against direct sums, and a radio
likelihood through the Hamiltonian and optimize_kl on the device."""
import numpy as np
import pytest
import torch

import nifty_amd as ift
from nifty_amd import nufft

from tests.test_nufft import SHAPES, _l2, _points, direct_matrix

pytestmark = pytest.mark.gpu


def _both(op, v, g):
    """TIMES of v and ADJOINT of g on the host and on cuda:0"""
    vf, gf = ift.makeField(op.domain, v), ift.makeField(op.target, g)
    dev_t, dev_a = op(vf.at(0)), op.adjoint(gf.at(0))
    assert dev_t.device_id == 0 and dev_a.device_id == 0
    return op(vf).asnumpy(), dev_t.asnumpy(), op.adjoint(gf).asnumpy(), dev_a.asnumpy()


@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-7, 1e-10, 1e-12, 2e-13])
@pytest.mark.parametrize("shape,dst", SHAPES)
@pytest.mark.parametrize("m", [1, 10, 100])
def test_device_matches_host_and_direct_sum(shape, dst, m, eps):
    rng = np.random.default_rng(len(shape) * 1000 + m)
    pos = _points(rng, m, dst)
    op = ift.Nufft(ift.RGSpace(shape, dst), pos, eps)
    v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    g = rng.standard_normal(shape)
    ht, dt, ha, da = _both(op, v, g)
    assert dt.dtype == np.float64 and da.dtype == np.complex128
    assert _l2(ht, dt) <= 1e-12 and _l2(ha, da) <= 1e-12
    e = direct_matrix(shape, dst, pos)
    assert _l2((e @ v).real, dt) < 10 * eps
    assert _l2(np.tensordot(g, np.conj(e), axes=(list(range(len(shape))), list(range(len(shape))))), da) < 10 * eps
    # exact transposes on the device
    a = float(np.vdot(g, dt).real)
    b = float(np.vdot(da, v).real)
    assert abs(a - b) <= 1e-12 * max(abs(a), np.linalg.norm(g) * np.linalg.norm(v))


@pytest.mark.parametrize("eps", [1e-2, 1e-7, 2e-13])
@pytest.mark.parametrize("shape", [(32, 48), (128, 128)])
def test_gridder_on_the_device(shape, eps):
    rng = np.random.default_rng(9)
    dst = (0.2, 1.12)
    uv = _points(rng, 100, dst)
    op = ift.Gridder(ift.RGSpace(shape, dst), uv=uv, eps=eps)
    v = rng.standard_normal(100) + 1j * rng.standard_normal(100)
    g = rng.standard_normal(shape)
    ht, dt, ha, da = _both(op, v, g)
    e = direct_matrix(shape, dst, uv)
    assert _l2((e @ v).real, dt) < eps and _l2(ht, dt) <= 1e-12 and _l2(ha, da) <= 1e-12
    ift.extra.check_linear_operator(op, np.complex128, np.float64, only_r_linear=True, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-7, 1e-12])
@pytest.mark.parametrize("shape,dst", [((128,), (0.2,)), ((27,), (1.0,)), ((32, 48), (0.2, 1.12)), ((10, 27, 32), (0.2, 1.12, 0.7))])
def test_single_precision(shape, dst, eps):
    rng = np.random.default_rng(21)
    pos = _points(rng, 100, dst)
    op = ift.Nufft(ift.RGSpace(shape, dst), pos, eps)
    v = (rng.standard_normal(100) + 1j * rng.standard_normal(100)).astype(np.complex64)
    g = rng.standard_normal(shape).astype(np.float32)
    dt = op(ift.makeField(op.domain, v).at(0))
    da = op.adjoint(ift.makeField(op.target, g).at(0))
    assert dt.val.dtype == torch.float32 and da.val.dtype == torch.complex64 and dt.device_id == 0
    e = direct_matrix(shape, dst, pos)
    bar = max(10 * eps, 2e-5)
    assert _l2((e @ v.astype(np.complex128)).real, dt.asnumpy()) < bar
    ref = np.tensordot(g.astype(np.float64), np.conj(e), axes=(list(range(len(shape))), list(range(len(shape)))))
    assert _l2(ref, da.asnumpy()) < bar


def _repeat_equal(op, v, g):
    vf, gf = ift.makeField(op.domain, v).at(0), ift.makeField(op.target, g).at(0)
    t1, t2 = op(vf).val, op(vf).val
    a1, a2 = op.adjoint(gf).val, op.adjoint(gf).val
    assert torch.equal(t1, t2) and torch.equal(a1, a2)
    return t1.cpu().numpy(), a1.cpu().numpy()


@pytest.mark.parametrize("kind", ["uniform", "one_tile"])
def test_bit_reproducible_and_split_lists(kind, monkeypatch):
    rng = np.random.default_rng(31)
    shape = (256, 256)
    m = 1 << 16
    if kind == "uniform":
        uv = rng.random((m, 2)) - 0.5
    else:  # every point in the tile of the origin (16 x 16 cells of the 512 x 512 grid)
        uv = rng.random((m, 2)) * (15.0 / 512.0)
    v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    g = rng.standard_normal(shape)
    op = ift.Gridder(ift.RGSpace(shape, (1.0, 1.0)), uv, eps=1e-7)
    if kind == "one_tile":
        assert op.plan.n_slabs > 0 and op.plan.max_list > nufft.CHUNK
    t_split, a_split = _repeat_equal(op, v, g)
    monkeypatch.setattr(nufft, "CHUNK", 1 << 40)
    whole = ift.Gridder(ift.RGSpace(shape, (1.0, 1.0)), uv, eps=1e-7)
    assert whole.plan.n_slabs == 0
    t_whole, a_whole = _repeat_equal(whole, v, g)
    assert _l2(t_whole, t_split) <= 1e-12
    np.testing.assert_array_equal(a_whole, a_split)  # the interpolation does not depend on the split


def test_large_grid_spot_check():
    rng = np.random.default_rng(41)
    shape, m, eps = (1024, 1024), 1 << 22, 1e-6
    uv = rng.random((m, 2)) - 0.5
    op = ift.Gridder(ift.RGSpace(shape, (1.0, 1.0)), uv, eps=eps)
    v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    g = rng.standard_normal(shape)
    dt = op(ift.makeField(op.domain, v).at(0)).asnumpy()
    da = op.adjoint(ift.makeField(op.target, g).at(0)).asnumpy()
    cells = rng.integers(0, 1024, size=(64, 2))
    k = cells - 512
    ref_t = np.array([(v * np.exp(2j * np.pi * (uv @ kk.astype(np.float64)))).real.sum() for kk in k])
    got_t = dt[cells[:, 0], cells[:, 1]]
    assert _l2(ref_t, got_t) < 10 * eps
    pts = rng.integers(0, m, size=64)
    kx, ky = np.meshgrid(np.arange(1024) - 512, np.arange(1024) - 512, indexing="ij")
    ref_a = np.array([np.sum(g * np.exp(-2j * np.pi * (kx * uv[j, 0] + ky * uv[j, 1]))) for j in pts])
    assert _l2(ref_a, da[pts]) < 10 * eps


def _radio_problem():
    rng = np.random.default_rng(51)
    sp = ift.RGSpace((128, 128))
    cf = ift.SimpleCorrelatedField(sp, 0.0, (1e-2, 1e-3), (1.0, 0.5), (1.0, 0.5), (0.5, 0.2), (-3.0, 0.5))
    uv = (rng.random((4096, 2)) - 0.5) * (0.8 * 128)  # in units of 1 / distance: 80 % of the band
    r = ift.Gridder(sp, uv, eps=1e-10).adjoint
    signal = cf
    ift.random.push_sseq_from_seed(52)
    try:
        truth = ift.from_random(signal.domain)
    finally:
        ift.random.pop_sseq()
    clean = r(signal(truth)).asnumpy()
    noise = 0.1 * np.sqrt(np.mean(np.abs(clean) ** 2))
    data = clean + noise * (rng.standard_normal(4096) + 1j * rng.standard_normal(4096))
    return sp, signal, r, data, noise


def _likelihood(signal, r, data, noise, device_id):
    d = ift.makeField(r.target, data)
    d = d if device_id < 0 else d.at(device_id)
    icov = ift.ScalingOperator(r.target, 1.0 / noise ** 2, sampling_dtype=np.complex128)
    return ift.GaussianEnergy(data=d, inverse_covariance=icov) @ (r @ signal)


def test_radio_hamiltonian_on_the_device():
    sp, signal, r, data, noise = _radio_problem()
    vals = {}
    for dev in (-1, 0):
        ham = ift.StandardHamiltonian(_likelihood(signal, r, data, noise, dev))
        x = ift.MultiField.from_dict({k: ift.makeField(d, 0.3 * np.random.default_rng(54 + i).standard_normal(d.shape))
                                      for i, (k, d) in enumerate(sorted(ham.domain.items()))})
        v = ift.MultiField.from_dict({k: ift.makeField(d, np.random.default_rng(64 + i).standard_normal(d.shape))
                                      for i, (k, d) in enumerate(sorted(ham.domain.items()))})
        if dev >= 0:
            x, v = x.at(dev), v.at(dev)
        lin = ham(ift.Linearization.make_var(x, want_metric=True))
        vals[dev] = (float(np.real(lin.val.asnumpy())), lin.gradient.asnumpy(), lin.metric(v).asnumpy())
        if dev >= 0:
            assert lin.gradient.device_id == dev
    (hv, hg, hm), (dv, dg, dm) = vals[-1], vals[0]
    assert abs(hv - dv) <= 1e-10 * abs(hv)
    for k in hg:
        assert _l2(hg[k], dg[k]) <= 1e-10 and _l2(hm[k], dm[k]) <= 1e-10


def _lognormal_field(sp):
    """a 2-D log-normal correlated field with a fixed power spectrum: exp(HT(A xi)), A = sqrt(P(|k|)) scaled to unit
    standard deviation of the log-field.  Every device sum of its Jacobian and adjoint is fixed-order (Hartley passes,
    diagonals), so with the NUFFT the whole optimize_kl run is bit-reproducible."""
    h = sp.get_default_codomain()
    ht = ift.HarmonicTransformOperator(h, sp)
    k = h.get_k_length_array().asnumpy()
    amp = 1.0 / (1.0 + (k / 8.0) ** 2)
    xi = np.random.default_rng(8).standard_normal(h.shape)
    scale = 1.0 / np.std(ht(ift.makeField(h, amp * xi)).asnumpy())
    return (ht @ ift.makeOp(ift.makeField(h, scale * amp)) @ ift.FieldAdapter(h, "xi")).exp()


def _okl(lh, dev):
    ift.random.push_sseq_from_seed(71)
    try:
        ic_s = ift.AbsDeltaEnergyController(deltaE=0.0, iteration_limit=10)
        mk = lambda i: ift.NewtonCG(ift.AbsDeltaEnergyController(0.0, iteration_limit=2), max_cg_iterations=8)  # noqa: E731
        return ift.optimize_kl(lh, 1, 1, mk, ic_s, output_directory=None, return_final_position=True, device_id=dev,
                               fuse=False)
    finally:
        ift.random.pop_sseq()


def test_radio_optimize_kl_on_the_device():
    """One optimize_kl iteration (2 mirrored samples, CG and NewtonCG bounded by iteration counts) of a log-normal field
    seen through Gridder(...).adjoint with a complex Gaussian likelihood: the whole run stays on cuda:0, two device runs
    give the same bits, and the KL matches the host run to 1e-6."""
    rng = np.random.default_rng(61)
    sp = ift.RGSpace((128, 128))
    signal = _lognormal_field(sp)
    uv = (rng.random((4096, 2)) - 0.5) * (0.8 * 128)
    r = ift.Gridder(sp, uv, eps=1e-10).adjoint
    ift.random.push_sseq_from_seed(62)
    try:
        truth = ift.from_random(signal.domain)
    finally:
        ift.random.pop_sseq()
    clean = r(signal(truth)).asnumpy()
    noise = 0.3 * np.sqrt(np.mean(np.abs(clean) ** 2))
    data = clean + noise * (rng.standard_normal(4096) + 1j * rng.standard_normal(4096))
    runs, kl_vals = [], {}
    for dev in (-1, 0, 0):
        lh = _likelihood(signal, r, data, noise, dev)
        sl, mean = _okl(lh, dev)
        samples = list(sl.iterator())
        assert len(samples) == 2
        if dev >= 0:
            assert mean.device_id == dev and all(s.device_id == dev for s in samples)
            runs.append([mean.val["xi"]] + [s.val["xi"] for s in samples])
        ham = ift.StandardHamiltonian(lh)
        kl_vals.setdefault(dev, []).append(sum(float(np.real(ham(s).asnumpy())) for s in samples) / len(samples))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert kl_vals[0][0] == kl_vals[0][1]
    assert abs(kl_vals[0][0] - kl_vals[-1][0]) <= 1e-6 * abs(kl_vals[-1][0])
