"""Non-uniform FFT: ``Nufft`` and ``Gridder`` (reference library/nft.py:40-141, docs/NUFFT.md).

For a target RGSpace of lengths N_d and distances dst_d, points pos[j] and the centred modes k_d = i_d - N_d // 2:
  TIMES    complex points v -> real grid:  out[i] = Re sum_j v_j exp(+2 pi i sum_d k_d dst_d pos_jd)
  ADJOINT  real grid g -> complex points:  y_j = sum_i g[i] exp(-2 pi i sum_d k_d dst_d pos_jd)
The reference calls ducc0 on the host, for device fields too.  Here both maps are the classic gridding algorithm with an
exponential-of-semicircle kernel (Barnett, Magland, af Klinteberg, SIAM J. Sci. Comput. 41 (2019) C479):
  TIMES    = spread the points onto the oversampled grid -> unscaled backward FFT -> crop the centred modes, divide by the
             kernel's Fourier transform, real part
  ADJOINT  = the exact transpose: divide the modes by the kernel's transform, zero-pad -> forward FFT -> interpolate.
The plan (kernel width, grid, points sorted by tile, correction tables) is made once per operator on the host, like
LOSResponse's matrix.  Device fields run the HIP kernels of nk_nufft.hip and nk_fftn; host fields run the same algorithm
-- the same grid, kernel and correction -- in numpy / scipy.fft, so both compute the same approximation.
"""
import math

import numpy as np
import scipy.fft
import torch

from . import backend as B
from .domains import DomainTuple, RGSpace, UnstructuredDomain
from .field import Field
from .operators import LinearOperator

TILE = {1: (256,), 2: (16, 16), 3: (4, 8, 8)}  # cells of one spreading tile (= one workgroup of 256 threads)
CHUNK = 8192  # shortest chunk of a split point list (nk_nufft_spread slabs) ...
CHUNK_MEDIANS = 2  # ... and the plan's chunk: max(CHUNK, CHUNK_MEDIANS x the median list length of the tiles)
HOST_ENTRIES = 1 << 22  # (point, footprint cell) pairs the host path evaluates at a time
MAX_WIDTH = 16


def kernel_params(eps):
    """(w, beta) of the exponential-of-semicircle kernel for the relative accuracy `eps`."""
    eps = float(eps)
    if not eps > 0.0:
        raise ValueError("eps must be positive")
    w = min(MAX_WIDTH, max(2, int(math.ceil(math.log10(1.0 / eps))) + 2))
    return w, 2.30 * w


def _smooth(n):
    """smallest 2^a 3^b 5^c 7^d >= n"""
    while True:
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def oversampled_length(nmodes, w):
    """length of the oversampled grid of one axis: the smallest 7-smooth number >= max(2 N, 2 w)"""
    return _smooth(max(2 * int(nmodes), 2 * int(w)))


def es_kernel(z, w, beta):
    """phi(z) = exp(beta (sqrt(1 - (2 z / w)^2) - 1)) on |z| <= w / 2"""
    x = np.asarray(z, dtype=np.float64) * (2.0 / w)
    return np.exp(beta * (np.sqrt(np.maximum(1.0 - x * x, 0.0)) - 1.0))


def kernel_ft(xi, w, beta, nodes=128):
    """phi_hat(xi) = int phi(z) exp(2 pi i xi z) dz (phi is even: 2 int_0^{w/2} phi(z) cos(2 pi xi z) dz), Gauss-Legendre"""
    x, wt = np.polynomial.legendre.leggauss(nodes)
    z = (x + 1.0) * (w / 4.0)
    return 2.0 * (w / 4.0) * (np.cos(2.0 * np.pi * np.outer(np.asarray(xi, dtype=np.float64), z)) @ (wt * es_kernel(z, w, beta)))


class NufftPlan:
    """Everything both maps need, made once on the host (numpy arrays; ``nk_nufft_plan`` of include/niftyk.h):
    the kernel (w, beta), the oversampled lengths n, the points in oversampled-grid units u = n frac(dst pos) SORTED by tile
    of the oversampled grid (perm = original index of every sorted point, bin_start = first point of every tile), the work
    items of the spreading pass and the correction tables 1 / phi_hat(k / n).  All of it is a function of the positions: a
    device-side builder (positions as operator inputs) would fill the same arrays."""

    def __init__(self, shape, distances, pos, eps):
        self.nmodes = tuple(int(s) for s in shape)
        self.ndim = nd = len(self.nmodes)
        pos = np.asarray(pos, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != nd:
            raise ValueError(f"positions must have shape (n, {nd}), got {pos.shape}")
        self.eps = float(eps)
        self.w, self.beta = kernel_params(eps)
        self.n = tuple(oversampled_length(s, self.w) for s in self.nmodes)
        self.m = int(pos.shape[0])
        n = np.array(self.n, dtype=np.float64)
        u = np.mod(pos * np.asarray(distances, dtype=np.float64)[None, :], 1.0) * n[None, :]
        self.u_host = np.where(u >= n[None, :], u - n[None, :], u)  # (frac can round up to 1)
        # corrections of the centred modes, axis after axis
        self.corr_axes = [1.0 / kernel_ft((np.arange(N) - N // 2) / nn, self.w, self.beta) for N, nn in zip(self.nmodes, self.n)]
        self.corr = np.concatenate(self.corr_axes)
        self._dev = {}
        self._build_bins()

    def _build_bins(self):
        nd, w = self.ndim, self.w
        self.tile = TILE[nd]
        self.ntiles = tuple(-(-n // t) for n, t in zip(self.n, self.tile))
        self.reach = tuple(-(-w // (2 * t)) + (1 if n % t else 0) for n, t in zip(self.n, self.tile))
        nbins = int(np.prod(self.ntiles))
        b = np.minimum((self.u_host // np.array(self.tile)[None, :]).astype(np.int64), np.array(self.ntiles)[None, :] - 1)
        flat = np.ravel_multi_index(tuple(b.T), self.ntiles) if self.m else np.zeros(0, dtype=np.int64)
        self.perm = np.argsort(flat, kind="stable").astype(np.int64)
        self.u = np.ascontiguousarray(self.u_host[self.perm])
        counts = np.bincount(flat, minlength=nbins).astype(np.int64)
        self.bin_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        # length of every tile's list: its neighbour bins (each once), axis after axis
        lengths = counts.reshape(self.ntiles)
        for d in range(nd):
            if 2 * self.reach[d] + 1 >= self.ntiles[d]:
                lengths = np.broadcast_to(lengths.sum(axis=d, keepdims=True), lengths.shape).copy()
            else:
                lengths = sum(np.roll(lengths, -o, axis=d) for o in range(-self.reach[d], self.reach[d] + 1))
        lengths = lengths.reshape(-1)
        # lists are split where they are long against the typical one: uniform coverage stays unsplit, the dense core of a
        # concentrated one is cut into chunks (a function of the list lengths only)
        self.chunk = chunk = int(max(CHUNK, CHUNK_MEDIANS * np.median(lengths)))
        chunks = np.maximum(1, -(-lengths // chunk))
        item_tile = np.repeat(np.arange(nbins, dtype=np.int64), chunks)
        first = np.concatenate([[0], np.cumsum(chunks)[:-1]])
        ci = np.arange(len(item_tile), dtype=np.int64) - np.repeat(first, chunks)
        lo = ci * chunk
        hi = np.minimum(lo + chunk, lengths[item_tile])
        split = chunks[item_tile] > 1
        slab = np.full(len(item_tile), -1, dtype=np.int64)
        slab[split] = np.arange(int(split.sum()), dtype=np.int64)
        self.item = np.ascontiguousarray(np.stack([item_tile, lo, hi, slab], axis=1).astype(np.int64))
        split_tiles = np.nonzero(chunks > 1)[0]
        self.split_tile = split_tiles.astype(np.int64)
        self.split_slab = np.concatenate([[0], np.cumsum(chunks[split_tiles])]).astype(np.int64)
        self.n_slabs = int(split.sum())
        self.max_list = int(lengths.max()) if len(lengths) else 0

    # ---- host: numpy / scipy.fft -------------------------------------------------------------------------------------
    def _host_weights(self, lo, hi):
        """flat oversampled-grid index and kernel weight of every (point, footprint cell) of the points lo .. hi-1"""
        nd, w = self.ndim, self.w
        t = np.arange(w)
        u = self.u_host[lo:hi]
        flat = wgt = None
        for d in range(nd):
            l0 = np.ceil(u[:, d] - 0.5 * w)
            ker = es_kernel((l0 - u[:, d])[:, None] + t[None, :], w, self.beta)
            idx = (l0.astype(np.int64)[:, None] + t[None, :]) % self.n[d]
            if d == 0:
                flat, wgt = idx, ker
            else:
                flat = (flat[:, :, None] * self.n[d] + idx[:, None, :]).reshape(hi - lo, -1)
                wgt = (wgt[:, :, None] * ker[:, None, :]).reshape(hi - lo, -1)
        return flat, wgt

    def _host_chunks(self):
        """point ranges whose (point, footprint cell) arrays stay near HOST_ENTRIES entries: the host path never holds
        m w^ndim of them"""
        step = max(1, HOST_ENTRIES // self.w ** self.ndim)
        return [(lo, min(lo + step, self.m)) for lo in range(0, self.m, step)]

    def _mode_index(self):
        return np.ix_(*[(np.arange(N) - N // 2) % n for N, n in zip(self.nmodes, self.n)])

    def _corr_outer(self):
        c = self.corr_axes[0]
        for a in self.corr_axes[1:]:
            c = np.multiply.outer(c, a)
        return c

    def times_host(self, v):
        """complex points (numpy [m]) -> real grid (numpy, fp64)"""
        size = int(np.prod(self.n))
        v = np.asarray(v, dtype=np.complex128)
        g = np.zeros(size, dtype=np.complex128)
        for lo, hi in self._host_chunks():
            flat, wgt = self._host_weights(lo, hi)
            g += (np.bincount(flat.reshape(-1), (wgt * v[lo:hi].real[:, None]).reshape(-1), size)
                  + 1j * np.bincount(flat.reshape(-1), (wgt * v[lo:hi].imag[:, None]).reshape(-1), size))
        f = scipy.fft.ifftn(g.reshape(self.n), norm="forward")  # unscaled exp(+2 pi i ...)
        return f[self._mode_index()].real * self._corr_outer()

    def adjoint_host(self, x):
        """real (or complex) grid (numpy) -> complex points (numpy [m], complex128)"""
        g = np.zeros(self.n, dtype=np.complex128)
        g[self._mode_index()] = np.asarray(x) * self._corr_outer()
        f = scipy.fft.fftn(g).reshape(-1)
        y = np.empty(self.m, dtype=np.complex128)
        for lo, hi in self._host_chunks():
            flat, wgt = self._host_weights(lo, hi)
            y[lo:hi] = (f[flat] * wgt).sum(axis=1)
        return y

    # ---- device: nk_nufft.hip + nk_fftn ------------------------------------------------------------------------------
    def device_plan(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = B.NufftDevicePlan(self, device)
        return self._dev[key]

    def times_device(self, v):
        """complex device points [m] -> real device grid, in v's precision"""
        dp = self.device_plan(v.device)
        rdt = torch.float32 if v.dtype == torch.complex64 else torch.float64
        grid = torch.empty(self.n, dtype=v.dtype, device=v.device)
        dp.spread(v.contiguous(), grid)
        f = B.fftn(grid, ndim=self.ndim, inverse=True)
        return dp.crop(f, torch.empty(self.nmodes, dtype=rdt, device=v.device))

    def adjoint_device(self, x):
        """real (or complex) device grid -> complex device points [m], in x's precision"""
        dp = self.device_plan(x.device)
        cdt = torch.complex64 if x.dtype in (torch.float32, torch.complex64) else torch.complex128
        grid = dp.pad(x.contiguous(), torch.empty(self.n, dtype=cdt, device=x.device))
        f = B.fftn(grid, ndim=self.ndim, inverse=False)
        return dp.interp(f, torch.empty(self.m, dtype=cdt, device=x.device))


class Nufft(LinearOperator):
    """Non-uniform FFT between UnstructuredDomain(n) points and a 1-3 axis RGSpace (reference library/nft.py:94-141, same
    arguments).  `pos`: (n, ndim) coordinates; only dst_d * pos_jd modulo 1 matters.  Device fields stay on their device
    and keep their precision (complex64 points / float32 grids compute in single precision with fp64 sums; the reference
    always returns complex128 from the adjoint)."""

    def __init__(self, target, pos, eps=2e-10):
        self._capability = self.TIMES | self.ADJOINT_TIMES
        self._target = DomainTuple.make(target)
        if len(self._target) != 1 or not isinstance(self._target[0], RGSpace):
            raise TypeError("target needs to be an RGSpace")
        if len(self._target.shape) > 3:
            raise ValueError("Only 1D, 2D and 3D FFTs are supported")
        pos = np.asarray(pos)
        if pos.ndim != 2:
            raise TypeError(f"pos needs to be 2d array (got shape {pos.shape})")
        self._domain = DomainTuple.make(UnstructuredDomain(pos.shape[0]))
        sp = self._target[0]
        self._plan = NufftPlan(sp.shape, sp.distances, pos, eps)

    @property
    def plan(self):
        return self._plan

    def apply(self, x, mode):
        self._check_input(x, mode)
        v = x.val
        if mode == self.TIMES:
            if not v.is_complex():
                v = v.to(torch.complex64 if v.dtype == torch.float32 else torch.complex128)
            if v.is_cuda:
                return Field(self._target, self._plan.times_device(v))
            res = self._plan.times_host(v.numpy())
            return Field(self._target, torch.from_numpy(res.astype(np.float32 if v.dtype == torch.complex64 else np.float64)))
        if v.is_cuda:
            return Field(self._domain, self._plan.adjoint_device(v))
        res = self._plan.adjoint_host(v.numpy())
        single = v.dtype in (torch.float32, torch.complex64)
        return Field(self._domain, torch.from_numpy(res.astype(np.complex64 if single else np.complex128)))


class Gridder(Nufft):
    """2-D non-uniform FFT of radio interferometry (reference library/nft.py:40-91, same arguments): `uv` (n, 2) points in
    inverse units of the target's distances.  The same plan and kernels as Nufft."""

    def __init__(self, target, uv, eps=2e-10):
        tgt = DomainTuple.make(target)
        if len(tgt) != 1 or not isinstance(tgt[0], RGSpace) or len(tgt.shape) != 2:
            raise ValueError("need target with exactly one 2D RGSpace")
        if tgt.shape[0] % 2 != 0 or tgt.shape[1] % 2 != 0:
            raise ValueError("even number of pixels is required for gridding operation")
        uv = np.asarray(uv)
        if uv.ndim != 2:
            raise ValueError("uv must be a 2D array")
        if uv.shape[1] != 2:
            raise ValueError("second dimension of uv must have length 2")
        super().__init__(tgt, uv, eps)
