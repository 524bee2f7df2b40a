"""``LinearInterpolator`` and ``RegriddingOperator`` (reference operators/linear_interpolation.py,
operators/regridding_operator.py; docs/SAMPLING.md): a field on an RGSpace read at arbitrary positions, or on a coarser grid.

Both are sparse linear maps with 2^d entries per output.  The reference writes the interpolation matrix down (scipy coo)
and walks the regridding axes with fancy indexing; here the weights are products of d numbers that are formed where they
are used.  The plans are made once per operator on the host in fp64, exactly as the reference defines them; device fields
run the HIP kernels of nk_sample.hip (matrix-free, no float atomics, bit-reproducible), host fields run the same sums in
numpy.  Sums are fp64 and the result keeps the input's precision (the reference returns fp64) -- the Nufft convention.
"""
import numpy as np
import torch

from . import backend as B
from .domains import DomainTuple, RGSpace, UnstructuredDomain
from .field import Field
from .operators import LinearOperator, _space_index

LONG_CELL = 128  # NK_SAMPLE_LONG of nk_sample.h: an occupied cell with more points is summed by a whole workgroup
MAX_DEVICE_AXES = 3


def _np_result(res, like):
    """numpy fp64 / complex128 result -> host tensor in the precision of the input tensor `like`"""
    single = like.dtype in (torch.float32, torch.complex64)
    if np.iscomplexobj(res):
        return torch.from_numpy(np.ascontiguousarray(res.astype(np.complex64 if single else np.complex128)))
    return torch.from_numpy(np.ascontiguousarray(res.astype(np.float32 if single else np.float64)))


class InterpolationPlan:
    """Multilinear interpolation of `sampling_points` (ndim, npoints) on the periodic grid `shape` with `distances`:
      pos = sampling_points / distances, cell = floor(pos), e = pos - cell (fp64, as the reference computes them);
      corner m in {0, 1}^ndim (C order) of a point is the grid point (cell_a + m_a) mod N_a, weight prod_a (m_a ? e_a : 1 - e_a).
    Host arrays in the caller's order (`cell_axes`, `e`) serve host fields.  The device plan (``nk_sample_plan`` of
    include/niftyk.h) lists the points SORTED stably by base cell: `cell` (flat base cell), `frac` (npoints, ndim), `perm`
    (original index of every sorted point), `cell_start` (first sorted point of every occupied cell) and `long_cell` (the
    occupied cells with more than LONG_CELL points): 8 ndim + 24 bytes per point at most and nothing per grid cell."""

    def __init__(self, shape, distances, sampling_points):
        self.shape = tuple(int(s) for s in shape)
        self.ndim = nd = len(self.shape)
        pts = np.asarray(sampling_points, dtype=np.float64)
        self.npoints = int(pts.shape[1])
        pos = pts / np.asarray(distances, dtype=np.float64).reshape(-1, 1)
        low = np.floor(pos)
        self.e = pos - low
        self.cell_axes = low.astype(np.int64) % np.asarray(self.shape, dtype=np.int64).reshape(-1, 1)
        self.size = int(np.prod(self.shape))
        flat = np.ravel_multi_index(tuple(self.cell_axes), self.shape) if self.npoints else np.zeros(0, dtype=np.int64)
        self.perm = np.argsort(flat, kind="stable").astype(np.int64)
        self.cell = np.ascontiguousarray(flat[self.perm]).astype(np.int64)
        self.frac = np.ascontiguousarray(self.e[:, self.perm].T)
        edges = np.flatnonzero(np.diff(self.cell)) + 1
        self.cell_start = (np.concatenate([[0], edges, [self.npoints]]) if self.npoints else np.zeros(1)).astype(np.int64)
        self.long_cell = np.flatnonzero(np.diff(self.cell_start) > LONG_CELL).astype(np.int64)
        self._dev = {}
        assert self.frac.shape == (self.npoints, nd)

    @property
    def nbytes(self):
        """bytes of the device plan"""
        return sum(getattr(self, k).nbytes for k in B.SampleDevicePlan._keys)

    # ---- host: numpy, the kernels' operations in the kernels' order per output ---------------------------------------
    def corner(self, m):
        """flat grid index and weight of corner m (bit of axis a = (m >> (ndim - 1 - a)) & 1) of every point"""
        idx = wgt = None
        for a, n in enumerate(self.shape):
            bit = (m >> (self.ndim - 1 - a)) & 1
            i = (self.cell_axes[a] + bit) % n
            f = self.e[a] if bit else 1.0 - self.e[a]
            idx, wgt = (i, f) if a == 0 else (idx * n + i, wgt * f)
        return idx, wgt

    def times_host(self, x):
        """grid (numpy, real or complex) -> points (fp64 / complex128)"""
        xf = np.asarray(x).reshape(-1)
        xf = xf.astype(np.complex128 if np.iscomplexobj(xf) else np.float64)
        acc = np.zeros(self.npoints, dtype=xf.dtype)
        for m in range(1 << self.ndim):
            idx, wgt = self.corner(m)
            acc += wgt * xf[idx]
        return acc

    def adjoint_host(self, y):
        """points (numpy, real or complex) -> grid (fp64 / complex128)"""
        y = np.asarray(y)
        planes = [y.real, y.imag] if np.iscomplexobj(y) else [y]
        acc = [np.zeros(self.size) for _ in planes]
        for m in range(1 << self.ndim):
            idx, wgt = self.corner(m)
            for a, p in zip(acc, planes):
                a += np.bincount(idx, wgt * p.astype(np.float64), self.size)
        res = acc[0] + 1j * acc[1] if len(acc) == 2 else acc[0]
        return res.reshape(self.shape)

    # ---- device: nk_sample.hip ---------------------------------------------------------------------------------------
    def device_plan(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = B.SampleDevicePlan(self, device)
        return self._dev[key]


class LinearInterpolator(LinearOperator):
    """Multilinear interpolation of a field on one or several RGSpaces at `sampling_points`, a numpy array of shape
    (total number of grid axes, npoints) in physical units (reference operators/linear_interpolation.py:32-125, same
    arguments and errors).  Positions outside the box wrap periodically.  Host fields take any number of axes; device
    fields 1 to 3.  The result keeps the input's precision (the reference returns fp64)."""

    def __init__(self, domain, sampling_points):
        self._domain = DomainTuple.make(domain)
        for dom in self._domain:
            if not isinstance(dom, RGSpace):
                raise TypeError("LinearInterpolator needs RGSpaces")
        dims = [len(dom.shape) for dom in self._domain]
        if dims.count(dims[0]) != len(dims):
            raise TypeError("all spaces of the domain need the same number of axes")
        if not (isinstance(sampling_points, np.ndarray) and sampling_points.ndim == 2):
            raise TypeError("sampling_points needs to be a numpy array of shape (ndim, npoints)")
        if sampling_points.shape[0] != sum(dims):
            raise TypeError(f"sampling_points needs {sum(dims)} rows, got {sampling_points.shape[0]}")
        self._target = DomainTuple.make(UnstructuredDomain(sampling_points.shape[1]))
        self._capability = self.TIMES | self.ADJOINT_TIMES
        distances = [d for dom in self._domain for d in dom.distances]
        self._plan = InterpolationPlan(self._domain.shape, distances, sampling_points)

    @property
    def plan(self):
        return self._plan

    def _device(self, v, mode):
        if self._plan.ndim > MAX_DEVICE_AXES:
            raise NotImplementedError(f"LinearInterpolator on device fields serves 1 to {MAX_DEVICE_AXES} grid axes, this "
                                      f"domain has {self._plan.ndim}; host fields take any number")
        dp = self._plan.device_plan(v.device)
        run = dp.times if mode == self.TIMES else dp.adjoint
        if v.is_complex():  # the real kernels on the real and imaginary planes
            return torch.complex(run(v.real.contiguous()), run(v.imag.contiguous()))
        return run(v.contiguous())

    def apply(self, x, mode):
        self._check_input(x, mode)
        v = x.val
        if v.is_cuda:
            return Field(self._tgt(mode), self._device(v, mode))
        res = self._plan.times_host(v.numpy()) if mode == self.TIMES else self._plan.adjoint_host(v.numpy())
        return Field(self._tgt(mode), _np_result(res, v))


class RegriddingOperator(LinearOperator):
    """Linear interpolation of domain[space], an RGSpace, onto a grid of `new_shape` with no more points per axis and the
    same total lengths (reference operators/regridding_operator.py:28-103, same arguments and errors).  Axis by axis,
    without wrap: new[j] = old[b_j] (1 - f_j) + old[b_j + 1] f_j with tmp = j newdist / dist, b_j = min(N - 2, int(tmp)),
    f_j = tmp - b_j (f can exceed 1 at the clamped end).  An axis of old length 1 (the reference's adjoint raises there)
    is the identity in both directions.  The result keeps the input's precision (the reference returns fp64)."""

    def __init__(self, domain, new_shape, space=0):
        self._domain = DomainTuple.make(domain)
        self._space = _space_index(self._domain, space)
        dom = self._domain[self._space]
        if not isinstance(dom, RGSpace):
            raise TypeError("RGSpace required")
        new_shape = tuple(new_shape)
        if len(new_shape) != len(dom.shape):
            raise ValueError("Shape mismatch")
        if any(a > b for a, b in zip(new_shape, dom.shape)):
            raise ValueError("New shape must not be larger than old shape")
        if any(ii <= 0 for ii in new_shape):
            raise ValueError("New shape must not be zero or negative.")
        newdist = tuple(dom.distances[i] * dom.shape[i] / new_shape[i] for i in range(len(dom.shape)))
        tgt = list(self._domain)
        tgt[self._space] = RGSpace(new_shape, newdist)
        self._target = DomainTuple.make(tgt)
        self._capability = self.TIMES | self.ADJOINT_TIMES
        self._bindex, self._frac, self._rstart = [], [], []
        for d in range(len(new_shape)):
            tmp = np.arange(new_shape[d]) * (newdist[d] / dom.distances[d])
            b = np.minimum(dom.shape[d] - 2, tmp.astype(np.int64))
            self._bindex.append(b)
            self._frac.append(tmp - b)
            # b is non-decreasing: rstart[i] = first new index whose b is >= i (the adjoint's contiguous ranges)
            self._rstart.append(np.searchsorted(b, np.arange(dom.shape[d] + 1), side="left").astype(np.int64))
        self._dev = {}

    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            up = lambda arrs: [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrs]  # noqa: E731
            self._dev[key] = (up(self._bindex), up(self._frac), up(self._rstart))
        return self._dev[key]

    def _axes(self):
        """(axis of the field, index into the tables) of every axis that is not the identity"""
        axes = self._target.axes[self._space]
        return [(d, d - axes[0]) for d in axes if self._domain.shape[d] > 1]

    def _device(self, v, mode):
        adjoint = mode != self.TIMES
        bindex, frac, rstart = self._tables(v.device)
        final = torch.float32 if v.dtype in (torch.float32, torch.complex64) else torch.float64
        cur = torch.view_as_real(v.contiguous()) if v.is_complex() else v.contiguous()
        planes = 2 if v.is_complex() else 1
        shp = list(v.shape)
        todo = self._axes()
        if not todo:
            return v.clone()
        for k, (d, t) in enumerate(todo):
            n_out = (self._domain if adjoint else self._target).shape[d]
            outer, inner = int(np.prod(shp[:d])), int(np.prod(shp[d + 1:])) * planes
            cur = B.regrid_axis(cur, outer, shp[d], n_out, inner, rstart[t] if adjoint else bindex[t], frac[t],
                                final if k == len(todo) - 1 else torch.float64, adjoint)  # fp64 between axes: rounded once
            shp[d] = n_out
        return torch.view_as_complex(cur.reshape(shp + [2])) if planes == 2 else cur.reshape(shp)

    def _host(self, v, mode):
        v = v.astype(np.complex128 if np.iscomplexobj(v) else np.float64)
        ndim = v.ndim
        for d, t in self._axes():
            b = self._bindex[t]
            wgt = self._frac[t].reshape((1,) * d + (-1,) + (1,) * (ndim - d - 1))
            idx = (slice(None),) * d
            if mode == self.TIMES:
                xnew = v[idx + (b,)] * (1.0 - wgt)
                xnew += v[idx + (b + 1,)] * wgt
            else:
                shp = list(v.shape)
                shp[d] = self._domain.shape[d]
                xnew = np.zeros(shp, dtype=v.dtype)
                np.add.at(xnew, idx + (b,), v * (1.0 - wgt))
                np.add.at(xnew, idx + (b + 1,), v * wgt)
            v = xnew
        return v

    def apply(self, x, mode):
        self._check_input(x, mode)
        v = x.val
        if v.is_cuda:
            return Field(self._tgt(mode), self._device(v, mode))
        return Field(self._tgt(mode), _np_result(self._host(v.numpy(), mode), v))
