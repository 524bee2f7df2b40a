"""First numbers of the device LinearInterpolator and RegriddingOperator (nk_sample.hip): warmed TIMES and ADJOINT_TIMES
times from device events (5 repetitions of a window of 20 launches, the median) -- uniform points against clustered ones (density ~ 1 / r around one point) -- each beside the same
product done by nk_csr_rowsum on the explicit matrix and its transpose (built here only: 2 x 2^d x 8 bytes of plan per
point against the matrix-free 8 d + 24), and the regridding passes against the copy bandwidth achieved in the same run.
One JSON line per workload.  Nothing here gates on a time.

usage: python tools/gpu_sampling_probe.py [--quick] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nifty_amd as ift  # noqa: E402
from nifty_amd import backend as B  # noqa: E402


def points(kind, m, shape, rng):
    """(ndim, m) positions in units of the box (distances 1 / N): uniform, or density ~ 1 / r around the box centre"""
    nd = len(shape)
    if kind == "uniform":
        return rng.random((nd, m))
    if nd == 2:  # density ~ 1 / r in the plane: uniform radius, uniform angle
        r, phi = 0.5 * rng.random(m), 2 * np.pi * rng.random(m)
        return 0.5 + np.stack([r * np.cos(phi), r * np.sin(phi)])
    r = 0.5 * np.sqrt(rng.random(m))  # density ~ 1 / r in space: p(r) ~ r
    d = rng.standard_normal((3, m))
    return 0.5 + r * d / np.linalg.norm(d, axis=0)


BATCH = 20  # launches per timed window: a single launch here is 0.1-1 ms, too short a window on its own


def timed(fn, reps):
    """`reps` repetitions of a warmed window of BATCH launches between two device events -> (median, min, max) ms per launch"""
    fn()
    fn()
    per_launch = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(BATCH):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        per_launch.append(ev[0].elapsed_time(ev[1]) / BATCH)
    return float(np.median(per_launch)), min(per_launch), max(per_launch)


def put(res, key, fn, reps):
    """res[key + "_ms"] = median time of fn, res[key + "_ms_range"] = [fastest, slowest] repetition"""
    med, lo, hi = timed(fn, reps)
    res[key + "_ms"], res[key + "_ms_range"] = med, [round(lo, 4), round(hi, 4)]
    return med


def explicit_matrix(plan, dev):
    """CSR arrays of the interpolation matrix and of its transpose on the device (int64 rowptr, int32 col, float32 weights:
    what nk_csr_rowsum reads), and their bytes"""
    from scipy.sparse import csr_matrix

    nc = 1 << plan.ndim
    col = np.empty((plan.npoints, nc), dtype=np.int32)
    wgt = np.empty((plan.npoints, nc), dtype=np.float32)
    for m in range(nc):
        idx, w = plan.corner(m)
        col[:, m], wgt[:, m] = idx, w
    rowptr = np.arange(plan.npoints + 1, dtype=np.int64) * nc
    mat = csr_matrix((wgt.reshape(-1), col.reshape(-1), rowptr), shape=(plan.npoints, plan.size))
    mt = mat.tocsc()
    host = (rowptr, col.reshape(-1), wgt.reshape(-1), mt.indptr.astype(np.int64), mt.indices.astype(np.int32), mt.data.astype(np.float32))
    return tuple(torch.from_numpy(a).to(dev) for a in host), sum(a.nbytes for a in host)


def run_interp(shape, m, kind, reps, seed=0):
    """both precisions of one workload (the plan and the explicit matrix are made once)"""
    rng = np.random.default_rng(seed)
    pts = points(kind, m, shape, rng)
    t0 = time.perf_counter()
    op = ift.LinearInterpolator(ift.RGSpace(shape), pts)
    plan_s = time.perf_counter() - t0
    plan = op.plan
    dev = torch.device("cuda", 0)
    dp = plan.device_plan(dev)
    arrs, nbytes = explicit_matrix(plan, dev)
    counts = np.diff(plan.cell_start)
    lt, la = B.lanes_for(m << plan.ndim, m), B.lanes_for(m << plan.ndim, plan.size)
    out = []
    for dtype, tdt in (("fp64", torch.float64), ("fp32", torch.float32)):
        x = torch.randn(shape, dtype=tdt, device=dev)
        y = torch.randn(m, dtype=tdt, device=dev)
        xf = x.reshape(-1)
        res = dict(op="LinearInterpolator", shape=list(shape), m=m, points=kind, dtype=dtype, plan_s=round(plan_s, 3),
                   occupied_cells=int(len(counts)), long_cells=int(len(plan.long_cell)), longest_cell=int(counts.max()),
                   plan_bytes=int(plan.nbytes), csr_bytes=int(nbytes), plan_ratio_csr_over_matrix_free=nbytes / plan.nbytes)
        put(res, "times", lambda: dp.times(x), reps)
        put(res, "adjoint", lambda: dp.adjoint(y), reps)
        put(res, "csr_times", lambda: B.spmv(arrs[0], arrs[1], arrs[2], xf, m, lt), reps)
        put(res, "csr_adjoint", lambda: B.spmv(arrs[3], arrs[4], arrs[5], y, plan.size, la), reps)
        res["times_over_csr"] = res["times_ms"] / res["csr_times_ms"]
        res["adjoint_over_csr"] = res["adjoint_ms"] / res["csr_adjoint_ms"]
        out.append(res)
    return out


def run_regrid(shape, new_shape, dtype, reps):
    dev = torch.device("cuda", 0)
    op = ift.RegriddingOperator(ift.RGSpace(shape), new_shape)
    tdt = torch.float32 if dtype == "fp32" else torch.float64
    x = ift.Field(op.domain, torch.randn(shape, dtype=tdt, device=dev))
    y = ift.Field(op.target, torch.randn(new_shape, dtype=tdt, device=dev))
    src, dst = torch.randn(int(np.prod(shape)), dtype=tdt, device=dev), torch.empty(int(np.prod(shape)), dtype=tdt, device=dev)
    copy_ms = timed(lambda: dst.copy_(src), reps)[0]
    copy_gbs = 2 * src.numel() * src.element_size() / copy_ms * 1e-6
    res = dict(op="RegriddingOperator", shape=list(shape), new_shape=list(new_shape), dtype=dtype, copy_gb_per_s=copy_gbs)
    put(res, "times", lambda: op(x), reps)
    put(res, "adjoint", lambda: op.adjoint(y), reps)
    # compulsory traffic: the input read once and the output written once (the fp64 intermediates between the axes come on top)
    size = src.element_size()
    moved = (int(np.prod(shape)) + int(np.prod(new_shape))) * size
    res["times_gb_per_s"] = moved / res["times_ms"] * 1e-6
    res["adjoint_gb_per_s"] = moved / res["adjoint_ms"] * 1e-6
    res["times_share_of_copy"] = res["times_gb_per_s"] / copy_gbs
    res["adjoint_share_of_copy"] = res["adjoint_gb_per_s"] / copy_gbs
    return res


def rounded(res):
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^20 points on small grids (a functional run)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU"
    m = 1 << 20 if a.quick else 1 << 22
    grids = [(1024, 1024), (64, 64, 64)] if a.quick else [(4096, 4096), (256, 256, 256)]
    regrids = [((1024, 1024), (750, 750))] if a.quick else [((4096, 4096), (3000, 3000)), ((512, 512, 512), (300, 300, 300))]
    lines = []
    with torch.cuda.device(0):
        for shape in grids:
            for kind in ("uniform", "clustered"):
                for res in run_interp(shape, m, kind, a.reps):
                    lines.append(rounded(res))
                    print(json.dumps(lines[-1]), flush=True)
        for shape, new_shape in regrids:
            for dt in ("fp64", "fp32"):
                lines.append(rounded(run_regrid(shape, new_shape, dt, a.reps)))
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
