"""First numbers of the device NUFFT (Nufft / Gridder, nk_nufft.hip): warmed TIMES and ADJOINT times from device events, the
spreading and interpolation cost per point, the share of nk_fftn, the host plan time -- uniform uv coverage against a
concentrated one (density ~ 1/|uv|, the dense core of radio coverage).  One JSON line per workload; the last lines are the
gate of docs/NUFFT.md (per point, concentrated <= 1.5 x uniform).

usage: python tools/gpu_nufft_probe.py [--quick] [--reps R] [--out FILE]
       per-kernel times: rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_nufft_probe.py --quick"""
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


def points(kind, m, ndim, rng):
    if kind == "uniform":
        return rng.random((m, ndim)) - 0.5
    # density ~ 1 / |uv| in the plane: uniform radius, uniform angle
    r = 0.5 * rng.random(m)
    phi = 2 * np.pi * rng.random(m)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def run(shape, m, eps, dtype, kind, reps, seed=0):
    rng = np.random.default_rng(seed)
    pos = points(kind, m, len(shape), rng)
    t0 = time.perf_counter()
    op = ift.Nufft(ift.RGSpace(shape, (1.0,) * len(shape)), pos, eps)  # uv in [-1/2, 1/2): the whole band
    plan_s = time.perf_counter() - t0
    p = op.plan
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    dp = p.device_plan(dev)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    cdt = torch.complex64 if dtype == "fp32" else torch.complex128
    rdt = torch.float32 if dtype == "fp32" else torch.float64
    v = torch.randn(m, dtype=cdt, device=dev)
    g = torch.randn(p.nmodes, dtype=rdt, device=dev)
    grid = torch.empty(p.n, dtype=cdt, device=dev)
    out = torch.empty(p.nmodes, dtype=rdt, device=dev)
    y = torch.empty(m, dtype=cdt, device=dev)
    times = lambda: p.times_device(v)  # noqa: E731
    adjoint = lambda: p.adjoint_device(g)  # noqa: E731
    for f in (times, adjoint):
        f()
        f()
    torch.cuda.synchronize()
    res = dict(shape=list(shape), grid=list(p.n), m=m, eps=eps, dtype=dtype, points=kind, w=p.w, items=int(len(p.item)),
               slabs=p.n_slabs, max_list=p.max_list, plan_s=round(plan_s, 3), upload_s=round(upload_s, 3))
    res["times_ms"] = timed(times, reps)
    res["adjoint_ms"] = timed(adjoint, reps)
    res["spread_ms"] = timed(lambda: dp.spread(v, grid), reps)
    res["interp_ms"] = timed(lambda: dp.interp(grid, y), reps)
    res["fft_inv_ms"] = timed(lambda: B.fftn(grid, ndim=p.ndim, inverse=True), reps)
    res["fft_fwd_ms"] = timed(lambda: B.fftn(grid, ndim=p.ndim, inverse=False), reps)
    res["crop_ms"] = timed(lambda: dp.crop(grid, out), reps)
    res["pad_ms"] = timed(lambda: dp.pad(g, grid), reps)
    res["spread_ns_per_point"] = 1e6 * res["spread_ms"] / m
    res["interp_ns_per_point"] = 1e6 * res["interp_ms"] / m
    res["fft_share_times"] = res["fft_inv_ms"] / res["times_ms"]
    res["fft_share_adjoint"] = res["fft_fwd_ms"] / res["adjoint_ms"]
    for k, val in list(res.items()):
        if isinstance(val, float) and k != "eps":
            res[k] = round(val, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^22 points, eps 1e-6 only (the profiled run)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU"
    work = []
    for m in ([1 << 22] if a.quick else [1 << 22, 1 << 24]):
        for eps, dt in ([(1e-6, "fp64")] if a.quick else [(1e-6, "fp64"), (1e-10, "fp64"), (1e-5, "fp32")]):
            for kind in ("uniform", "concentrated"):
                work.append(((1024, 1024), m, eps, dt, kind))
    work.append(((128, 128, 128), 1 << 22, 1e-6, "fp64", "uniform"))
    lines = []
    with torch.cuda.device(0):
        for shape, m, eps, dt, kind in work:
            r = run(shape, m, eps, dt, kind, a.reps)
            lines.append(r)
            print(json.dumps(r), flush=True)
        gates = []
        for r in lines:
            if r["points"] != "concentrated":
                continue
            u = next(x for x in lines if x["points"] == "uniform" and x["shape"] == r["shape"] and x["m"] == r["m"]
                     and x["eps"] == r["eps"] and x["dtype"] == r["dtype"])
            g = dict(gate="concentrated/uniform per point", m=r["m"], eps=r["eps"], dtype=r["dtype"],
                     times=round(r["times_ms"] / u["times_ms"], 3), adjoint=round(r["adjoint_ms"] / u["adjoint_ms"], 3))
            g["pass"] = g["times"] <= 1.5 and g["adjoint"] <= 1.5
            gates.append(g)
            print(json.dumps(g), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines + gates:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
