"""Generate tests/golden/sampling_ops.npz from the REAL reference: LinearInterpolator and RegriddingOperator on the host
cases of tests/sampling_cases.py -- the points, the inputs and the reference's fp64 TIMES / ADJOINT_TIMES outputs.

Runs only where the reference tree is present (tests/golden/_ref_shim.py); the .npz it writes is committed, this script
documents how.  Usage:  python tests/golden/make_golden_sampling.py

The reference's RegriddingOperator raises in ADJOINT_TIMES on an axis of old length 1 (np.bincount of a negative index):
that case stores its TIMES output only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_shim  # noqa: E402

from tests import sampling_cases as sc  # noqa: E402

ift = _ref_shim.load()


def main():
    out = {}
    for seed, (name, spaces) in enumerate(sc.INTERP_CASES.items()):
        rng = np.random.default_rng(100 + seed)
        shape, dist = sc.grid_of(spaces)
        points = sc.interp_points(shape, dist, rng)
        dom = tuple(ift.RGSpace(shp, dst) for shp, dst in spaces)
        op = ift.LinearInterpolator(dom, points)
        x, y = rng.standard_normal(shape), rng.standard_normal(points.shape[1])
        out[f"interp.{name}.points"], out[f"interp.{name}.x"], out[f"interp.{name}.y"] = points, x, y
        out[f"interp.{name}.times"] = op(ift.makeField(op.domain, x)).asnumpy()
        out[f"interp.{name}.adjoint"] = op.adjoint(ift.makeField(op.target, y)).asnumpy()
    for seed, (name, case) in enumerate(sc.REGRID_CASES.items()):
        rng = np.random.default_rng(200 + seed)
        desc, new_shape, space = case
        dom = tuple(ift.RGSpace(v) if kind == "rg" else ift.UnstructuredDomain(v) for kind, v in desc)
        op = ift.RegriddingOperator(dom, new_shape, space)
        x, y = rng.standard_normal(op.domain.shape), rng.standard_normal(op.target.shape)
        out[f"regrid.{name}.x"], out[f"regrid.{name}.y"] = x, y
        out[f"regrid.{name}.times"] = op(ift.makeField(op.domain, x)).asnumpy()
        try:
            out[f"regrid.{name}.adjoint"] = op.adjoint(ift.makeField(op.target, y)).asnumpy()
        except ValueError as exc:
            print(f"regrid.{name}: the reference's adjoint raises ({exc}); TIMES only")
    path = os.path.join(HERE, "sampling_ops.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
