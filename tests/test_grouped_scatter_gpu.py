"""nk_octant_scatter_k2_group: the shell scatter of the members of a launch group in one walk.

Kernel level (this process, through the C ABI, every array between guard bands): for groups of 2, 3 and 4 members on the shapes
of tests/binmap_cases.py where the walk branches -- fewer first-axis lines than splits (16, 16, 256), odd lengths (33, 31, 255),
a second and a third shell, nb = 4096 exactly (8191,), runs past 16 points; every shape but (64, 64, 64) has more than 2048 bins,
so the boundary of a narrower grouped shell (NK_SHELL_GROUP_BINS = 2048) is crossed as well -- every member's bins must be the
BITS of nk_octant_scatter_k2 on that member alone and the bits of `fixed_point_scatter` on the host.  The members differ so that
a swapped scale or buffer shows: maxima 2^40 and 2^-40, an all-zero member, a maximum below 2^-979, a member with a NaN (its
bins, and only its, are NaN) and one array passed as two members.  A group without scales takes the floating-point kernel member
by member: held to the per-bin bound tests/test_binmap_kernels_gpu.py holds the single call to.

Engine level (two child processes, NK_GROUP_SCATTER=0 against the default; the engine reads the switch once per model):
lh_metric_group with 2, 3 and 4 jobs -- with cg_direction, identity and dot_out, and with linearisation points of their own --
and lh_metric_accumulate_pair at the 3-D shapes of tests/group_cases.py, fp64 and fp32: xi and small of every member and the
curvature dots are compared as SHA-256 digests."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nifty_amd import _lib as L
from tests import binmap_cases as bc
from tests import group_cases as gc
from tests.test_fused_transforms_gpu import Guarded, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def shp(shape):
    return (ctypes.c_int64 * len(shape))(*shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ptrs(items):
    return (ctypes.c_void_p * len(items))(*[g.ptr for g in items])


def members(geo):
    """name -> (w8, w8max): what the issue asks the members of a group to be"""
    sets = {name: (w8, wmax) for name, w8, wmax, _ in bc.scatter_datasets(geo)}
    normal, lu = sets["normal_wmax_true"][0], sets["loguniform_12_decades"][0]
    big, small = np.ldexp(normal, 40), np.ldexp(lu, -40)
    with_nan = normal.copy()
    with_nan.reshape(-1)[with_nan.size // 3] = NAN
    tiny = np.ldexp(sets["all_negative"][0], -990)  # maximum ~2^-988 < 2^-979: the clamped quantum 2^-1023, sums of ~2^33 quanta
    assert 0 < np.abs(tiny).max() < 2.0 ** -979
    return {
        "big": (big, float(np.abs(big).max())),
        "small": (small, float(np.abs(small).max())),
        "zero": (np.zeros(geo.oshape), 0.0),
        "tiny": (tiny, float(np.abs(tiny).max())),
        "nan": (with_nan, NAN),                      # the final pass joins the maxima with a NaN-propagating rule
    }


GROUPS = [("big", "small"), ("nan", "zero"), ("small", "small"),
          ("small", "nan", "big"), ("tiny", "zero", "big"),
          ("big", "small", "zero", "tiny"), ("nan", "big", "big", "small")]


class GroupDevice:
    def __init__(self, geo):
        self.geo, self.lib = geo, L.load()
        self.pidx, self.k2 = Guarded(geo.pidx), Guarded(geo.bin_k2)
        self.w8 = {}

    def operand(self, name, w8):
        if name not in self.w8:  # one device array per member NAME: a name used twice in a group is the same pointer twice
            self.w8[name] = Guarded(w8)
        return self.w8[name]

    def single(self, name, w8, wmax):
        geo, w8d = self.geo, self.operand(name, w8)
        wm = None if wmax is None else Guarded(np.array([wmax], dtype=np.float64))
        scratch, abar = Guarded(nbytes=8 * geo.scratch_doubles()), Guarded(np.full(geo.nb, NAN))
        L.check(self.lib.nk_octant_scatter_k2(geo.ndim, shp(geo.shape), w8d.ptr, self.pidx.ptr, self.k2.ptr, geo.nb, scratch.ptr,
                                              abar.ptr, wm.ptr if wm else None, stream()), "nk_octant_scatter_k2")
        return self.settle([abar, scratch], [w8d] + ([wm] if wm else []))[0]

    def group(self, names, data, scaled=True):
        geo = self.geo
        w8d = [self.operand(n, data[n][0]) for n in names]
        wm = [Guarded(np.array([data[n][1]], dtype=np.float64)) for n in names] if scaled else []
        scratch = [Guarded(nbytes=8 * 16 * (geo.nb + 32)) for _ in names]  # include/niftyk.h: 16 split rows per member
        abar = [Guarded(np.full(geo.nb, NAN)) for _ in names]
        L.check(self.lib.nk_octant_scatter_k2_group(geo.ndim, shp(geo.shape), len(names), ptrs(w8d), self.pidx.ptr, self.k2.ptr,
                                                    geo.nb, ptrs(scratch), ptrs(abar), ptrs(wm) if scaled else None, stream()),
                "nk_octant_scatter_k2_group")
        return self.settle(abar + scratch, w8d + wm)[:len(names)]

    def settle(self, outputs, inputs):
        torch.cuda.synchronize()
        for g in list(outputs) + list(inputs) + [self.pidx, self.k2]:
            assert g.guards_intact()
        for g in list(inputs) + [self.pidx, self.k2]:
            assert g.unchanged()
        return [g.get() if g.arr is not None else None for g in outputs]


_REF = {}


def references(shape):
    """per shape, once: the members, the host restatement and the single device call of each"""
    if shape not in _REF:
        geo = bc.geometry(shape)
        dev, data = GroupDevice(geo), members(geo)
        host = {n: bc.fixed_point_scatter(geo, w8, wmax)[0] for n, (w8, wmax) in data.items()}
        single = {n: dev.single(n, w8, wmax) for n, (w8, wmax) in data.items()}
        _REF[shape] = (geo, dev, data, host, single)
    return _REF[shape]


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.mark.parametrize("shape", list(bc.SHELL_SHAPES), ids=ids(bc.SHELL_SHAPES))
def test_single_calls_are_the_host_restatement(shape):
    """the two references of the grouped test agree with each other (and the NaN member is NaN in every bin, no other is)"""
    geo, _, data, host, single = references(shape)
    assert (geo.nb, geo.shells) == bc.SHELL_SHAPES[shape]
    for n in data:
        assert np.array_equal(bits(single[n]), bits(host[n])), n
        assert np.isnan(single[n]).all() if n == "nan" else np.isfinite(single[n]).all(), n
    assert not single["zero"].any() and single["tiny"].any()


@pytest.mark.parametrize("names", GROUPS, ids=["+".join(g) for g in GROUPS])
@pytest.mark.parametrize("shape", list(bc.SHELL_SHAPES), ids=ids(bc.SHELL_SHAPES))
def test_group_is_bitwise_the_single_call_per_member(shape, names):
    geo, dev, data, host, single = references(shape)
    got = dev.group(names, data)
    bad = []
    for g, n in enumerate(names):
        d_single = int(np.count_nonzero(bits(got[g]) != bits(single[n])))
        d_host = int(np.count_nonzero(bits(got[g]) != bits(host[n])))
        print(f"BITS nk_octant_scatter_k2_group {'x'.join(map(str, shape))} member {g}:{n} of {len(names)} "
              f"differing from single={d_single} from host={d_host}")
        if d_single or d_host:
            bad.append((g, n, d_single, d_host))
    assert not bad, bad


@pytest.mark.parametrize("shape", [(16, 16, 256), (33, 31, 255), (8191,)], ids=ids([(16, 16, 256), (33, 31, 255), (8191,)]))
def test_group_without_scales_runs_the_floating_point_singles(shape):
    geo, dev, data, _, _ = references(shape)
    for names in (("big", "small"), ("small", "big", "small"), ("big", "small", "zero", "big")):
        got = dev.group(names, data, scaled=False)
        for g, n in enumerate(names):
            ref, mag = bc.shell_reference(geo, data[n][0])
            bound = bc.float_shell_bound(geo, mag)
            w = bc.worst(got[g], ref, bound)
            bc.record("nk_octant_scatter_k2_group", shape, "f64", f"float:{n}:{g}of{len(names)}", w)
            assert w[0] <= 1, (names, g, w)
            one = dev.single(n, data[n][0], None)  # both within `bound` of the exact sum: within 2 bound of each other
            assert np.all(np.abs(got[g].astype(bc.LD) - one.astype(bc.LD)) <= 2 * bound), (names, g)


def test_group_refuses_bad_arguments():
    geo, dev, data, _, _ = references((16, 16, 256))
    lib, st = dev.lib, stream()
    w8d = [dev.operand(n, data[n][0]) for n in ("big", "small")]
    wm = [Guarded(np.array([data[n][1]])) for n in ("big", "small")]
    scratch = [Guarded(nbytes=8 * geo.scratch_doubles()) for _ in range(2)]
    abar = [Guarded(np.full(geo.nb, NAN)) for _ in range(2)]
    s3, nb = shp(geo.shape), geo.nb
    null2 = (ctypes.c_void_p * 2)(w8d[0].ptr, None)
    big = shp((8192, 8192, 8192))
    cases = {
        "n = 0": lambda: lib.nk_octant_scatter_k2_group(3, s3, 0, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st),
        "n = 5": lambda: lib.nk_octant_scatter_k2_group(3, s3, 5, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st),
        "null w8": lambda: lib.nk_octant_scatter_k2_group(3, s3, 2, None, dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st),
        "null member": lambda: lib.nk_octant_scatter_k2_group(3, s3, 2, null2, dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st),
        "null pidx": lambda: lib.nk_octant_scatter_k2_group(3, s3, 2, ptrs(w8d), None, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st),
        "nb = 0": lambda: lib.nk_octant_scatter_k2_group(3, s3, 2, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, 0, ptrs(scratch), ptrs(abar), ptrs(wm), st),
        "shared scratch": lambda: lib.nk_octant_scatter_k2_group(3, s3, 2, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, nb, ptrs([scratch[0]] * 2), ptrs(abar), ptrs(wm), st),
        "shared abar": lambda: lib.nk_octant_scatter_k2_group(3, s3, 2, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs([abar[0]] * 2), ptrs(wm), st),
        "ndim 4": lambda: lib.nk_octant_scatter_k2_group(4, shp((4, 4, 4, 4)), 2, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st),
    }
    for name, call in cases.items():
        assert call() == L.NK_ERR_INVALID, name
    rc = lib.nk_octant_scatter_k2_group(3, big, 2, ptrs(w8d), dev.pidx.ptr, dev.k2.ptr, nb, ptrs(scratch), ptrs(abar), ptrs(wm), st)
    assert rc == L.NK_ERR_UNSUPPORTED and b"k^2 range too large" in lib.nk_last_error()
    torch.cuda.synchronize()
    for g in abar + scratch:  # nothing was launched
        assert g.guards_intact() and (g.arr is None or np.isnan(g.get()).all())


# ---- engine level ---------------------------------------------------------------------------------------------------------------
def _pair_digests(model, lps, d):
    from nifty_amd.engine import LatentVec

    out = LatentVec(torch.empty_like(d.xi), None)
    dot = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    model.lh_metric_accumulate_pair(lps[0], lps[1], d, out, 0.5, True, identity=1.0, dot_out=dot)
    return {"pair_xi": out.xi, "pair_small": out.small, "pair_dot": dot}


def engine_digests():
    """xi, small and the curvature dot of every member of every grouped route (run in a child process)"""
    out = {}
    for shape, dtype in gc.PASS_SHAPES:
        model, xs, ds, rs = gc.pass_setup(shape, dtype)
        assert model.group_ready() and model.pair_ready() and model.bin_k2 is not None and model.scatter_fixed_point
        lps = [model.linearize(x) for x in xs]
        tag = "x".join(map(str, shape))
        for count in (2, 3, 4):
            for k, v in gc.class8_group(model, lps[0], ds, rs, count).items():
                if k.startswith(("out", "small", "dot")):
                    out[f"{tag}/c8/{count}/{k}"] = gc.digest(v)
            for k, v in gc.class5_group(model, lps, ds[0], count).items():
                if k.startswith(("out", "small")):
                    out[f"{tag}/c5/{count}/{k}"] = gc.digest(v)
        for k, v in _pair_digests(model, lps, ds[1]).items():
            out[f"{tag}/{k}"] = gc.digest(v)
        for k, v in gc.kl_metric(model, xs, ds[0]).items():
            out[f"{tag}/{k}"] = gc.digest(v)
        out[f"{tag}/grouped_scatter"] = repr(bool(model.group_scatter))
    return out


def _child(switch):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("NK_GROUP_SCATTER", None)
    if switch is not None:
        env["NK_GROUP_SCATTER"] = switch
    r = subprocess.run([sys.executable, "-c", "import json; from tests.test_grouped_scatter_gpu import engine_digests; "
                        "print('DIGESTS ' + json.dumps(engine_digests()))"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGESTS ")][-1]
    return json.loads(line[8:])


def test_engine_outputs_do_not_depend_on_the_grouped_scatter():
    on, off = _child(None), _child("0")
    tags = ["x".join(map(str, s)) for s, _ in gc.PASS_SHAPES]
    assert all(off[f"{t}/grouped_scatter"] == "False" for t in tags)
    assert sorted(on) == sorted(off) and len(on) > 60
    differ = [k for k in on if on[k] != off[k] and not k.endswith("/grouped_scatter")]
    assert not differ, differ
