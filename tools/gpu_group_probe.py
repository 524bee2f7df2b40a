"""Grouped launches of the sandwich's first and final pass (nk_hartley_sandwich_group) against separate launches, 1024^3 fp32
by default: per-pass times from the library's live profile (HIP events around every pass launch) and whole applications from
HIP events, for count = 2 and 4 of
  class 8  first pass with the pending CG direction update: members share in2 / xi / afield (sampling solves),
  class 5  first pass with a shared `in` at different linearisation points (samples of a KL metric),
each with the VJP final pass of class 2/1 (shared xi / afield in the class-8 case).  Bit equality of every output is checked
on the way.  Counters: run it under `rocprofv3 --pmc FETCH_SIZE` (and TCC_HIT TCC_MISS) in a run of its own, tools/pmc_fetch.sh
is the pattern; NK_PROBE_ONLY=grouped|single restricts the launches to one side for that.
    python tools/gpu_group_probe.py [edge]"""
import os
import sys

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from nifty_amd import _lib as L  # noqa: E402
from nifty_amd import random  # noqa: E402
from nifty_amd.engine import CgWorkspace, FusedModel, LatentVec  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
only = os.environ.get("NK_PROBE_ONLY", "")
reps = int(os.environ.get("NK_PROBE_REPS", "5"))
model = FusedModel((n, n, n), offset_mean=2.0, likelihood="gaussian", icov=100.0, dtype=torch.float32, device="cuda:0")
random.push_sseq_from_seed(3)
model.set_data(model.signal(model.draw_prior()), 100.0)
xs = [0.1 * model.draw_prior() for _ in range(4)]
ds = [model.draw_prior() for _ in range(4)]
rs = [model.draw_prior() for _ in range(4)]
random.pop_sseq()
lps = [model.metric_point(x) for x in xs]
lib = L.load()
assert model.group_ready(), "the grouped path does not serve this model (NK_GROUP=0?)"


def clone(v):
    return LatentVec(v.xi.clone(), v.small.clone())


def workspace(m):
    ws = CgWorkspace(torch.device("cuda:0"))
    ws.scal[0], ws.scal[2] = 2.0 + m, 1.0 + 0.25 * m
    return ws


def class8(count, grouped):
    dd, wss = [clone(ds[m]) for m in range(count)], [workspace(m) for m in range(count)]
    dots = [torch.zeros(1, dtype=torch.float64, device="cuda:0") for _ in range(count)]
    for m in range(count):
        wss[m].direction_small(dd[m], rs[m])
    if grouped:
        qs = model.lh_metric_group(lps[0], [dict(d=dd[m], identity=1.0, dot_out=dots[m], cg_direction=(rs[m], wss[m]))
                                            for m in range(count)])
    else:
        qs = [model.metric(lps[0], dd[m], dot_out=dots[m], cg_direction=(rs[m], wss[m])) for m in range(count)]
    return [t for q, d, dot in zip(qs, dd, dots) for t in (q.xi, q.small, d.xi, dot)]


def class5(count, grouped):
    if grouped:
        qs = model.lh_metric_group(lps[0], [dict(d=ds[0], addend=(xs[m], -1.0), lp=lps[m]) for m in range(count)])
    else:
        qs = [model.lh_metric(lps[m], ds[0], minus=xs[m]) for m in range(count)]
    return [t for q in qs for t in (q.xi, q.small)]


def timed(fn, count, grouped):
    fn(count, grouped)
    torch.cuda.synchronize()
    lib.nk_profile_enable(1)
    bench.collect_profile()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn(count, grouped)
    e1.record()
    torch.cuda.synchronize()
    prof = bench.collect_profile()
    lib.nk_profile_enable(0)
    first = sum(ms for (k, p, e), (ms, c) in prof.items() if k == 5) / (reps * count)
    final = sum(ms for (k, p, e), (ms, c) in prof.items() if k == 3) / (reps * count)
    return e0.elapsed_time(e1) / (reps * count), first, final, out


for name, fn in (("class 8 (shared in2 / xi / afield)", class8), ("class 5 (shared in)", class5)):
    for count in (2, 4):
        res = {}
        for grouped in (False, True):
            if only and only != ("grouped" if grouped else "single"):
                continue
            res[grouped] = timed(fn, count, grouped)
            app, first, final, _ = res[grouped]
            print(f"{name:36s} count {count} {'grouped ' if grouped else 'separate'}: first pass {first:6.3f} ms / member, "
                  f"final pass {final:6.3f} ms / member, application {app:7.3f} ms / member", flush=True)
        if len(res) == 2:
            same = all(torch.equal(a, b) for a, b in zip(res[False][3], res[True][3]))
            print(f"{name:36s} count {count} bit-identical outputs: {same}", flush=True)
            assert same
print(f"peak allocated {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
