"""Times nk_octant_scatter_k2 against nk_octant_scatter_k2_group on one octant (default 1024^3: 513^3 doubles per member).

    python tools/gpu_scatter_group_probe.py [--shape 1024,1024,1024] [--configs 4096x512,2048x1024,default] [--out FILE.jsonl]

The library reads the grouped kernel's shell width and workgroup size once per process (NK_SHELL_GROUP_BINS / _THREADS), so
every configuration runs in a child process of its own, under its own time limit; a child prints one JSON line (`default`,
reported as bins 0 x threads 0: what the library does with none of the sweep variables set).  Per configuration: the single
launch, 2, 3 and 4 singles back to back, the grouped launch for 2, 3 (the kernel of four with an inactive member) and 4 members
-- HIP events around 20 launches, REPEATS interleaved rounds after a warm-up round; reported are the median, the minimum and the
spread (max - min) of the rounds in ms per launch sequence, and whether every member's bins equal the single call's bits."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(4096, 256), (4096, 512), (4096, 1024), (2048, 256), (2048, 512), (2048, 1024)]  # (shell width, workgroup size)
LAUNCHES, REPEATS = 20, 7


def child(shape):
    import numpy as np
    import torch

    import nifty_amd as ift
    from nifty_amd import _lib as L, backend as B

    hsp = ift.RGSpace(shape).get_default_codomain()
    ps = ift.PowerSpace(hsp)
    dev = torch.device("cuda:0")
    pidx, nb = ps.device_pindex(dev), ps.shape[0]
    lib = L.load()
    shp = (ctypes.c_int64 * len(shape))(*shape)
    oshape = tuple(n // 2 + 1 for n in shape)
    k2 = torch.from_numpy(np.nonzero(hsp._k2_flags())[0].astype(np.int32)).to(dev)
    torch.manual_seed(0)
    w8 = [torch.randn(oshape, dtype=torch.float64, device=dev) * 4.0 ** g for g in range(4)]
    wmax = [w.abs().max().reshape(1).clone() for w in w8]
    scratch = [torch.empty(64 * (nb + 32), dtype=torch.float64, device=dev) for _ in range(4)]
    single = [torch.empty(nb, dtype=torch.float64, device=dev) for _ in range(4)]
    grouped = [torch.empty(nb, dtype=torch.float64, device=dev) for _ in range(4)]
    st = B._stream()

    def ptrs(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def singles(n):
        for g in range(n):
            L.check(lib.nk_octant_scatter_k2(len(shape), shp, w8[g].data_ptr(), pidx.data_ptr(), k2.data_ptr(), nb,
                                             scratch[g].data_ptr(), single[g].data_ptr(), wmax[g].data_ptr(), st), "single")

    def group(n):
        L.check(lib.nk_octant_scatter_k2_group(len(shape), shp, n, ptrs(w8[:n]), pidx.data_ptr(), k2.data_ptr(), nb,
                                               ptrs(scratch[:n]), ptrs(grouped[:n]), ptrs(wmax[:n]), st), "group")

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(LAUNCHES):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / LAUNCHES

    res = {"shape": list(shape), "nb": int(nb), "bins": int(os.environ.get("NK_SHELL_GROUP_BINS", 0)),
           "threads": int(os.environ.get("NK_SHELL_GROUP_THREADS", 0)), "launches": LAUNCHES, "repeats": REPEATS}
    singles(4)
    for n in (2, 3, 4):
        for t in grouped:
            t.fill_(float("nan"))
        group(n)
        torch.cuda.synchronize()
        res[f"bits_equal_{n}"] = all(bool(torch.equal(single[g].view(torch.int64), grouped[g].view(torch.int64))) for g in range(n))
    arms = (("single_x1", lambda: singles(1)), ("single_x2", lambda: singles(2)), ("group_2", lambda: group(2)),
            ("single_x3", lambda: singles(3)), ("group_3", lambda: group(3)),
            ("single_x4", lambda: singles(4)), ("group_4", lambda: group(4)))
    times = {name: [] for name, _ in arms}
    for r in range(REPEATS + 1):  # interleaved rounds: every arm of a round sees the same clocks; round 0 is the warm-up
        for name, fn in arms:
            t = timed(fn)
            if r:
                times[name].append(t)
    for name, out in times.items():
        res[name] = {"median_ms": float(np.median(out)), "spread_ms": float(max(out) - min(out)), "min_ms": float(min(out))}
    print("PROBE " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1024,1024,1024")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--configs", default=None, help="BINSxTHREADS,... (default: every configuration the library builds)")
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.shape.split(","))
    if a.child:
        return child(shape)
    lines = []
    configs = CONFIGS + [(0, 0)] if a.configs is None else [(0, 0) if c == "default" else tuple(int(v) for v in c.split("x"))
                                                            for c in a.configs.split(",")]
    for bins, threads in configs:
        env = {k: v for k, v in os.environ.items() if not k.startswith("NK_SHELL_GROUP_")}
        if bins:  # (0, 0) = `default`: what the library does unasked (reported as bins 0, threads 0)
            env.update(NK_SHELL_GROUP_BINS=str(bins), NK_SHELL_GROUP_THREADS=str(threads), NK_SHELL_GROUP_MAX="4")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", a.shape], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:  # a child that failed ends the sweep: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"configuration {bins} x {threads} ended with status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("PROBE "):
                lines.append(line[6:])
                print(line[6:], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
