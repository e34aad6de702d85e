"""Timing of AvgPool2d on position-pair maps (csrc/covpool.hip), HIP events,
all in one process, by the method of tools/pool_bench.py: cgp_covmap_avgpool_* at k = s = 2
on ``--pairs`` position-pair maps of 28x28 images, in GB/s over its algorithmic bytes (one
read of the map and one write of a map a sixteenth its size), with cgp_cov_nonlin_* ReLU (a
read and a write of the map) and cgp_cov_pool_* (a read) on the same maps as yardsticks, and
cgp_covmap_diag_* on them for its launch time.  Then pairs/s end to end of one off-diagonal
16 x 16 tile of configs/mnist_paper_convnet_gp.py's body + GlobalAvgPool, with an
AvgPool2d(2) after its second and fourth conv + ReLU and without (tools/pool_bench.py's
model), interleaved.

After a warm-up of every pass, ``--reps`` rounds each time every pass once; a kernel pass is
``--inner`` back-to-back launches between two events.  Every figure is the per-launch median
over the rounds with the fastest and slowest round beside it.

    python tools/avgpool_bench.py [--pairs 64] [--tile 16] [--reps 9] [--inner 5]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

import torch  # noqa: E402

import cnn_gp  # noqa: E402
from cnn_gp import _native as N  # noqa: E402

from erf_bench import timed_interleaved  # noqa: E402
from pool_bench import pooled_convnet  # noqa: E402


def kernels(pairs, side, reps, inner, dt):
    sfx = "f64" if dt == torch.float64 else "f32"
    hw = side * side
    n = hw * hw
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *s: torch.rand(s, dtype=dt, device="cuda", generator=g)        # noqa: E731
    pi = torch.arange(pairs, dtype=torch.int32, device="cuda")
    vx, vy = rand(pairs, hw) + 0.5, rand(pairs, hw) + 0.5
    s = rand(pairs, n) * 0.9
    out = torch.empty_like(s)
    small = torch.empty((pairs, n // 16), dtype=dt, device="cuda")
    pooled = torch.empty(pairs, dtype=dt, device="cuda")
    diag = torch.empty((pairs, hw), dtype=dt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    gb = s.numel() * s.element_size() / 1e9

    a = N.CovAvgPoolArgs()
    a.in_, a.out, a.npairs = N.ptr(s), N.ptr(small), pairs
    a.h = a.w = side
    a.ho = a.wo = side // 2
    a.k = a.stride = 2
    r = N.CovNonlinArgs()
    r.in_, r.out, r.xx, r.yy = N.ptr(s), N.ptr(out), N.ptr(vx), N.ptr(vy)
    r.pair_i, r.pair_j, r.npairs = N.ptr(pi), N.ptr(pi), pairs
    r.h = r.w = side
    r.kind = N.CGP_COV_RELU
    avg, nonlin = getattr(lib, f"cgp_covmap_avgpool_{sfx}"), getattr(lib, f"cgp_cov_nonlin_{sfx}")
    # name -> (launch, map passes over HBM)
    passes = {
        "covmap_avgpool": (lambda: N.check(avg(ctypes.byref(a), stream), "bench"), 1 + 1 / 16),
        "cov_relu": (lambda: N.check(nonlin(ctypes.byref(r), stream), "bench"), 2),
        "cov_pool": (lambda: N.call(f"cgp_cov_pool_{sfx}", N.ptr(s), pairs, n, N.ptr(pooled),
                                    stream), 1),
        "covmap_diag": (lambda: N.call(f"cgp_covmap_diag_{sfx}", N.ptr(s), N.ptr(pi), pairs, side,
                                       side, N.ptr(diag), stream), 0),
    }
    times = timed_interleaved({k: fn for k, (fn, _) in passes.items()}, reps, inner)
    return {k: dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                    **({"gbps": round(passes[k][1] * gb / (med / 1e3), 1)} if passes[k][1] else {}))
            for k, (med, lo, hi) in times.items()}


def avgpooled_convnet():
    """pool_bench's model with an AvgPool2d(2) after the second and fourth conv + ReLU:
    28x28 -> 14x14 -> 7x7 maps"""
    mods = list(pooled_convnet().mods)
    for at in (8, 4):
        mods.insert(at, cnn_gp.AvgPool2d(2))
    return cnn_gp.Sequential(*mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--tile", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 position-pair maps", dtype=name, pairs=args.pairs,
                              **kernels(args.pairs, 28, args.reps, args.inner, dt))), flush=True)
    B = args.tile
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        g = torch.Generator().manual_seed(0)
        x = torch.rand((B, 1, 28, 28), generator=g, dtype=dt).cuda()
        y = torch.rand((B, 1, 28, 28), generator=g, dtype=dt).cuda()
        models = {"mnist_paper_convnet_gp body + GlobalAvgPool": pooled_convnet().to("cuda", dt),
                  "the same with AvgPool2d(2) after conv 2 and conv 4":
                      avgpooled_convnet().to("cuda", dt)}
        with torch.no_grad():
            times = timed_interleaved(
                {k: (lambda mod=mod: mod(x, y, False, False)) for k, mod in models.items()},
                args.reps, 1)
        for k, (med, lo, hi) in times.items():
            print(json.dumps(dict(config=k, dtype=name, tile=B, ms=round(med, 3),
                                  min_ms=round(lo, 3), max_ms=round(hi, 3),
                                  pairs_per_s=round(B * B / (med / 1e3), 1))), flush=True)


if __name__ == "__main__":
    main()
