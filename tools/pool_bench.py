"""Timing of the position-pair kernels of GlobalAvgPool (csrc/covpool.hip), HIP events, all
in one process: each cgp_cov_* kernel on ``--pairs`` position-pair maps of 28x28 images
((28·28)² = 614 656 elements per pair), with the bandwidth it achieves over its algorithmic
bytes (conv: itemsize·P·((HW)² + (HoWo)²), plus the addend; elementwise: one read and one
write; moments: the write; pool: the read), and beside them, in the same call, the layer
path's cgp_relu_* and cgp_conv_* (3x3 "same" stencil) on ordinary pair maps of equal total
size, as the yardstick.  Then pairs/s end to end of configs/mnist_paper_convnet_gp.py's
body with the final dense conv replaced by GlobalAvgPool, on a 16 x 16 tile.

The passes are timed interleaved: after a warm-up of every pass, ``--reps`` rounds each time
every pass once, as ``--inner`` back-to-back launches between two events.  Every figure is
the per-launch median over the rounds with the fastest and slowest round beside it.

    python tools/pool_bench.py [--pairs 64] [--tile 16] [--reps 9] [--inner 5]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

import torch  # noqa: E402

import cnn_gp  # noqa: E402
from cnn_gp import _native as N  # noqa: E402

from erf_bench import timed, timed_interleaved  # noqa: E402


def kernels(pairs, side, reps, inner, dt):
    sfx = "f64" if dt == torch.float64 else "f32"
    hw = side * side
    n = hw * hw
    n1 = int(round((pairs * hw) ** 0.5))
    assert n1 * n1 == pairs * hw, "pairs·side² must be a square (the yardstick's n1 x n1 tile)"
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *s: torch.rand(s, dtype=dt, device="cuda", generator=g)        # noqa: E731
    x, y = rand(pairs, 3, side, side), rand(pairs, 3, side, side)
    pi = torch.arange(pairs, dtype=torch.int32, device="cuda")
    vx, vy = rand(pairs, hw) + 0.5, rand(pairs, hw) + 0.5
    s = rand(pairs, n) * 0.9
    out, add = torch.empty_like(s), rand(pairs, n)
    pooled = torch.empty(pairs, dtype=dt, device="cuda")
    lvx, lvy = rand(n1, hw) + 0.5, rand(n1, hw) + 0.5
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    item = s.element_size()
    gb = s.numel() * item / 1e9

    def conv_args(post, addend):
        a = N.CovConvArgs()
        a.in_, a.out, a.xx, a.yy = N.ptr(s), N.ptr(out), N.ptr(vx), N.ptr(vy)
        a.addend = N.ptr(add) if addend else None
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pi), pairs
        a.h = a.w = a.ho = a.wo = side
        a.taps, a.offset, a.stride, a.dilation = 3, -1, 1, 1
        a.post, a.weight, a.bias = post, 1 / 9, 0.1
        return a

    def nonlin_args(kind):
        a = N.CovNonlinArgs()
        a.in_, a.out, a.xx, a.yy = N.ptr(s), N.ptr(out), N.ptr(vx), N.ptr(vy)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pi), pairs
        a.h = a.w = side
        a.kind = kind
        return a

    r = N.ReluArgs()
    r.xy, r.out, r.xx, r.yy = N.ptr(s), N.ptr(out), N.ptr(lvx), N.ptr(lvy)
    r.nmaps, r.n1, r.n2, r.hw = n1 * n1, n1, n1, hw
    c = N.ConvArgs()
    c.in_, c.out = N.ptr(s), N.ptr(out)
    c.nmaps, c.n1, c.n2 = n1 * n1, n1, n1
    c.h = c.w = c.ho = c.wo = side
    c.taps, c.offset, c.stride, c.dilation = 3, -1, 1, 1
    c.weight, c.bias = 1 / 9, 0.1

    cov_conv, cov_nonlin = (getattr(lib, f"cgp_cov_{k}_{sfx}") for k in ("conv", "nonlin"))
    relu, conv = getattr(lib, f"cgp_relu_{sfx}"), getattr(lib, f"cgp_conv_{sfx}")
    byref = lambda fn, a: (lambda: N.check(fn(ctypes.byref(a), stream), "bench"))   # noqa
    # name -> (launch, map passes over HBM)
    passes = {
        "cov_moments": (lambda: N.call(f"cgp_cov_moments_{sfx}", N.ptr(x), N.ptr(y), N.ptr(pi),
                                       N.ptr(pi), pairs, 3, side, side, N.ptr(out), stream), 1),
        "cov_conv": (byref(cov_conv, conv_args(N.CGP_COV_NONE, False)), 2),
        "cov_conv_relu": (byref(cov_conv, conv_args(N.CGP_COV_RELU, False)), 2),
        "cov_conv_relu_add": (byref(cov_conv, conv_args(N.CGP_COV_RELU, True)), 3),
        "cov_relu": (byref(cov_nonlin, nonlin_args(N.CGP_COV_RELU)), 2),
        "cov_erf": (byref(cov_nonlin, nonlin_args(N.CGP_COV_ERF)), 2),
        "cov_pool": (lambda: N.call(f"cgp_cov_pool_{sfx}", N.ptr(s), pairs, n, N.ptr(pooled),
                                    stream), 1),
        "layer_relu": (byref(relu, r), 2),
        "layer_conv": (byref(conv, c), 2),
    }
    times = timed_interleaved({k: fn for k, (fn, _) in passes.items()}, reps, inner)
    return {k: dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                    gbps=round(passes[k][1] * gb / (med / 1e3), 1))
            for k, (med, lo, hi) in times.items()}


def pooled_convnet():
    cfg = importlib.import_module("configs.mnist_paper_convnet_gp")
    mods = [cnn_gp.ReLU() if isinstance(m, cnn_gp.ReLU) else
            cnn_gp.Conv2d(m.kernel_size, stride=m.stride, padding=m._padding_arg,
                          var_weight=m.var_weight, var_bias=m.var_bias)
            for m in cfg.initial_model.mods[:-1]]
    return cnn_gp.Sequential(*mods, cnn_gp.GlobalAvgPool())


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
        model = pooled_convnet().to("cuda", dt)
        with torch.no_grad():
            med, lo, hi = timed(lambda: model(x, y, False, False), args.reps)
        print(json.dumps(dict(config="mnist_paper_convnet_gp body + GlobalAvgPool", dtype=name,
                              tile=B, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                              pairs_per_s=round(B * B / (med / 1e3), 1))), flush=True)


if __name__ == "__main__":
    main()
