"""Timing of the NTK kernels on position-pair maps (csrc/covntk.hip), HIP events, all in one
process, with tools/pool_bench.py's method: ``--pairs`` position-pair maps of 28x28 images
((28·28)² = 614 656 elements per pair), the passes timed interleaved -- after a warm-up of
every pass, ``--reps`` rounds each time every pass once, as ``--inner`` back-to-back launches
between two events -- and every figure the per-launch median over the rounds with the fastest
and slowest round beside it.

* cgp_covntk_nonlin_* per kind (4 map passes: K, Θ in, K', Θ' out) against the forward-only
  cgp_cov_nonlin_* / cgp_gelu_cov_* (2 passes); ``gbps`` is over those algorithmic bytes.
* cgp_covntk_conv_* (3x3 "same", post ReLU: 4 passes) against its own launch-by-launch
  sequence in the same call: cgp_cov_conv_* on K, cgp_cov_conv_* on Θ with bias 0 and addend
  K', cgp_covntk_nonlin_* (2 + 3 + 4 = 9 passes).  ``fused_wins`` says whether the fused
  median is faster than the sequence's by more than the fastest-slowest spread of the two.
* ntk_maps of the README's GAP net and Myrtle net on a ``--tile`` x ``--tile`` block of
  28x28 images with the fused lowering on and off (set_ntk_maps_fusion), pairs/s.

    python tools/pool_ntk_bench.py [--pairs 64] [--tile 8] [--reps 9] [--inner 5]
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


def kernels(pairs, side, reps, inner, dt):
    sfx = "f64" if dt == torch.float64 else "f32"
    hw = side * side
    n = hw * hw
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *s: torch.rand(s, dtype=dt, device="cuda", generator=g)        # noqa: E731
    pi = torch.arange(pairs, dtype=torch.int32, device="cuda")
    vx, vy = rand(pairs, hw) + 0.5, rand(pairs, hw) + 0.5
    s, th = rand(pairs, n) * 0.9, rand(pairs, n)
    out, tout, kp, tp = (torch.empty_like(s) for _ in range(4))
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    gb = s.numel() * s.element_size() / 1e9

    def pairs_of(a):
        a.xx, a.yy = N.ptr(vx), N.ptr(vy)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pi), pairs
        return a

    def geometry(a, bias):
        a.npairs = pairs
        a.h = a.w = a.ho = a.wo = side
        a.taps, a.offset, a.stride, a.dilation = 3, -1, 1, 1
        a.weight, a.bias = 1 / 9, bias
        return a

    def nonlin(kind):
        a = pairs_of(N.GeluCovArgs() if kind == N.CGP_COV_GELU else N.CovNonlinArgs())
        a.in_, a.out = N.ptr(s), N.ptr(out)
        a.h = a.w = side
        if kind != N.CGP_COV_GELU:
            a.kind = kind
        return a

    def nonlin_ntk(kind, src=s, theta=th):
        a = pairs_of(N.CovNonlinNtkArgs())
        a.in_, a.theta, a.out, a.out_theta = N.ptr(src), N.ptr(theta), N.ptr(out), N.ptr(tout)
        a.h = a.w = side
        a.kind = kind
        return a

    fused = geometry(pairs_of(N.CovConvNtkArgs()), 0.1)
    fused.in_, fused.theta, fused.out, fused.out_theta = N.ptr(s), N.ptr(th), N.ptr(out), \
        N.ptr(tout)
    fused.post = N.CGP_COV_RELU
    conv_k = geometry(N.CovConvArgs(), 0.1)
    conv_k.in_, conv_k.out = N.ptr(s), N.ptr(kp)
    conv_t = geometry(N.CovConvArgs(), 0.0)
    conv_t.in_, conv_t.out, conv_t.addend = N.ptr(th), N.ptr(tp), N.ptr(kp)
    step = nonlin_ntk(N.CGP_COV_RELU, kp, tp)

    fn = lambda name: getattr(lib, f"{name}_{sfx}")                              # noqa: E731
    byref = lambda f, a: (lambda: N.check(f(ctypes.byref(a), stream), "bench"))  # noqa: E731
    cov_conv, cov_step = fn("cgp_cov_conv"), fn("cgp_covntk_nonlin")

    def sequence():
        N.check(cov_conv(ctypes.byref(conv_k), stream), "bench")
        N.check(cov_conv(ctypes.byref(conv_t), stream), "bench")
        N.check(cov_step(ctypes.byref(step), stream), "bench")

    # name -> (launch, map passes over HBM)
    passes = {}
    for name, kind in (("relu", N.CGP_COV_RELU), ("erf", N.CGP_COV_ERF),
                       ("gelu", N.CGP_COV_GELU)):
        fwd = fn("cgp_gelu_cov") if kind == N.CGP_COV_GELU else fn("cgp_cov_nonlin")
        passes[f"cov_{name}"] = (byref(fwd, nonlin(kind)), 2)
        passes[f"cov_{name}_ntk"] = (byref(cov_step, nonlin_ntk(kind)), 4)
    passes["cov_conv_relu_ntk"] = (byref(fn("cgp_covntk_conv"), fused), 4)
    passes["cov_conv_relu_ntk_sequence"] = (sequence, 9)
    times = timed_interleaved({k: f for k, (f, _) in passes.items()}, reps, inner)
    res = {k: dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                   gbps=round(passes[k][1] * gb / (med / 1e3), 1))
           for k, (med, lo, hi) in times.items()}
    (fm, flo, fhi), (sm, slo, shi) = times["cov_conv_relu_ntk"], \
        times["cov_conv_relu_ntk_sequence"]
    res["fused_over_sequence"] = round(fm / sm, 3)
    res["fused_wins"] = bool(sm - fm > max(fhi - flo, shi - slo))
    return res


def readme_nets():
    m = cnn_gp
    C, R, G, A = m.Conv2d, m.ReLU, m.GlobalAvgPool, m.AvgPool2d
    return {
        "gap_net": lambda: m.Sequential(C(3, var_bias=0.1), R(), C(3), R(), G(),
                                        C(1, var_weight=2.0, var_bias=0.3)),
        "myrtle": lambda: m.Sequential(C(3, var_bias=0.1), R(), C(3), R(), A(2), C(3), R(), A(2),
                                       G(), C(1, var_weight=2.0, var_bias=0.3)),
    }


def networks(tile, reps, dt):
    g = torch.Generator().manual_seed(0)
    x = torch.rand((tile, 1, 28, 28), generator=g, dtype=dt).cuda()
    y = torch.rand((tile, 1, 28, 28), generator=g, dtype=dt).cuda()
    fns = {}
    for name, make in readme_nets().items():
        for fused in (True, False):
            model = make().to("cuda", dt).set_ntk_maps_fusion(fused)
            fns[f"{name}_{'fused' if fused else 'sequence'}"] = \
                (lambda model=model: model.ntk_maps(x, y, False, False))
    with torch.no_grad():
        times = timed_interleaved(fns, reps, 1)
    return {k: dict(ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                    pairs_per_s=round(tile * tile / (med / 1e3), 1))
            for k, (med, lo, hi) in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--tile", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 position-pair maps, K and Θ", dtype=name,
                              pairs=args.pairs,
                              **kernels(args.pairs, 28, args.reps, args.inner, dt))), flush=True)
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="ntk_maps, 28x28 images", dtype=name, tile=args.tile,
                              **networks(args.tile, args.reps, dt))), flush=True)


if __name__ == "__main__":
    main()
