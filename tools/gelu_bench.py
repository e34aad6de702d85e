"""Timing of the GELU nonlinearity on one off-diagonal tile, HIP events, all in one process:
cgp_gelu_* alone (forward-only and with Θ) beside cgp_erf_* and cgp_relu_* / cgp_relu_ntk_*
(closed form) as yardsticks, on the same 256 x 256 pair maps of 28x28, float64 and float32,
with the HBM bandwidth each achieves over its pair-map passes (forward: 1 read + 1 write;
with Θ: 2 + 2; the per-image variance maps are 1/128 of a pair map at this tile and
L2-resident, not counted); then one cgp_gelu_cov_* pass beside cgp_cov_nonlin_* erf on 64
position-pair maps of 28x28 (614 656 elements per pair).

tools/erf_bench.py's method: the passes are timed interleaved.  After a warm-up of every
pass, ``--reps`` rounds each time every pass once, as ``--inner`` back-to-back launches
between two events.  Every figure is the per-launch median over the rounds with the fastest
and slowest round beside it; the comparator for cgp_gelu_* is cgp_erf_* of the same call, and
the spread of the yardstick's own rounds is the margin.

    python tools/gelu_bench.py [--tile 256] [--pairs 64] [--reps 9] [--inner 20]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

import torch  # noqa: E402

from cnn_gp import _native as N  # noqa: E402


def timed_interleaved(fns, reps, inner):
    """name -> (median, min, max) ms per launch: every fn warmed, then `reps` rounds that
    time each fn once over `inner` back-to-back calls"""
    for fn in fns.values():
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / inner)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in out.items()}


def report(passes, gb, reps, inner, stream):
    """passes: name -> (entry point, arguments, pair-map passes)"""
    fns = {k: (lambda fn=fn, s=s, k=k: N.check(fn(ctypes.byref(s), stream), k))
           for k, (fn, s, _) in passes.items()}
    times = timed_interleaved(fns, reps, inner)
    return {k: dict(ms=med, min_ms=lo, max_ms=hi, gbps=passes[k][2] * gb / (med / 1e3))
            for k, (med, lo, hi) in times.items()}


def ops(n, hw, reps, inner, dt):
    """the pointwise passes on n x n pair maps of hw pixels in dtype dt"""
    sfx = "f64" if dt == torch.float64 else "f32"
    g = torch.Generator(device="cuda").manual_seed(1)
    vx = torch.rand((n, hw), dtype=dt, device="cuda", generator=g) + 0.5
    vy = torch.rand((n, hw), dtype=dt, device="cuda", generator=g) + 0.5
    rho = torch.rand((n, n, hw), dtype=dt, device="cuda", generator=g) * 1.9 - 0.95
    xy = (rho * torch.sqrt(vx[:, None] * vy[None])).view(n * n, hw)
    del rho
    th = torch.rand_like(xy)
    out, tout = torch.empty_like(xy), torch.empty_like(xy)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    r = N.ReluArgs()
    r.xy, r.out, r.xx, r.yy = N.ptr(xy), N.ptr(out), N.ptr(vx), N.ptr(vy)
    r.nmaps, r.n1, r.n2, r.hw = n * n, n, n, hw
    a = N.ReluNtkArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(xy), N.ptr(th), N.ptr(out), N.ptr(tout)
    a.xx, a.yy = N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2, a.hw = n * n, n, n, hw

    def pointwise(cls):
        e = cls()
        e.xy, e.out_xy, e.out_theta = N.ptr(xy), N.ptr(out), N.ptr(tout)
        e.xx, e.yy = N.ptr(vx), N.ptr(vy)
        e.nmaps, e.n1, e.n2, e.hw = n * n, n, n, hw
        et = cls.from_buffer_copy(e)
        et.theta = N.ptr(th)
        return e, et
    e, et = pointwise(N.ErfArgs)
    ge, get = pointwise(N.GeluArgs)
    fn = lambda k: getattr(lib, f"cgp_{k}_{sfx}")                                # noqa: E731
    passes = {"gelu": (fn("gelu"), ge, 2), "gelu_ntk": (fn("gelu"), get, 4),
              "erf": (fn("erf"), e, 2), "erf_ntk": (fn("erf"), et, 4),
              "relu": (fn("relu"), r, 2), "relu_ntk": (fn("relu_ntk"), a, 4)}
    gb = xy.numel() * xy.element_size() / 1e9
    return report(passes, gb, reps, inner, stream)


def cov_ops(npairs, side, reps, inner, dt):
    """one pass over npairs position-pair maps of side x side, every pair (i, j), i != j"""
    sfx = "f64" if dt == torch.float64 else "f32"
    hw = side * side
    nimg = 16
    g = torch.Generator(device="cuda").manual_seed(2)
    vx = torch.rand((nimg, hw), dtype=dt, device="cuda", generator=g) + 0.5
    vy = torch.rand((nimg, hw), dtype=dt, device="cuda", generator=g) + 0.5
    pi = (torch.arange(npairs, device="cuda") % nimg).to(torch.int32)
    pj = ((torch.arange(npairs, device="cuda") * 7 + 3) % nimg).to(torch.int32)
    s = torch.empty((npairs, hw, hw), dtype=dt, device="cuda")
    for m in range(npairs):                                  # |rho| <= 0.95, pair by pair
        rho = torch.rand((hw, hw), dtype=dt, device="cuda", generator=g) * 1.9 - 0.95
        s[m] = rho * torch.sqrt(vx[pi[m]][:, None] * vy[pj[m]][None])
    out = torch.empty_like(s)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    c = N.CovNonlinArgs()
    c.in_, c.out, c.xx, c.yy = N.ptr(s), N.ptr(out), N.ptr(vx), N.ptr(vy)
    c.pair_i, c.pair_j, c.npairs = N.ptr(pi), N.ptr(pj), npairs
    c.h, c.w, c.kind = side, side, N.CGP_COV_ERF
    q = N.GeluCovArgs()
    q.in_, q.out, q.xx, q.yy = N.ptr(s), N.ptr(out), N.ptr(vx), N.ptr(vy)
    q.pair_i, q.pair_j, q.npairs = N.ptr(pi), N.ptr(pj), npairs
    q.h, q.w = side, side
    passes = {"gelu_cov": (getattr(lib, f"cgp_gelu_cov_{sfx}"), q, 2),
              "cov_nonlin_erf": (getattr(lib, f"cgp_cov_nonlin_{sfx}"), c, 2)}
    gb = s.numel() * s.element_size() / 1e9
    return report(passes, gb, reps, inner, stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 pair maps", dtype=name, tile=args.tile,
                              **ops(args.tile, 784, args.reps, args.inner, dt))), flush=True)
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 position-pair maps", dtype=name, pairs=args.pairs,
                              **cov_ops(args.pairs, 28, args.reps, args.inner, dt))),
              flush=True)


if __name__ == "__main__":
    main()
