"""Timing of the two-slope ReLU (cgp_abrelu_*, cgp_abrelu_cov_*) on one off-diagonal tile, HIP
events, all in one process: each new pass beside the ReLU pass that moves the same bytes, on
the same buffers --

    256 x 256 pair maps of 28x28:      cgp_abrelu_* forward          vs cgp_relu_*
                                       cgp_abrelu_* with Θ           vs cgp_relu_ntk_*
    64 position-pair maps of 28x28:    cgp_abrelu_cov_* forward      vs cgp_cov_nonlin_* (RELU)
    (614 656 elements per pair)        cgp_abrelu_cov_* with Θ       vs cgp_covntk_nonlin_* (RELU)

float64 and float32, closed-form ReLU, slopes (0.01, 1), with the HBM bandwidth each achieves
over its map passes (forward: 1 read + 1 write; with Θ: 2 + 2; the per-image variance maps are
small and L2-resident, not counted).

tools/gelu_bench.py's method: the passes are timed interleaved.  After a warm-up of every
pass, ``--reps`` rounds each time every pass once, as ``--inner`` back-to-back launches
between two events.  Every figure is the per-launch median over the rounds with the fastest
and slowest round beside it.  ``ratio`` is a new pass's median over its yardstick's, and
``yardstick_spread`` the yardstick's slowest round over its fastest: a ratio inside the spread
is not a difference.

    python tools/abrelu_bench.py [--tile 256] [--pairs 64] [--reps 9] [--inner 20]
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

SLOPES = (0.01, 1.0)
# new pass -> its ReLU yardstick
YARDSTICK = {"abrelu": "relu", "abrelu_ntk": "relu_ntk", "abrelu_cov": "cov_nonlin_relu",
             "abrelu_cov_ntk": "covntk_nonlin_relu"}


def smh():
    a, b = SLOPES
    return (a - b) * (a - b), a * b, (a * a + b * b) / 2


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
    """passes: name -> (entry point, arguments, map passes)"""
    fns = {k: (lambda fn=fn, s=s, k=k: N.check(fn(ctypes.byref(s), stream), k))
           for k, (fn, s, _) in passes.items()}
    times = timed_interleaved(fns, reps, inner)
    res = {k: dict(ms=med, min_ms=lo, max_ms=hi, gbps=passes[k][2] * gb / (med / 1e3))
           for k, (med, lo, hi) in times.items()}
    for k, y in YARDSTICK.items():
        if k in res:
            res[k]["ratio"] = res[k]["ms"] / res[y]["ms"]
            res[k]["yardstick_spread"] = res[y]["max_ms"] / res[y]["min_ms"]
    return res


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
    e = N.ABReluArgs()
    e.xy, e.out_xy, e.out_theta = N.ptr(xy), N.ptr(out), N.ptr(tout)
    e.xx, e.yy = N.ptr(vx), N.ptr(vy)
    e.nmaps, e.n1, e.n2, e.hw = n * n, n, n, hw
    e.s, e.m, e.h = smh()
    et = N.ABReluArgs.from_buffer_copy(e)
    et.theta = N.ptr(th)
    fn = lambda k: getattr(lib, f"cgp_{k}_{sfx}")                                # noqa: E731
    passes = {"abrelu": (fn("abrelu"), e, 2), "abrelu_ntk": (fn("abrelu"), et, 4),
              "relu": (fn("relu"), r, 2), "relu_ntk": (fn("relu_ntk"), a, 4)}
    gb = xy.numel() * xy.element_size() / 1e9
    return report(passes, gb, reps, inner, stream)


def cov_ops(npairs, side, reps, inner, dt):
    """the passes over npairs position-pair maps of side x side, every pair (i, j), i != j"""
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
    th = torch.rand_like(s)
    out, tout = torch.empty_like(s), torch.empty_like(s)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()

    def fill(q, theta):
        q.in_, q.out, q.xx, q.yy = N.ptr(s), N.ptr(out), N.ptr(vx), N.ptr(vy)
        q.pair_i, q.pair_j, q.npairs = N.ptr(pi), N.ptr(pj), npairs
        q.h, q.w = side, side
        if theta:
            q.theta, q.out_theta = N.ptr(th), N.ptr(tout)
        return q
    c = fill(N.CovNonlinArgs(), False)
    c.kind = N.CGP_COV_RELU
    ct = fill(N.CovNonlinNtkArgs(), True)
    ct.kind = N.CGP_COV_RELU
    q, qt = fill(N.ABReluCovArgs(), False), fill(N.ABReluCovArgs(), True)
    q.s, q.m, q.hh = qt.s, qt.m, qt.hh = smh()
    fn = lambda k: getattr(lib, f"cgp_{k}_{sfx}")                                # noqa: E731
    passes = {"abrelu_cov": (fn("abrelu_cov"), q, 2), "abrelu_cov_ntk": (fn("abrelu_cov"), qt, 4),
              "cov_nonlin_relu": (fn("cov_nonlin"), c, 2),
              "covntk_nonlin_relu": (fn("covntk_nonlin"), ct, 4)}
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
        print(json.dumps(dict(op="28x28 pair maps", dtype=name, tile=args.tile, slopes=SLOPES,
                              **ops(args.tile, 784, args.reps, args.inner, dt))), flush=True)
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 position-pair maps", dtype=name, pairs=args.pairs,
                              slopes=SLOPES,
                              **cov_ops(args.pairs, 28, args.reps, args.inner, dt))),
              flush=True)


if __name__ == "__main__":
    main()
