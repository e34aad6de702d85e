"""Timing of the sinusoid family (cgp_sin_*, cgp_sin_cov_*) on one off-diagonal tile, HIP
events, all in one process: the Sin, Cos and Rbf passes beside the Erf and Gelu passes that
move the same bytes, on the same buffers --

    256 x 256 pair maps of 28x28:      cgp_sin_* forward       vs cgp_erf_*, cgp_gelu_*
                                       cgp_sin_* with Θ        vs cgp_erf_*, cgp_gelu_* with Θ
    64 position-pair maps of 28x28:    cgp_sin_cov_* forward   vs cgp_cov_nonlin_* (ERF),
    (614 656 elements per pair)                                   cgp_gelu_cov_*
                                       cgp_sin_cov_* with Θ    vs cgp_covntk_nonlin_* (ERF, GELU)

float64 and float32, Sin(1.5, 2, 0.3), Cos(1, 2) and Rbf(0.5) (one exponential instead of two),
with the HBM bandwidth each achieves over its map passes (forward: 1 read + 1 write; with Θ:
2 + 2; the per-image variance maps are small and L2-resident, not counted).

tools/abrelu_bench.py's method: the passes are timed interleaved.  After a warm-up of every
pass, ``--reps`` rounds each time every pass once, as ``--inner`` back-to-back launches
between two events.  Every figure is the per-launch median over the rounds with the fastest
and slowest round beside it.  ``vs_erf`` / ``vs_gelu`` is a new pass's median over that
yardstick's, and ``erf_spread`` / ``gelu_spread`` the yardstick's slowest round over its
fastest: a ratio inside the spread is not a difference.

    python tools/sin_bench.py [--tile 256] [--pairs 64] [--reps 9] [--inner 20]
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

import torch  # noqa: E402

from abrelu_bench import timed_interleaved  # noqa: E402
from cnn_gp import _native as N  # noqa: E402

# name -> (A, B, C, D) = (a²/2, b²/2, cos 2θ, a²b²/2)
CONSTS = {"sin": (1.125, 2.0, math.cos(0.6), 4.5), "cos": (0.5, 2.0, -1.0, 2.0),
          "rbf": (1.0, 0.5, 0.0, 1.0)}


def report(passes, gb, reps, inner, stream):
    """passes: name -> (entry point, arguments, map passes); a name ending in "_ntk" is
    compared with erf_ntk / gelu_ntk, any other with erf / gelu"""
    fns = {k: (lambda fn=fn, s=s, k=k: N.check(fn(ctypes.byref(s), stream), k))
           for k, (fn, s, _) in passes.items()}
    times = timed_interleaved(fns, reps, inner)
    res = {k: dict(ms=med, min_ms=lo, max_ms=hi, gbps=passes[k][2] * gb / (med / 1e3))
           for k, (med, lo, hi) in times.items()}
    for k in res:
        if k.split("_")[0] not in CONSTS:
            continue
        tail = "_ntk" if k.endswith("_ntk") else ""
        for y in ("erf", "gelu"):
            res[k]["vs_" + y] = res[k]["ms"] / res[y + tail]["ms"]
            res[k][y + "_spread"] = res[y + tail]["max_ms"] / res[y + tail]["min_ms"]
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

    def fill(e, theta):
        e.xy, e.out_xy, e.out_theta = N.ptr(xy), N.ptr(out), N.ptr(tout)
        e.xx, e.yy = N.ptr(vx), N.ptr(vy)
        e.nmaps, e.n1, e.n2, e.hw = n * n, n, n, hw
        if theta:
            e.theta = N.ptr(th)
        return e
    fn = lambda k: getattr(lib, f"cgp_{k}_{sfx}")                                # noqa: E731
    passes = {}
    for name, k4 in CONSTS.items():
        for theta in (False, True):
            e = fill(N.SinArgs(), theta)
            e.A, e.B, e.C, e.D = k4
            passes[name + ("_ntk" if theta else "")] = (fn("sin"), e, 4 if theta else 2)
    for name, rec in (("erf", N.ErfArgs), ("gelu", N.GeluArgs)):
        for theta in (False, True):
            passes[name + ("_ntk" if theta else "")] = (fn(name), fill(rec(), theta),
                                                        4 if theta else 2)
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
    fn = lambda k: getattr(lib, f"cgp_{k}_{sfx}")                                # noqa: E731
    passes = {}
    for name, k4 in CONSTS.items():
        for theta in (False, True):
            q = fill(N.SinCovArgs(), theta)
            q.A, q.B, q.C, q.D = k4
            passes[name + ("_ntk" if theta else "")] = (fn("sin_cov"), q, 4 if theta else 2)
    c = fill(N.CovNonlinArgs(), False)
    c.kind = N.CGP_COV_ERF
    passes["erf"] = (fn("cov_nonlin"), c, 2)
    passes["gelu"] = (fn("gelu_cov"), fill(N.GeluCovArgs(), False), 2)
    for name, kind in (("erf_ntk", N.CGP_COV_ERF), ("gelu_ntk", N.CGP_COV_GELU)):
        ct = fill(N.CovNonlinNtkArgs(), True)
        ct.kind = kind
        passes[name] = (fn("covntk_nonlin"), ct, 4)
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
        print(json.dumps(dict(op="28x28 pair maps", dtype=name, tile=args.tile, consts=CONSTS,
                              **ops(args.tile, 784, args.reps, args.inner, dt))), flush=True)
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 position-pair maps", dtype=name, pairs=args.pairs,
                              consts=CONSTS,
                              **cov_ops(args.pairs, 28, args.reps, args.inner, dt))),
              flush=True)


if __name__ == "__main__":
    main()
