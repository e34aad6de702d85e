"""Timing of the Hermite-series nonlinearity (cgp_hermite_coef_*, cgp_hermite_*) on one
off-diagonal tile, HIP events, all in one process: at order 8, 16, 32 and 64 the coefficient
kernel over the tile's 2 x 256 variance maps (the tables of φ alone, and of φ and φ'), the
forward walk and the walk with Θ, beside the Erf passes that move the same map bytes on the
same buffers --

    256 x 256 pair maps of 28x28:   cgp_hermite_coef_* (a; a and a')
                                    cgp_hermite_* forward       vs cgp_erf_*
                                    cgp_hermite_* with Θ        vs cgp_erf_* with Θ

float64 and float32, tanh at 96 nodes.  ``gbps`` is the HBM bandwidth over the map passes
(forward: 1 read + 1 write; with Θ: 2 + 2); ``table_gb`` the bytes of coefficients an element
walk loads through L2 and L1 per launch (2·(order + 1) values per element, twice that with Θ),
and ``table_gbps`` that over the time: the tables themselves are (order + 1) x 2 x 256 x 784
values, small next to the maps, so these loads hit in cache.

tools/abrelu_bench.py's method: the passes are timed interleaved.  After a warm-up of every
pass, ``--reps`` rounds each time every pass once, as ``--inner`` back-to-back launches between
two events.  Every figure is the per-launch median over the rounds with the fastest and slowest
round beside it.  ``vs_erf`` is a walk's median over the erf pass's, and ``erf_spread`` the erf
pass's slowest round over its fastest: a ratio inside the spread is not a difference.

    python tools/hermite_bench.py [--tile 256] [--reps 9] [--inner 10]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

import torch  # noqa: E402

from abrelu_bench import timed_interleaved  # noqa: E402
from cnn_gp import _native as N  # noqa: E402
from cnn_gp.program import Plan  # noqa: E402

ORDERS = (8, 16, 32, 64)
PHI, NODES = "tanh", 96


def ops(n, hw, reps, inner, dt):
    """the passes on n x n pair maps of hw pixels in dtype dt"""
    sfx = "f64" if dt == torch.float64 else "f32"
    g = torch.Generator(device="cuda").manual_seed(1)
    var = torch.rand((2 * n, hw), dtype=dt, device="cuda", generator=g) + 0.5
    vx, vy = var[:n], var[n:]
    rho = torch.rand((n, n, hw), dtype=dt, device="cuda", generator=g) * 1.9 - 0.95
    xy = (rho * torch.sqrt(vx[:, None] * vy[None])).view(n * n, hw)
    del rho
    th = torch.rand_like(xy)
    out, tout = torch.empty_like(xy), torch.empty_like(xy)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    nodes = Plan._hermite_nodes(xy.device, NODES)
    count = 2 * n * hw                                       # one table over xx and yy
    item = xy.element_size()

    def fill(e, theta):
        e.xy, e.out_xy, e.out_theta = N.ptr(xy), N.ptr(out), N.ptr(tout)
        e.xx, e.yy = N.ptr(vx), N.ptr(vy)
        e.nmaps, e.n1, e.n2, e.hw = n * n, n, n, hw
        if theta:
            e.theta = N.ptr(th)
        return e
    fn = lambda k: getattr(lib, f"cgp_{k}_{sfx}")                                # noqa: E731
    passes, tables, loads = {}, [], {}
    for order in ORDERS:
        a = torch.empty((2, order + 1, count), dtype=dt, device="cuda")
        tables.append(a)
        for deriv in (False, True):
            c = N.HermiteCoefArgs()
            c.var, c.a, c.nodes, c.count = N.ptr(var), a[0].data_ptr(), N.ptr(nodes), count
            c.da = a[1].data_ptr() if deriv else None
            c.phi, c.order, c.nq = N.HERMITE_PHI[PHI], order, NODES
            passes[f"coef{order}" + ("_da" if deriv else "")] = (fn("hermite_coef"), c)
        for theta in (False, True):
            e = fill(N.HermiteArgs(), theta)
            e.ax, e.ay = a[0].data_ptr(), a[0].data_ptr() + n * hw * item
            e.dax, e.day = a[1].data_ptr(), a[1].data_ptr() + n * hw * item
            e.stride_x = e.stride_y = count
            e.order = order
            name = f"hermite{order}" + ("_ntk" if theta else "")
            passes[name] = (fn("hermite"), e)
            loads[name] = (4 if theta else 2) * (order + 1) * xy.numel() * item / 1e9
    for theta in (False, True):
        passes["erf" + ("_ntk" if theta else "")] = (fn("erf"), fill(N.ErfArgs(), theta))
    fns = {k: (lambda f=f, s=s, k=k: N.check(f(ctypes.byref(s), stream), k))
           for k, (f, s) in passes.items()}
    times = timed_interleaved(fns, reps, inner)
    gb = xy.numel() * item / 1e9
    res = {}
    for k, (med, lo, hi) in times.items():
        res[k] = dict(ms=med, min_ms=lo, max_ms=hi)
        if k.startswith("coef"):
            continue
        tail = "_ntk" if k.endswith("_ntk") else ""
        res[k]["gbps"] = (4 if tail else 2) * gb / (med / 1e3)
        if k in loads:
            erf = times["erf" + tail]
            res[k].update(table_gb=loads[k], table_gbps=loads[k] / (med / 1e3),
                          vs_erf=med / erf[0], erf_spread=erf[2] / erf[1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 pair maps", dtype=name, tile=args.tile, phi=PHI,
                              nodes=NODES, **ops(args.tile, 784, args.reps, args.inner, dt))),
              flush=True)


if __name__ == "__main__":
    main()
