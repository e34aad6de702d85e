"""Timing of the erf nonlinearity on one off-diagonal tile, HIP events, all in one process:
cgp_erf_* alone (forward-only and with Θ) against cgp_relu_* / cgp_relu_ntk_* alone in
both ReLU modes, on the same 28x28 pair maps, float64 and float32, with the HBM bandwidth
each achieves over its pair-map passes (forward: 1 read + 1 write; with Θ: 2 + 2; the
per-image variance maps are 1/128 of a pair map at this tile and L2-resident, not
counted); then one erf ConvNet (configs/mnist_paper_convnet_gp.py with every ReLU replaced
by Erf) through forward and ntk beside the ReLU ConvNet's layer path.

The pointwise passes are timed interleaved: after a warm-up of every pass, ``--reps``
rounds each time every pass once, as ``--inner`` back-to-back launches between two events.
Every figure is the per-launch median over the rounds with the fastest and slowest round
beside it: the comparator for cgp_erf_* forward is cgp_relu_* with CGP_FLAG_EXACT_RELU, and
the spread of its own rounds is the margin.

    python tools/erf_bench.py [--tile 256] [--reps 9] [--inner 20]
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


def timed(fn, reps):
    """(median, min, max) of `reps` event-timed calls after one warm call, ms"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


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


def ops(n, hw, reps, inner, dt):
    """the three pointwise passes on n x n pair maps of hw pixels in dtype dt"""
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
    e = N.ErfArgs()
    e.xy, e.out_xy, e.out_theta = N.ptr(xy), N.ptr(out), N.ptr(tout)
    e.xx, e.yy = N.ptr(vx), N.ptr(vy)
    e.nmaps, e.n1, e.n2, e.hw = n * n, n, n, hw
    relu, relu_ntk, erf = (getattr(lib, f"cgp_{k}_{sfx}") for k in ("relu", "relu_ntk", "erf"))
    gb = xy.numel() * xy.element_size() / 1e9

    ea, rf, rx, af, ax = (type(v).from_buffer_copy(v) for v in (e, r, r, a, a))
    ea.theta = N.ptr(th)
    rx.flags = ax.flags = N.CGP_FLAG_EXACT_RELU
    # name -> (entry point, arguments, pair-map passes)
    passes = {"erf": (erf, e, 2), "erf_ntk": (erf, ea, 4),
              "relu_fast": (relu, rf, 2), "relu_ntk_fast": (relu_ntk, af, 4),
              "relu_exact": (relu, rx, 2), "relu_ntk_exact": (relu_ntk, ax, 4)}
    fns = {k: (lambda fn=fn, s=s, k=k: N.check(fn(ctypes.byref(s), stream), k))
           for k, (fn, s, _) in passes.items()}
    times = timed_interleaved(fns, reps, inner)
    return {k: dict(ms=med, min_ms=lo, max_ms=hi, gbps=passes[k][2] * gb / (med / 1e3))
            for k, (med, lo, hi) in times.items()}


def erf_convnet():
    cfg = importlib.import_module("configs.mnist_paper_convnet_gp")
    mods = [cnn_gp.Erf() if isinstance(m, cnn_gp.ReLU) else
            cnn_gp.Conv2d(m.kernel_size, stride=m.stride, padding=m._padding_arg,
                          var_weight=m.var_weight, var_bias=m.var_bias)
            for m in cfg.initial_model.mods]
    return cnn_gp.Sequential(*mods), cfg.initial_model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    B = args.tile
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        print(json.dumps(dict(op="28x28 pair maps", dtype=name, tile=B,
                              **ops(B, 784, args.reps, args.inner, dt))), flush=True)
    erf_model, relu_model = erf_convnet()
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        g = torch.Generator().manual_seed(0)
        x = torch.rand((B, 1, 28, 28), generator=g, dtype=dt).cuda()
        y = torch.rand((B, 1, 28, 28), generator=g, dtype=dt).cuda()
        row = dict(config="mnist_paper_convnet_gp", dtype=name, tile=B)
        with torch.no_grad():
            for tag, model in (("erf", erf_model), ("relu", relu_model)):
                model = model.to("cuda", dt).set_fused_network(False)
                row[tag + "_forward_ms"] = timed(lambda: model(x, y, False, False), args.reps)[0]
                row[tag + "_ntk_ms"] = timed(lambda: model.ntk(x, y, False, False), args.reps)[0]
                model.set_fused_network(True)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
