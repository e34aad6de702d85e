"""Timing of the neural tangent kernel on one off-diagonal tile, HIP events, fp64:
model.ntk against the layer-path NNGP forward (set_fused_network(False)), and
cgp_relu_ntk_f64 alone against cgp_relu_f64 alone on the tile's largest pair maps, with
the HBM bandwidth each achieves over its pair-map passes (relu_ntk: K and Θ read, K' and
Θ' written = 4; relu: 1 + 1; the per-image variance maps are 1/128 of a pair map at this
tile and L2-resident, not counted).

    python tools/ntk_bench.py [--tile 256] [--reps 5] [--configs a,b]
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

from cnn_gp import _native as N  # noqa: E402


def timed(fn, reps):
    """median of `reps` event-timed calls after one warm call, ms"""
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
    return sorted(out)[len(out) // 2]


def relu_ops(n, hw, reps):
    """cgp_relu_f64 and cgp_relu_ntk_f64 on n x n pair maps of hw pixels"""
    g = torch.Generator(device="cuda").manual_seed(1)
    vx = torch.rand((n, hw), dtype=torch.float64, device="cuda", generator=g) + 0.5
    vy = torch.rand((n, hw), dtype=torch.float64, device="cuda", generator=g) + 0.5
    rho = torch.rand((n, n, hw), dtype=torch.float64, device="cuda", generator=g) * 1.9 - 0.95
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
    res = {}
    for flags, tag in ((0, "fast"), (N.CGP_FLAG_EXACT_RELU, "exact")):
        r.flags = a.flags = flags
        t_relu = timed(lambda: N.check(lib.cgp_relu_f64(ctypes.byref(r), stream), "relu"), reps)
        t_ntk = timed(lambda: N.check(lib.cgp_relu_ntk_f64(ctypes.byref(a), stream), "relu_ntk"),
                      reps)
        gb = xy.numel() * 8 / 1e9
        res[tag] = dict(relu_ms=t_relu, relu_ntk_ms=t_ntk, ratio=t_ntk / t_relu,
                        relu_gbps=2 * gb / (t_relu / 1e3), relu_ntk_gbps=4 * gb / (t_ntk / 1e3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="mnist_paper_convnet_gp,mnist_as_tf")
    args = ap.parse_args()
    B = args.tile
    for name in args.configs.split(","):
        cfg = importlib.import_module(f"configs.{name}")
        model = cfg.initial_model.to("cuda", torch.float64)
        g = torch.Generator().manual_seed(0)
        x = torch.rand((B, 1, 28, 28), generator=g, dtype=torch.float64).cuda()
        y = torch.rand((B, 1, 28, 28), generator=g, dtype=torch.float64).cuda()
        with torch.no_grad():
            t_ntk = timed(lambda: model.ntk(x, y, False, False), args.reps)
            t_fused = timed(lambda: model(x, y, False, False), args.reps)
            model.set_fused_network(False)
            t_layer = timed(lambda: model(x, y, False, False), args.reps)
            model.set_fused_network(True)
        print(json.dumps(dict(config=name, tile=B, ntk_ms=t_ntk, layer_nngp_ms=t_layer,
                              fused_nngp_ms=t_fused, ntk_over_layer=t_ntk / t_layer)),
              flush=True)
    print(json.dumps(dict(op="relu 28x28", tile=B, **relu_ops(B, 784, args.reps))), flush=True)


if __name__ == "__main__":
    main()
