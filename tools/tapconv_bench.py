"""Timing of convs whose taps carry individual weights (csrc/tapconv.hip), HIP
events, all in one process, by the method of tools/corrconv_bench.py.

Layer path, on ``--maps`` maps of 28x28 in float64 and float32: cgp_tapconv_* against
cgp_conv_* (the box stencil, the yardstick) on the same geometry, passes interleaved, for

  (a) 3x3 "same", (b) 7x7 "same", (c) the 28 -> 1x1 dense readout.

GB/s are over each pass's algorithmic bytes (one read of the input maps and one write of the
outputs); ``ratio`` is the tapconv's time over the box's on the same geometry and
``macs_per_ns`` the multiply-adds extent²·outputs over the time.

End to end (``--tile``, default 256): one off-diagonal tile of mnist_paper_convnet_gp with
Gaussian-tapered 7x7 tables against the same model with box kernels on the layer path
(set_fused_network(False)) and, for scale, on its default path.

After a warm-up of every pass, ``--reps`` rounds each time every pass once; a pass is
``--inner`` back-to-back launches between two events.  Every figure is the per-launch median
over the rounds with the fastest and slowest round beside it.

    python tools/tapconv_bench.py [--maps 65536] [--reps 9] [--inner 5] [--tile 256]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import cnn_gp  # noqa: E402
from cnn_gp import _native as N  # noqa: E402
from cnn_gp import program as P  # noqa: E402

from erf_bench import timed_interleaved  # noqa: E402

GEOMS = {"a_3x3_same": (3, "same"), "b_7x7_same": (7, "same"), "c_readout_28": (28, 0)}


def kernels(maps, side, reps, inner, dt):
    sfx = "f64" if dt == torch.float64 else "f32"
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((maps, side, side), dtype=dt, device="cuda", generator=g)
    out = torch.empty_like(x)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    conv, tap = getattr(lib, f"cgp_conv_{sfx}"), getattr(lib, f"cgp_tapconv_{sfx}")
    passes, meta, keep = {}, {}, []
    for name, (k, pad) in GEOMS.items():
        mod = cnn_gp.Conv2d(k, padding=pad, var_bias=0.1,
                            tap_weights=cnn_gp.gaussian_taps(k, k / 4))
        box = cnn_gp.Conv2d(k, padding=pad, var_bias=0.1)
        prog, _, _ = P.compile_program(cnn_gp.Sequential(box), side, side)
        op = prog.ops[0]
        ho, wo = op.shape_out
        ca = P.Plan._conv_args(op, x, out, maps, maps, 1)
        tg = P.tap_geometry(mod)
        table = torch.tensor(tg.table, dtype=torch.float64).to(dt).cuda()
        ta = N.TapConvArgs()
        ta.in_, ta.out, ta.table, ta.nmaps = N.ptr(x), N.ptr(out), N.ptr(table), maps
        ta.h, ta.w, ta.ho, ta.wo = side, side, ho, wo
        ta.extent, ta.offset, ta.stride, ta.dilation = tg.extent, tg.offset, 1, 1
        ta.bias = 0.1
        keep += [ca, ta, table]
        passes[name + "_tapconv"] = (lambda a=ta: N.check(tap(ctypes.byref(a), stream), "bench"))
        passes[name + "_box"] = (lambda a=ca: N.check(conv(ctypes.byref(a), stream), "bench"))
        gb = (x.numel() + maps * ho * wo) * x.element_size() / 1e9
        meta[name] = (gb, k * k * maps * ho * wo)
    torch.cuda.synchronize()
    times = timed_interleaved(passes, reps, inner)
    res = []
    for name, (gb, macs) in meta.items():
        tm, bm = times[name + "_tapconv"], times[name + "_box"]
        for what, (med, lo, hi) in (("tapconv", tm), ("box", bm)):
            res.append(dict({"pass": f"{name}_{what}", "dtype": sfx}, ms=round(med, 4),
                            min_ms=round(lo, 4), max_ms=round(hi, 4),
                            gbps=round(gb / (med / 1e3), 1)))
        res.append(dict({"pass": name, "dtype": sfx}, ratio=round(tm[0] / bm[0], 2),
                        macs_per_ns=round(macs / (tm[0] * 1e6), 1)))
    return res


def end_to_end(tile, reps, inner):
    cfg = importlib.import_module("configs.mnist_paper_convnet_gp")
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand((tile, 1, 28, 28), dtype=torch.float64, device="cuda", generator=g)
    z = torch.rand((tile, 1, 28, 28), dtype=torch.float64, device="cuda", generator=g)
    models = {}
    for name in ("tapered", "box_layer_path", "box_default_path"):
        importlib.reload(cfg)
        m = cfg.initial_model.double().cuda()
        if name == "tapered":
            taper = cnn_gp.gaussian_taps(7, 2.0).cuda().reshape(1, 1, 7, 7)
            with torch.no_grad():
                for c in m.mods:
                    if isinstance(c, cnn_gp.Conv2d) and c.kernel_size == 7:
                        c.kernel.mul_(taper * (49.0 / float(taper.sum())))
        m.set_fused_network(name == "box_default_path")
        models[name] = m

    def run(m):
        def f():
            with torch.no_grad():
                m(x, z, False, False)
        return f

    times = timed_interleaved({k: run(m) for k, m in models.items()}, reps, inner)
    kinds = [o.kind for o in models["tapered"]._plan(28, 28).prog.ops]
    res = [dict({"pass": f"tile_{k}", "dtype": "f64", "tile": tile}, ms=round(med, 3),
                min_ms=round(lo, 3), max_ms=round(hi, 3)) for k, (med, lo, hi) in times.items()]
    res.append(dict({"pass": "tile", "dtype": "f64"}, tapconv_ops=kinds.count("tapconv"),
                    ratio_to_box_layer_path=round(times["tapered"][0] /
                                                  times["box_layer_path"][0], 2)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--tile", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tapconv_bench needs a GPU: nothing is measured without one")
    for dt in (torch.float64, torch.float32):
        print(json.dumps(dict(op="28x28 maps", maps=args.maps)), flush=True)
        for r in kernels(args.maps, 28, args.reps, args.inner, dt):
            print(json.dumps(r), flush=True)
    if args.tile:
        for r in end_to_end(args.tile, args.reps, args.inner):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
