"""Timing of convs with correlated weights on position-pair maps (csrc/corrconv.hip, DESIGN
§3.5), HIP events, all in one process, by the method of tools/avgpool_bench.py, on ``--pairs``
position-pair maps of 28x28 images:

  (a) cgp_corrconv_* 3x3 "same" with an RBF R (9 input blocks per output row pair), with
      cgp_cov_conv_* 3x3 and cgp_covmap_avgpool_* k = s = 2 on the same maps as yardsticks;
  (b) the same with R = I (3 input blocks per output row pair, cgp_cov_conv_*'s traffic);
  (c) the k = 28 readout, one value per pair, with R = ones and with band_corr(28, 2), with
      cgp_cov_pool_* (one read of the map) as the yardstick.

GB/s are over each pass's algorithmic bytes: one read of the map plus one write of the
output (a whole map for the 3x3 passes, nothing to speak of for the readouts; the band
readout reads the 134 of 784 row-pair blocks its R_rows leaves).  Beside them, the bytes a
pass requests of the memory system over its algorithmic bytes ("requests"): every input
block is asked for once per output row pair and row-offset pair that reads it.

After a warm-up of every pass, ``--reps`` rounds each time every pass once; a pass is
``--inner`` back-to-back launches between two events.  Every figure is the per-launch median
over the rounds with the fastest and slowest round beside it.

    python tools/corrconv_bench.py [--pairs 64] [--reps 9] [--inner 5]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cnn_gp  # noqa: E402
from cnn_gp import _native as N  # noqa: E402

from erf_bench import timed_interleaved  # noqa: E402


def kernels(pairs, side, reps, inner, dt):
    sfx = "f64" if dt == torch.float64 else "f32"
    hw = side * side
    n = hw * hw
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand((pairs, n), dtype=dt, device="cuda", generator=g) * 0.9
    out = torch.empty_like(s)
    small = torch.empty((pairs, n // 16), dtype=dt, device="cuda")
    one = torch.empty(pairs, dtype=dt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.load()
    gb = s.numel() * s.element_size() / 1e9
    table = lambda r: torch.tensor(np.asarray(r), dtype=dt, device="cuda")       # noqa: E731
    tabs = {"rbf": table(cnn_gp.rbf_corr(3, 1.0)), "eye": table(np.eye(3)),
            "ones": table(np.ones((side, side))), "band": table(cnn_gp.band_corr(side, 2))}
    torch.cuda.synchronize()

    def corr(tab, readout):
        a = N.CorrConvArgs()
        a.in_, a.out, a.npairs = N.ptr(s), N.ptr(one if readout else out), pairs
        a.corr_rows = a.corr_cols = N.ptr(tabs[tab])
        a.h = a.w = side
        a.ho = a.wo = 1 if readout else side
        a.taps, a.offset = (side, 0) if readout else (3, -1)
        a.stride = a.dilation = 1
        a.weight, a.bias = 1 / a.taps ** 2, 0.1
        return a

    c = N.CovConvArgs()
    c.in_, c.out, c.npairs = N.ptr(s), N.ptr(out), pairs
    c.h = c.w = c.ho = c.wo = side
    c.taps, c.offset, c.stride, c.dilation = 3, -1, 1, 1
    c.post, c.weight, c.bias = N.CGP_COV_NONE, 1 / 9, 0.1
    p = N.CovAvgPoolArgs()
    p.in_, p.out, p.npairs = N.ptr(s), N.ptr(small), pairs
    p.h = p.w = side
    p.ho = p.wo = side // 2
    p.k = p.stride = 2
    fn = getattr(lib, f"cgp_corrconv_{sfx}")
    conv, avg = getattr(lib, f"cgp_cov_conv_{sfx}"), getattr(lib, f"cgp_covmap_avgpool_{sfx}")
    args = {"a_corrconv_3x3_rbf": corr("rbf", False), "b_corrconv_3x3_identity": corr("eye", False),
            "c_corrconv_readout_ones": corr("ones", True),
            "c_corrconv_readout_band2": corr("band", True)}
    launch = lambda a: (lambda: N.check(fn(ctypes.byref(a), stream), "bench"))    # noqa: E731
    # blocks of the 784 a band of half-width 2 leaves non-zero in R_rows
    band_blocks = int(np.count_nonzero(cnn_gp.band_corr(side, 2))) / side ** 2
    # name -> (launch, map passes over HBM, requested passes)
    passes = {
        "a_corrconv_3x3_rbf": (launch(args["a_corrconv_3x3_rbf"]), 2, 9 + 1),
        "b_corrconv_3x3_identity": (launch(args["b_corrconv_3x3_identity"]), 2, 3 + 1),
        "yardstick_cov_conv_3x3": (lambda: N.check(conv(ctypes.byref(c), stream), "bench"), 2,
                                   3 + 1),
        "yardstick_covmap_avgpool_k2": (lambda: N.check(avg(ctypes.byref(p), stream), "bench"),
                                        1 + 1 / 16, 1 + 1 / 16),
        "c_corrconv_readout_ones": (launch(args["c_corrconv_readout_ones"]), 1, 1),
        "c_corrconv_readout_band2": (launch(args["c_corrconv_readout_band2"]), band_blocks,
                                     band_blocks),
        "yardstick_cov_pool": (lambda: N.call(f"cgp_cov_pool_{sfx}", N.ptr(s), pairs, n,
                                              N.ptr(one), stream), 1, 1),
    }
    times = timed_interleaved({k: f for k, (f, _, _) in passes.items()}, reps, inner)
    return {k: dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                    gbps=round(passes[k][1] * gb / (med / 1e3), 1),
                    requests=round(passes[k][2] / passes[k][1], 2))
            for k, (med, lo, hi) in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        res = kernels(args.pairs, 28, args.reps, args.inner, dt)
        print(json.dumps(dict(op="28x28 position-pair maps", dtype=name, pairs=args.pairs)),
              flush=True)
        for k, v in res.items():
            print(json.dumps({"pass": k, "dtype": name, **v}), flush=True)


if __name__ == "__main__":
    main()
