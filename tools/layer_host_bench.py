"""Wall time of layer-path calls on a tile small enough that the host sets the pace: the chain
network of tests/test_layer_lowering_pinned.py with its readout covering a 16x16 map, float64,
set_fused_network(False), 8 x 8 images of 3 channels.

    python tools/layer_host_bench.py [--tree DIR] [--tag NAME] [--calls 200]

Prints one JSON line: microseconds per call (wall clock over --calls calls, after 20 warm-up
calls and a synchronize, ended by a synchronize) of the fused forward, the unfused forward and
ntk.  ``--tree`` names the checkout whose package runs (default: this one), so two commits
can alternate on one library (CNNGP_LIB).
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--tag", default="tree", help="names the run in the output line")
args = ap.parse_args()
sys.path[:0] = [os.path.join(args.tree, "cnn-gp_amd"), args.tree]

import torch  # noqa: E402

import cnn_gp as m  # noqa: E402

S, C, R = m.Sequential, m.Conv2d, m.ReLU


def wall_us(fn, calls):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


model = S(C(3, var_bias=.1), R(), C(3), R(), C(16, padding=0)).double().cuda()
model.set_fused_network(False)
g = torch.Generator().manual_seed(0)
x, z = (torch.rand((8, 3, 16, 16), generator=g, dtype=torch.float64).cuda() for _ in range(2))
res = dict(run=args.tag, calls=args.calls)
with torch.no_grad():
    res["forward_us"] = wall_us(lambda: model(x, z), args.calls)
    res["ntk_us"] = wall_us(lambda: model.ntk(x, z, False), args.calls)
    model.set_fusion(False)
    res["unfused_forward_us"] = wall_us(lambda: model(x, z), args.calls)
print(json.dumps(res), flush=True)
