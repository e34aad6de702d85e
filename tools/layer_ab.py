"""Bits and peak memory of the layer path under two versions of the Python package: another
commit's (a git worktree of it) against the one in the tree, both on the same built library.

    git worktree add ../parent HEAD~1
    python tools/layer_ab.py --parent ../parent [--lib LIB] [--out FILE] [--keep DIR]

Each package runs in a fresh child process (its tree first on sys.path, CNNGP_LIB naming the one
library), one after the other, each under its own ``timeout``; a child that fails ends the run.
A child runs every case on the same seeded inputs and writes the outputs and each case's
torch.cuda.max_memory_allocated() to a scratch directory.  This process compares the outputs as
integer bit patterns, so NaNs count, and the peaks; it prints (and writes to --out) the case
count, how many outputs differ and how many peaks grew; its exit status is 0 only when none did.

Cases: the four networks of tests/test_layer_lowering_pinned.py (6x6 images of 3 channels) and
every network of tests/net_zoo.py, all with set_fused_network(False) so that forward takes the
layer path; float32 and float64; x against z, x against itself (same), diag on equal-length
inputs and same with diag; set_fusion on and off; set_exact_relu on and off; forward and
ntk(return_nngp=True).  N1 = 3, N2 = 2.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("xz", "same", "diag", "same_diag")
# the tests' networks; this tree's package unless a child has put another first
sys.path += [os.path.join(ROOT, "tests"), os.path.join(ROOT, "cnn-gp_amd"), ROOT]


def cases():
    """(case name, network, dtype, fusion, exact, mode, ntk) in a fixed order; needs no GPU"""
    import net_zoo
    import test_layer_lowering_pinned as pinned
    names = ["pinned:" + n for n in pinned.nets()] + ["zoo:" + n for n in net_zoo.NAMES]
    for net, dt, fusion, exact, mode, ntk in itertools.product(
            names, ("f32", "f64"), (1, 0), (0, 1), MODES, (0, 1)):
        yield (f"{net} {dt} fusion={fusion} exact={exact} {mode} {'ntk' if ntk else 'forward'}",
               net, dt, fusion, exact, mode, ntk)


def child(tree, out_dir):
    """Runs every case with the package of ``tree``; one .npy per output, peaks.json."""
    sys.path[:0] = [os.path.join(tree, "cnn-gp_amd"), tree]
    import torch
    import cnn_gp
    assert os.path.realpath(cnn_gp.__file__).startswith(os.path.realpath(tree) + os.sep)
    import net_zoo
    import test_layer_lowering_pinned as pinned
    zoo = net_zoo.zoo()
    peaks, models, inputs = [], {}, {}
    for idx, (_name, net, dt, fusion, exact, mode, ntk) in enumerate(cases()):
        dtype = torch.float32 if dt == "f32" else torch.float64
        kind, key = net.split(":")
        if (net, dt) not in inputs:
            c, side = (3, 6) if kind == "pinned" else (zoo[key].channels, zoo[key].side)
            rng = np.random.default_rng(7)
            inputs[net, dt] = tuple(torch.as_tensor(rng.random((n, c, side, side))).to(dtype)
                                    .cuda() for n in (3, 2))
        if (net, dt, fusion, exact) not in models:
            model = pinned.nets()[key] if kind == "pinned" else zoo[key].build()
            models.clear()
            models[net, dt, fusion, exact] = model.to(dtype).cuda().set_fused_network(False) \
                .set_fusion(bool(fusion)).set_exact_relu(bool(exact))
        model = models[net, dt, fusion, exact]
        x, z = inputs[net, dt]
        args = {"xz": (x, z, False, False), "same": (x,), "diag": (x[:2], z, False, True),
                "same_diag": (x, None, None, True)}[mode]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            outs = model.ntk(*args, return_nngp=True) if ntk else (model(*args),)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
        for k, t in enumerate(outs):
            np.save(os.path.join(out_dir, f"{idx:05d}_{k}.npy"), t.cpu().numpy())
        del outs
    with open(os.path.join(out_dir, "peaks.json"), "w") as f:
        json.dump(peaks, f)
    print(f"{len(peaks)} cases", flush=True)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the other commit")
    ap.add_argument("--lib", default=os.path.join(ROOT, "cnn-gp_amd", "lib", "libcnngp.so"))
    ap.add_argument("--out", help="write the summary lines to this file as well")
    ap.add_argument("--keep", help="keep the outputs under this directory")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--child", nargs=2, metavar=("TREE", "DIR"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.parent:
        ap.error("--parent is required")
    with tempfile.TemporaryDirectory() as tmp:
        top = args.keep or tmp
        dirs = {}
        for tag, tree in (("parent", os.path.abspath(args.parent)), ("new", ROOT)):
            dirs[tag] = os.path.join(top, tag)
            os.makedirs(dirs[tag], exist_ok=True)
            # a failed or timed-out child ends the run: nothing more starts on the GPU after it
            subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable,
                            os.path.abspath(__file__), "--child", tree, dirs[tag]],
                           env=dict(os.environ, CNNGP_LIB=os.path.abspath(args.lib)), check=True)
        peaks = {}
        for tag in dirs:
            with open(os.path.join(dirs[tag], "peaks.json")) as f:
                peaks[tag] = json.load(f)
        names = [c[0] for c in cases()]
        differ = grew = 0
        lines = []
        for idx, name in enumerate(names):
            bad = []
            for k in (0, 1):
                f = f"{idx:05d}_{k}.npy"
                have = [os.path.exists(os.path.join(dirs[t], f)) for t in ("parent", "new")]
                if have[0] != have[1]:
                    bad.append(f"output {k} missing")
                elif have[0]:
                    a, b = (bits(np.load(os.path.join(dirs[t], f))) for t in ("parent", "new"))
                    if a.shape != b.shape or not np.array_equal(a, b):
                        bad.append(f"output {k}: {int((a != b).sum())} of {a.size} elements")
            differ += bool(bad)
            if bad:
                lines.append(f"DIFFER {name}: {'; '.join(bad)}")
            if peaks["new"][idx] > peaks["parent"][idx]:
                grew += 1
                lines.append(f"PEAK {name}: {peaks['parent'][idx]} -> {peaks['new'][idx]} bytes")
        lower = sum(n < p for n, p in zip(peaks["new"], peaks["parent"]))
        lines.append(f"{len(names)} cases, {differ} differ in bits, {grew} with a larger "
                     f"max_memory_allocated ({lower} with a smaller one)")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if differ or grew else 0


if __name__ == "__main__":
    sys.exit(main())
