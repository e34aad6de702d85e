"""Bits of every nonlinearity entry point under two builds of libcnngp: the library of another
commit (tools/build_variant.sh with VARIANT_TREE) against the one in the tree.

    python tools/nonlin_ab.py --parent cnn-gp_amd/lib/ab/lib_parent.so [--new LIB] [--keep DIR]

Each library is loaded in a fresh child process (CNNGP_LIB), one after the other; a child runs
every case on the same seeded inputs and writes the outputs to a scratch directory.  This
process compares them as integer bit patterns, so NaNs count, and prints the case count and
how many differ; its exit status is 0 only when none does.

Cases (float32 and float64 each):
  layer path   cgp_relu_*, cgp_relu_ntk_*, cgp_erf_*, cgp_gelu_*, cgp_abrelu_* on pair maps of
               hw = 49 (49 maps: 41 in the first workgroup, 8 in the last), 2048 (one map per
               workgroup) and 1; same / diag in every legal combination, same && diag also
               with yy = NULL; forward and with Θ; CGP_FLAG_EXACT_RELU on and off; no addend
               and a K addend; separate outputs, in place, and Θ aliasing K
  variances    cgp_var_{relu,erf,gelu,abrelu}_* on the same variance maps
  position-pair maps   cgp_cov_nonlin_*, cgp_covntk_nonlin_*, cgp_gelu_cov_*, cgp_abrelu_cov_* on
               19 pairs of 5x3 maps (two full chunks and a partial one, chunks straddle pairs)
               and 3 pairs of 7x7 maps (a chunk boundary inside a pair); same on and off;
               no addend, a K addend and, with Θ, a Θ addend alone and both; separate outputs
               and in place
Inputs are Gram matrices of random features, so they are consistent covariances, with a
zero-variance pixel, rho = +1 and rho = -1 pixels, negative covariances and one NaN planted.
"""
import argparse
import ctypes
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cnn-gp_amd"), ROOT]

KINDS = ("relu", "erf", "gelu", "abrelu")
SLOPES = (0.01, 1.0)
NP_DT = {"f32": np.float32, "f64": np.float64}
# (hw, images per side): 49 maps of 49 pixels, 4 of 2048, 49 of 1
LAYER_SHAPES = ((49, 7), (2048, 2), (1, 7))
# (h, w, images, pairs)
COV_SHAPES = ((5, 3, 5, [(i, j) for i in range(5) for j in range(5)][:19]),
              (7, 7, 3, [(0, 0), (1, 2), (1, 1)]))


def smh(a=SLOPES[0], b=SLOPES[1]):
    return (a - b) * (a - b), a * b, (a * a + b * b) / 2


# ------------------------------------------------------------------------------------
# inputs (numpy, host): Gram matrices of 3-dimensional features per image and pixel
# ------------------------------------------------------------------------------------
def _features(rng, n, hw, same):
    """(fx, fy) [n][hw][3] with the planted pixels: image 0 pixel 0 has zero variance; pixel p1
    of x image 1 and y image 1 are parallel (rho = +1), pixel p2 of x image 1 and y image 2
    antiparallel (rho = -1); with same (fy is fx) the rho = +1 pixels are the self pairs'."""
    fx = rng.standard_normal((n, hw, 3))
    fx[0, 0] = 0.0
    p1, p2 = hw // 3, hw // 2
    if same:
        fx[2 % n, p2] = -0.5 * fx[1 % n, p2]
        return fx, fx, p1, p2
    fy = rng.standard_normal((n, hw, 3))
    fy[1 % n, p1] = 2.0 * fx[1 % n, p1]
    fy[2 % n, p2] = -0.5 * fx[1 % n, p2]
    return fx, fy, p1, p2


def layer_maps(n, hw, same, diag, dtn, seed=0):
    """Pair maps [nmaps][hw] of n x n images (n with diag): xy, theta, addend, xx, yy"""
    rng = np.random.default_rng(seed)
    fx, fy, _, _ = _features(rng, n, hw, same)
    xy = np.einsum("ipd,ipd->ip", fx, fy) if diag else \
        np.einsum("ipd,jpd->ijp", fx, fy).reshape(n * n, hw)
    xy[(3 * n + 1) % xy.shape[0], hw // 4] = np.nan
    m = dict(xy=xy, theta=rng.standard_normal(xy.shape), addend=rng.standard_normal(xy.shape),
             xx=(fx * fx).sum(-1), yy=(fy * fy).sum(-1))
    return {k: np.ascontiguousarray(v.astype(NP_DT[dtn])) for k, v in m.items()}


def cov_maps(h, w, nimg, pairs, same, dtn, seed=0):
    """Position-pair maps [pair][p_row][q_row][p_col][q_col] flattened: s, theta, addend,
    addend_theta [npairs][(h·w)²]; xx, yy [nimg][h·w]; pi, pj int32"""
    rng = np.random.default_rng(seed)
    hw = h * w
    fx, fy, _, _ = _features(rng, nimg, hw, same)
    s = np.stack([np.einsum("pd,qd->pq", fx[i], fy[j]).reshape(h, w, h, w)
                  .transpose(0, 2, 1, 3).reshape(-1) for i, j in pairs])
    s[len(pairs) // 2, (hw * hw) // 5] = np.nan
    m = dict(s=s, xx=(fx * fx).sum(-1), yy=(fy * fy).sum(-1),
             **{k: rng.standard_normal(s.shape) for k in ("theta", "addend", "addend_theta")})
    m = {k: np.ascontiguousarray(v.astype(NP_DT[dtn])) for k, v in m.items()}
    m["pi"] = np.array([p[0] for p in pairs], dtype=np.int32)
    m["pj"] = np.array([p[1] for p in pairs], dtype=np.int32)
    return m


# ------------------------------------------------------------------------------------
# one launch of an entry point (GPU); returns the outputs as numpy arrays
# ------------------------------------------------------------------------------------
def _gpu():
    import torch
    from cnn_gp import _native as N
    return torch, N


def _dev(a):
    torch, _ = _gpu()
    return torch.from_numpy(a).cuda()


def _launch(name, dtn, rec):
    torch, N = _gpu()
    N.check(getattr(N.load(), f"cgp_{name}_{dtn}")(ctypes.byref(rec),
                                                   torch.cuda.current_stream().cuda_stream),
            "cgp_" + name)
    torch.cuda.synchronize()


def run_layer(kind, dtn, m, n, same, diag, ntk=False, addend=False, exact=False, alias="none",
              yy_null=False):
    """kind's layer-path entry point on layer_maps() m.  alias: "none", "inplace" (the outputs
    are the inputs) or "theta_is_xy" (Θ is K's buffer).  Returns (K', Θ' or None)."""
    torch, N = _gpu()
    xy, xx = _dev(m["xy"]), _dev(m["xx"])
    yy = xx if same else _dev(m["yy"])
    th = (xy if alias == "theta_is_xy" else _dev(m["theta"])) if ntk else None
    out = xy if alias == "inplace" else torch.empty_like(xy)
    tout = (th if alias == "inplace" else torch.empty_like(xy)) if ntk else None
    add = _dev(m["addend"]) if addend else None
    name = "relu_ntk" if kind == "relu" and ntk else kind
    a = {"relu": N.ReluArgs, "relu_ntk": N.ReluNtkArgs, "erf": N.ErfArgs, "gelu": N.GeluArgs,
         "abrelu": N.ABReluArgs}[name]()
    a.xy = N.ptr(xy)
    setattr(a, "out" if name == "relu" else "out_xy", N.ptr(out))
    if ntk:
        a.theta, a.out_theta = N.ptr(th), N.ptr(tout)
    if addend:
        a.addend = N.ptr(add)
    a.xx, a.yy = N.ptr(xx), (None if yy_null else N.ptr(yy))
    a.nmaps, a.n1, a.n2 = xy.shape[0], n, n
    a.hw, a.same, a.diag = xy.shape[1], int(same), int(diag)
    a.flags = N.CGP_FLAG_EXACT_RELU if exact else 0
    if kind == "abrelu":
        a.s, a.m, a.h = smh()
    _launch(name, dtn, a)
    return out.cpu().numpy(), (tout.cpu().numpy() if ntk else None)


def run_var(kind, dtn, m, n, same):
    """cgp_var_<kind>_* on the variance maps of m.  Returns (xx', yy')."""
    torch, N = _gpu()
    xx = _dev(m["xx"])
    yy = xx if same else _dev(m["yy"])
    xo, yo = torch.empty_like(xx), torch.empty_like(yy)
    extra = (smh()[2],) if kind == "abrelu" else ()
    N.call(f"cgp_var_{kind}_{dtn}", N.ptr(xx), N.ptr(yy), n, n, xx.shape[1], int(same), *extra,
           N.ptr(xo), N.ptr(yo), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return xo.cpu().numpy(), yo.cpu().numpy()


def run_cov(kind, dtn, m, h, w, same, ntk=False, addend=False, addend_theta=False, exact=False,
            inplace=False):
    """kind's position-pair entry point on cov_maps() m: cgp_cov_nonlin_* / cgp_gelu_cov_* /
    cgp_abrelu_cov_* forward, cgp_covntk_nonlin_* / cgp_abrelu_cov_* with Θ.
    Returns (S', Θ' or None)."""
    torch, N = _gpu()
    s, xx = _dev(m["s"]), _dev(m["xx"])
    yy = xx if same else _dev(m["yy"])
    th = _dev(m["theta"]) if ntk else None
    out = s if inplace else torch.empty_like(s)
    tout = (th if inplace else torch.empty_like(s)) if ntk else None
    add = _dev(m["addend"]) if addend else None
    addt = _dev(m["addend_theta"]) if addend_theta else None
    pi, pj = _dev(m["pi"]), _dev(m["pj"])
    if kind == "abrelu":
        name, a = "abrelu_cov", N.ABReluCovArgs()
        a.s, a.m, a.hh = smh()
    elif ntk:
        name, a = "covntk_nonlin", N.CovNonlinNtkArgs()
    elif kind == "gelu":
        name, a = "gelu_cov", N.GeluCovArgs()
    else:
        name, a = "cov_nonlin", N.CovNonlinArgs()
    if hasattr(a, "kind"):
        a.kind = {"relu": N.CGP_COV_RELU, "erf": N.CGP_COV_ERF, "gelu": N.CGP_COV_GELU}[kind]
    a.in_, a.out, a.xx, a.yy = N.ptr(s), N.ptr(out), N.ptr(xx), N.ptr(yy)
    a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pj), s.shape[0]
    a.h, a.w, a.same = h, w, int(same)
    a.flags = N.CGP_FLAG_EXACT_RELU if exact else 0
    if ntk:
        a.theta, a.out_theta = N.ptr(th), N.ptr(tout)
    if addend:
        a.addend = N.ptr(add)
    if addend_theta:
        a.addend_theta = N.ptr(addt)
    _launch(name, dtn, a)
    return out.cpu().numpy(), (tout.cpu().numpy() if ntk else None)


# ------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------
def exact_modes(kind):
    return (False, True) if kind in ("relu", "abrelu") else (False,)


def cases():
    """(case name, function of no arguments that returns the outputs) in a fixed order"""
    for dtn in ("f32", "f64"):
        for (hw, n), (same, diag, yy_null) in itertools.product(
                LAYER_SHAPES, ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1))):
            m = layer_maps(n, hw, same, diag, dtn)
            tag = f"{dtn} hw={hw} same={same} diag={diag} yy_null={yy_null}"
            for kind in KINDS:
                for ntk, exact in itertools.product((False, True), exact_modes(kind)):
                    # cgp_relu_ntk_* has no addend
                    adds = (False,) if kind == "relu" and ntk else (False, True)
                    aliases = ("none", "inplace") + (("theta_is_xy",) if ntk else ())
                    for addend, alias in itertools.product(adds, aliases):
                        yield (f"layer {kind} {tag} ntk={int(ntk)} exact={int(exact)} "
                               f"addend={int(addend)} alias={alias}",
                               lambda kind=kind, m=m, n=n, same=same, diag=diag, ntk=ntk,
                               addend=addend, exact=exact, alias=alias, yy_null=yy_null, dtn=dtn:
                               run_layer(kind, dtn, m, n, same, diag, ntk, addend, exact, alias,
                                         bool(yy_null)))
                if not (diag or yy_null):
                    yield (f"var {kind} {tag}", lambda kind=kind, m=m, n=n, same=same, dtn=dtn:
                           run_var(kind, dtn, m, n, same))
        for (h, w, nimg, pairs), same in itertools.product(COV_SHAPES, (0, 1)):
            m = cov_maps(h, w, nimg, pairs, same, dtn)
            tag = f"{dtn} {h}x{w} pairs={len(pairs)} same={same}"
            for kind in KINDS:
                for ntk, exact, inplace in itertools.product((False, True), exact_modes(kind),
                                                             (False, True)):
                    adds = ((0, 0), (1, 0), (0, 1), (1, 1)) if ntk else ((0, 0), (1, 0))
                    for addend, addt in adds:
                        yield (f"cov {kind} {tag} ntk={int(ntk)} exact={int(exact)} "
                               f"addend={addend} addend_theta={addt} inplace={int(inplace)}",
                               lambda kind=kind, m=m, h=h, w=w, same=same, ntk=ntk, addend=addend,
                               addt=addt, exact=exact, inplace=inplace, dtn=dtn:
                               run_cov(kind, dtn, m, h, w, same, ntk, bool(addend), bool(addt),
                                       exact, inplace))


def child(out_dir):
    """Runs every case with the library CNNGP_LIB names; one .npy per output."""
    for idx, (name, fn) in enumerate(cases()):
        for k, arr in enumerate(fn()):
            if arr is not None:
                np.save(os.path.join(out_dir, f"{idx:05d}_{k}.npy"), arr)
    print(f"{idx + 1} cases", flush=True)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other commit's library")
    ap.add_argument("--new", default=os.path.join(ROOT, "cnn-gp_amd", "lib", "libcnngp.so"))
    ap.add_argument("--keep", help="keep the outputs under this directory")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.parent:
        ap.error("--parent is required")
    with tempfile.TemporaryDirectory() as tmp:
        top = args.keep or tmp
        dirs = {}
        for tag, lib in (("parent", args.parent), ("new", args.new)):
            dirs[tag] = os.path.join(top, tag)
            os.makedirs(dirs[tag], exist_ok=True)
            # a failed child ends the run: nothing more starts on the GPU after it
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dirs[tag]],
                           env=dict(os.environ, CNNGP_LIB=os.path.abspath(lib)), check=True,
                           timeout=args.timeout)
        names = [name for name, _ in cases()]
        differ = 0
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
            if bad:
                differ += 1
                print(f"DIFFER {name}: {'; '.join(bad)}")
        print(f"{len(names)} cases, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
