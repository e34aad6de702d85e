"""Generate tests/golden/ntk_e2e.npz: the neural tangent kernel of every config and of the
two mixture networks, from the REFERENCE by autograd through its own ``propagate``.

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_golden_ntk.py

Same import shims as make_golden.py (imported from it, with its input generators and
mixture networks).  The reference has no NTK entry point; its NTK is taken as

    Θ = Σ over all Conv2d outputs l of ⟨∂K_final/∂K_xy^l, K_xy^l⟩   at fixed variances

by the scale trick: every ``Conv2d.propagate`` output's ``.xy`` is multiplied by a leaf
tensor of ones, one entry per pair, and ``K.sum()`` is differentiated in those leaves; the
sum of the gradients over the convs is Θ per pair (pairs do not interact).  Nothing of the
reference is copied: the file holds inputs and results only, all float64 (the images are
float32-representable).

Inputs: uniform for CIFAR-10 and the 10x10 mixture network, MNIST-like for 28x28 -- but
make_golden.py's MNIST-like images share a 4-pixel zero border, and wherever two images
have the same all-zero patch the first ReLU sees c = v1 = v2 (rho = 1 exactly), where the
reference's autograd returns NaN (sqrt and acos at the end of their domains).  So the
zero pixels, the border included, are lit with values from {1, ..., 16}/255 drawn per image
and pixel (``mnist_like_lit``): still dark background, sparse bright strokes and values
k/255, rho close to 1 in the background but not equal to it (16 levels, so that the four
pixels a corner's 3x3 patch sees are not proportional in two images either: a bias-free
first conv has rho = 1 there too).  main() asserts every stored Θ finite.

Per network ``n`` (5 images X, 3 images Z):
  n_X, n_Z
  n_Kxz, n_Txz          model(X, Z, False, False) and its Θ
  n_Kxx, n_Txx          model(X, X, False, False) and its Θ, diagonal entries NaN (the pairs
                        (i, i) have rho = 1, where autograd through acos is singular)
  n_Kxzdiag, n_Txzdiag  model(X[:3], Z, False, True) and its Θ
  n_Kdiag, n_Tdiag      model(X, X, True, True) and Θ(x_i, x_i).  In that mode the
                        reference's ReLU sets xy = xx/2 and the xy and xx streams are equal
                        functions of the images, so the leaves scale BOTH streams of every
                        conv output: the Jacobian of xx/2 is the Θ/2 rule at rho = 1.  (Scaling
                        xx alone would miss the last conv, whose result is read from xy.)
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

import torch  # noqa: E402

import cnn_gp  # noqa: E402
from cnn_gp.kernel_patch import ConvKP  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def mnist_like_lit(n, c, side, rng):
    """make_golden.mnist_like with every zero pixel replaced by one of 1/255 ... 16/255."""
    x = G.mnist_like(n, c, side, rng)
    dark = x == 0
    x[dark] = rng.integers(1, 17, size=int(dark.sum())).astype(np.float32) / 255
    return x


def ntk_by_scale(model, x, y, same, diag):
    """(K, Θ) of the reference model as numpy arrays, Θ by the scale trick."""
    scales = []
    orig = cnn_gp.Conv2d.propagate
    both = bool(same) and bool(diag)

    def propagate(self, kp):
        out = orig(self, kp)
        s = torch.ones(out.xy.shape[0], 1, 1, 1, dtype=out.xy.dtype, requires_grad=True)
        scales.append(s)
        return ConvKP(out.same, out.diag, out.xy * s, out.xx * s if both else out.xx, out.yy)

    cnn_gp.Conv2d.propagate = propagate
    try:
        k = model(x, y, same, diag)
        theta = torch.zeros_like(k)
        if scales:
            for g in torch.autograd.grad(k.sum(), scales):
                theta = theta + g.view(k.shape)
    finally:
        cnn_gp.Conv2d.propagate = orig
    return k.detach().numpy(), theta.detach().numpy()


def networks():
    """name -> (model, channels, side, input generator)"""
    nets = {}
    for name in G.CONFIGS:
        cfg = importlib.import_module(f"configs.{name}")
        side = 32 if name == "cifar10" else 28
        nets[name] = (cfg.initial_model, getattr(cfg, "in_channels", 1), side,
                      G.uniform if name == "cifar10" else mnist_like_lit)
    for name, (model, side) in G.mixture_nets(cnn_gp).items():
        nets["mixture_" + name] = (model, 1, side, mnist_like_lit if side == 28 else G.uniform)
    return nets


def main():
    recs = {}
    for n, (name, (model, chans, side, gen)) in enumerate(networks().items()):
        rng = np.random.default_rng(4000 + n)
        X = gen(5, chans, side, rng).astype(np.float64)
        Z = gen(3, chans, side, rng).astype(np.float64)
        model = model.to(torch.float64)
        Xt, Zt = torch.from_numpy(X), torch.from_numpy(Z)
        recs[f"{name}_X"], recs[f"{name}_Z"] = X, Z
        recs[f"{name}_Kxz"], recs[f"{name}_Txz"] = ntk_by_scale(model, Xt, Zt, False, False)
        kxx, txx = ntk_by_scale(model, Xt, Xt, False, False)
        eye = np.eye(len(X), dtype=bool)
        kxx[eye] = np.nan
        txx[eye] = np.nan
        recs[f"{name}_Kxx"], recs[f"{name}_Txx"] = kxx, txx
        recs[f"{name}_Kxzdiag"], recs[f"{name}_Txzdiag"] = ntk_by_scale(model, Xt[:3], Zt, False,
                                                                        True)
        recs[f"{name}_Kdiag"], recs[f"{name}_Tdiag"] = ntk_by_scale(model, Xt, Xt, True, True)
        for k in ("Txz", "Txzdiag", "Tdiag"):
            assert np.all(np.isfinite(recs[f"{name}_{k}"])), (name, k)
        assert np.all(np.isfinite(txx[~eye])), name
        model.to(torch.float32)
        print(name, "Txz[0] =", recs[f"{name}_Txz"][0])
    np.savez_compressed(os.path.join(OUT, "ntk_e2e.npz"), **recs)
    print("ntk_e2e:", len(recs), "arrays")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
