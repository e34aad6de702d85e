"""Generate tests/golden/tapconv.npz by running the REFERENCE with its Conv2d.kernel buffers
overwritten: the reference's Conv2d.propagate is F.conv2d with that buffer (kernels.py:92-98),
so whatever is written into it the reference evaluates.

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_golden_tapconv.py

The import shims are make_golden.py's (a stub torchvision, np.int).  Nothing of the reference
is copied: the file holds inputs, tables and the reference's outputs only, all inputs
float32-representable.  The networks and op geometries are tests/tapconv_nets.py's.

  op<n>_par / _tab / _in / _out   Conv2d.propagate on random maps, the buffer overwritten by
                                  a random table (some with zero and negative entries, some
                                  even "same" buffers with their first row and column written)
  X_<side> / Z_<side>             the images of the end-to-end cases, 2 channels
  <net>_<side>_tab<i>             the tables of an end-to-end case, one per tapped conv
  <net>_<side>_<f64|f32>_Kxx / _Kxz / _Kxdiag / _Kxzdiag
                                  model(X), model(X, Z), model(X, X, True, True),
                                  model(X[:3], Z, False, True)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

np.int = int  # data.py:12 (numpy >= 1.24 removed the alias)
_tv = types.ModuleType("torchvision")
_tv.datasets = types.SimpleNamespace(MNIST=None, CIFAR10=None)
_tv.transforms = types.SimpleNamespace(ToTensor=None, Compose=None)
sys.modules["torchvision"] = _tv
sys.path.insert(0, "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import torch  # noqa: E402

import cnn_gp  # noqa: E402
from cnn_gp.kernel_patch import ConvKP  # noqa: E402

import tapconv_nets as TN  # noqa: E402


def gen_ops(recs):
    rng = np.random.default_rng(77)
    n = 0
    for k, s, pad, d, side, mode in TN.op_cases():
        vb = float(rng.choice([0.0, 0.25, 4.5]))
        mod = cnn_gp.Conv2d(k, stride=s, padding=pad, dilation=d, var_bias=vb).double()
        ke = mod.kernel.shape[-1]
        tab = np.zeros((ke, ke), np.float32)
        new = rng.random((ke, ke), dtype=np.float32)
        if mode != "pos":
            new -= np.float32(0.3)
            new[rng.random((ke, ke)) < 0.2] = 0
        if mode == "full":
            tab[:] = new
        else:
            tab[ke - k:, ke - k:] = new[ke - k:, ke - k:]
        maps = rng.random((3, side, side), dtype=np.float32)
        with torch.no_grad():
            mod.kernel.copy_(torch.from_numpy(tab).double().reshape(1, 1, ke, ke))
            t = torch.from_numpy(maps.astype(np.float64))[:, None]
            try:
                out = mod.propagate(ConvKP(False, True, t, t, t)).xy[:, 0].numpy()
            except RuntimeError:
                continue  # geometry invalid for this size (F.conv2d refuses it)
        recs[f"op{n}_par"] = np.array([k, s, -1 if pad == "same" else pad, d, vb])
        recs[f"op{n}_tab"], recs[f"op{n}_in"], recs[f"op{n}_out"] = tab, maps, out
        n += 1
    print("op cases:", n)


def gen_e2e(recs):
    rng = np.random.default_rng(78)
    for side in TN.SIDES:
        X = rng.random((4, TN.CHANNELS, side, side), dtype=np.float32)
        Z = rng.random((3, TN.CHANNELS, side, side), dtype=np.float32)
        recs[f"X_{side}"], recs[f"Z_{side}"] = X, Z
        for name in TN.NETS:
            key = f"{name}_{side}"
            model, which = TN.build(cnn_gp, name, side)
            tables = [TN.random_table(TN.convs(cnn_gp, model)[i], rng) for i in which]
            for i, tab in enumerate(tables):
                recs[f"{key}_tab{i}"] = tab
            for dtn, tdt in (("f64", torch.float64), ("f32", torch.float32)):
                model = TN.set_tables(cnn_gp, model.to(tdt), which, tables)
                Xt, Zt = torch.from_numpy(X).to(tdt), torch.from_numpy(Z).to(tdt)
                with torch.no_grad():
                    recs[f"{key}_{dtn}_Kxx"] = model(Xt).numpy()
                    recs[f"{key}_{dtn}_Kxz"] = model(Xt, Zt, False, False).numpy()
                    recs[f"{key}_{dtn}_Kxdiag"] = model(Xt, Xt, True, True).numpy()
                    recs[f"{key}_{dtn}_Kxzdiag"] = model(Xt[:3], Zt, False, True).numpy()
            assert all((recs[f"{key}_f64_{m}"] > 0).all()
                       for m in ("Kxx", "Kxz", "Kxdiag", "Kxzdiag")), key
    print("e2e cases:", len(TN.NETS) * len(TN.SIDES))


def main():
    recs = {}
    gen_ops(recs)
    gen_e2e(recs)
    path = os.path.join(OUT, "tapconv.npz")
    np.savez_compressed(path, **recs)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
