"""The lean op chain of the compiled fp64 programs (csrc/netfuse.hip prog_lean, relu_q_n NOCAP
/ HALF; DESIGN §4.1 "Round 8") against the op-record interpreter, which only has the default
ReLU form: bit for bit, on the image sets of tests/test_gpu_relu_one_root.py.

Kxz is 9 x 7 and Kxx is of 11 images: odd sizes, so a two-pair head workgroup has a half
without a pair, the 8x8 supertiles are ragged and a workgroup walks several groups.
cgp_net_program_lean says which chain a case runs: the ConvNet (7 cap-free, 6 add-free sites)
and the Residual net (9 cap-free) on their own weights.  The ConvNet with var_bias = 0 runs
the default chain of the same kernel (the fallback); mnist_as_tf, whose programs hold the
default chain only, as configured (var_bias = 0) and with a bias on every conv."""
import functools

import numpy as np
import pytest
import torch

import cnn_gp
import configs_util
from cnn_gp import _native as N
from oracle import nngp_oracle as O

from test_gpu_parity import DEV, RTOL64, rel_err
from test_gpu_relu_one_root import dev, images
from test_relu_lean_host import model_lean

pytestmark = pytest.mark.gpu

SETS = ["uniform", "mnist", "huge", "twins", "negative"]
# net -> (config, var_bias for every conv or None for the config's own, cgp_net_program_lean
# per stage)
NETS = {
    "convnet": ("mnist_paper_convnet_gp", None, [(1, 7, 6)]),
    "residual": ("mnist_paper_residual_cnn_gp", None, [(1, 9, 0)]),
    "as_tf_biased": ("mnist_as_tf", 0.5, [(1, 0, 0)] * 3),
    "as_tf": ("mnist_as_tf", None, [(0, -1, -1)] * 3),
    "convnet_bias0": ("mnist_paper_convnet_gp", 0.0, [(0, -1, -1)]),
}


def build(net):
    cfg, bias, _ = NETS[net]
    m = configs_util.model(cfg)
    if bias is not None:
        for mod in m.modules():
            if isinstance(mod, cnn_gp.Conv2d):
                mod.var_bias = bias
    return m.to(DEV, torch.float64)


@functools.lru_cache(maxsize=None)
def inputs(kind):
    """(X [9], Z [7], the 11 images of Kxx) on the device"""
    X, Z = images(kind)
    return dev(X), dev(Z), dev(np.concatenate([X, Z[:2]]))


def forward(m):
    def run(kind):
        x, z, xx = inputs(kind)
        with torch.no_grad():
            return {"Kxz": m(x, z, False, False).cpu().numpy(), "Kxx": m(xx).cpu().numpy(),
                    "diag": m(xx, xx, True, True).cpu().numpy()}
    return run


def programs_of(m):
    net = m._net_plan(m._plan(28, 28), 8)
    return [t[3] for t in net.__dict__["_templates"].values()]


def both_paths(net, kind, monkeypatch):
    """the net's kernels through the compiled programs and through the interpreter"""
    from cnn_gp import netplan
    m = build(net)
    assert model_lean(m, 28) == NETS[net][2], net
    prog = forward(m)(kind)
    assert all(p > 0 for p in programs_of(m)), programs_of(m)
    with monkeypatch.context() as mp:
        mp.setattr(N.load(), "cgp_net_program", lambda *a: 0, raising=False)
        mp.setattr(netplan, "USE_PROGRAMS", False)
        mi = build(net)
        interp = forward(mi)(kind)
        assert all(p == 0 for p in programs_of(mi)), programs_of(mi)
    return prog, interp


def check_equal(prog, interp, what):
    for k in prog:
        assert np.array_equal(prog[k], interp[k], equal_nan=True), \
            (what, k, rel_err(prog[k], interp[k]))
    # Kxx stays exactly symmetric and its diagonal is kdiag
    assert np.array_equal(prog["Kxx"], prog["Kxx"].T, equal_nan=True), what
    assert np.array_equal(np.diag(prog["Kxx"]), prog["diag"], equal_nan=True), what


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("net", ["convnet", "residual", "as_tf_biased", "as_tf"])
def test_lean_program_equals_interpreter(net, kind, monkeypatch):
    prog, interp = both_paths(net, kind, monkeypatch)
    assert np.isfinite(prog["Kxz"]).all() and np.isfinite(prog["Kxx"]).all()
    check_equal(prog, interp, (net, kind))


def test_fallback_with_live_cap(monkeypatch):
    """var_bias = 0 on zero-border images with an all-zero image: zero-variance pixels, so
    the cap is live and the condition fails on these records; the same program kernel then
    runs its default chain: equal to the interpreter bit for bit and to the oracle within
    the suite's fp64 bound (measured: 7.4e-10 on Kxz, 6.2e-10 on Kxx)"""
    prog, interp = both_paths("convnet_bias0", "mnist", monkeypatch)
    check_equal(prog, interp, "convnet_bias0")
    X, Z = images("mnist")
    XX = np.concatenate([X, Z[:2]])
    # zero-variance pixels on both sides: a corner's whole 7x7 window lies in the border
    assert not X[:, :, :4, :4].any() and not Z[:, :, :4, :4].any() and not X[3].any()
    spec = configs_util.spec_of(build("convnet_bias0"))
    ref = {"Kxz": O.kernel(spec, X, Z, False, False), "Kxx": O.kernel(spec, XX)}
    errs = {k: rel_err(prog[k], ref[k]) for k in ref}
    print(f"lean fallback: rel err vs oracle {errs}")
    for k, e in errs.items():
        assert e < RTOL64["fast"], (k, e)
