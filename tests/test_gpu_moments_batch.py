"""The MOMENTS op of the compiled programs with batched image loads (csrc/netfuse.hip,
moments_batch): one-channel, three-channel and any-other-count inputs take three code paths
of one program, on the conv's column items where the program hoists its item decode and on
the elementwise layout elsewhere.  Every path stores what the interpreter's runtime channel
loop stores, bit for bit, and agrees with the CPU oracle.

Sizes: a Kxx of n = 21 (ragged 8x8 supertiles, diagonal entries, a two-pair workgroup whose
second half has no pair) and a Kxz of 9 x 13."""
import functools

import numpy as np
import pytest
import torch

from cnn_gp import _native as N
from oracle import nngp_oracle as O
from oracle import specs

import configs_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
# tests/test_gpu_parity.py: fp64 closed-form ReLU vs the oracle, fp32 vs the fp64 oracle
RTOL64 = 1e-8
RTOL32 = 2e-5
NXX, NX, NZ = 21, 9, 13

# (config, channels): the four reference architectures on their own inputs, and the two
# hoisted programs (ConvNet, Residual) on 1, 2 and 3 channels; the elementwise layout of
# mnist_as_tf's head on 1 and 3; cifar10's 32x32 head on 3
CASES = [("mnist_paper_convnet_gp", 1), ("mnist_paper_convnet_gp", 2),
         ("mnist_paper_convnet_gp", 3), ("mnist_paper_residual_cnn_gp", 1),
         ("mnist_paper_residual_cnn_gp", 2), ("mnist_paper_residual_cnn_gp", 3),
         ("mnist_as_tf", 1), ("mnist_as_tf", 3), ("cifar10", 3)]


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


@functools.lru_cache(maxsize=None)
def inputs(cfg, ch):
    """images exact in float32, so both precisions and the oracle see the same values;
    signed, so the channel sum cancels"""
    side = specs.GEOMETRY[cfg][1]
    rng = np.random.default_rng(1000 + 10 * len(cfg) + ch)
    def draw(n):
        return (rng.random((n, ch, side, side)) - 0.3).astype(np.float32).astype(np.float64)
    return draw(NXX), draw(NX), draw(NZ)


@functools.lru_cache(maxsize=None)
def oracle(cfg, ch):
    A, X, Z = inputs(cfg, ch)
    spec = specs.CONFIGS[cfg]()
    return O.kernel(spec, A), O.kernel(spec, X, Z, False, False)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("cfg,ch", CASES)
def test_batched_moments_equal_interpreter_and_oracle(cfg, ch, dtn, monkeypatch):
    from cnn_gp import netplan
    tdt = torch.float64 if dtn == "f64" else torch.float32
    A, X, Z = (torch.as_tensor(a).to(DEV, tdt) for a in inputs(cfg, ch))
    m = configs_util.model(cfg).to(DEV, tdt)
    picked = []
    real = N.load().cgp_net_program

    def spy(*a):
        picked.append(real(*a))
        return picked[-1]
    with torch.no_grad():
        monkeypatch.setattr(N.load(), "cgp_net_program", spy, raising=False)
        kxx = m(A).cpu().numpy()
        kxz = m(X, Z, False, False).cpu().numpy()
        assert picked and all(p > 0 for p in picked), picked   # the compiled programs ran
        monkeypatch.setattr(netplan, "USE_PROGRAMS", False)
        ixx = m(A).cpu().numpy()
        ixz = m(X, Z, False, False).cpu().numpy()
    assert kxx.shape == (NXX, NXX) and kxz.shape == (NX, NZ)
    assert np.array_equal(kxx, ixx), rel_err(kxx, ixx)
    assert np.array_equal(kxz, ixz), rel_err(kxz, ixz)
    assert np.array_equal(kxx, kxx.T)
    rxx, rxz = oracle(cfg, ch)
    tol = RTOL64 if dtn == "f64" else RTOL32
    exx, exz = rel_err(kxx, rxx), rel_err(kxz, rxz)
    print(f"{cfg} C={ch} {dtn}: Kxx rel err {exx:.2e}, Kxz rel err {exz:.2e}")
    assert exx < tol and exz < tol, (exx, exz)
