"""The one-root fp64 closed-form ReLU of the whole-network kernel (csrc/cgp_common.h
relu_q_n, CGP_RELU_ONE_ROOT) and the 1/sqrt(v/8) maps it reads (cgp_rsqrt_batch_f64):
small ragged tiles of every code form against the CPU oracle on image sets that reach the
form's edges, and the maps themselves.

9 x 7 tiles of 28x28 images: odd sizes, so a two-pair head workgroup has a lone half and the
8x8 supertiles are ragged.  mnist_paper_convnet_gp runs the one-pair halves (a wave's vote,
AD 1) and the sum-fused last conv; mnist_as_tf the 4- and 16-pair stages (votes per group,
AD 2) and the dual-output convs; the zoo's in14 the same form through the op-record
interpreter."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import configs_util
import net_zoo
from cnn_gp import _native as N
from oracle import nngp_oracle as O

from test_gpu_parity import DEV, RTOL64, rel_err, stream

pytestmark = pytest.mark.gpu

N1, N2 = 9, 7
SETS = ["uniform", "mnist", "tiny", "huge", "twins", "negative"]


def _uniform(seed, n, c, side):
    rng = np.random.default_rng(seed)
    return rng.random((n, c, side, side), dtype=np.float32).astype(np.float64)


def _mnist_like(seed, n, c, side):
    """zero borders, ~60% zero pixels and one all-zero image: zero-variance pixels on one
    side of a pair and, where two borders or the zero image meet, on both"""
    rng = np.random.default_rng(seed)
    a = np.floor(rng.random((n, c, side, side)) * 256) / 255.0
    a[rng.random(a.shape) < 0.6] = 0.0
    b = side // 7
    a[:, :, :b, :] = 0.0
    a[:, :, -b:, :] = 0.0
    a[:, :, :, :b] = 0.0
    a[:, :, :, -b:] = 0.0
    a[3] = 0.0
    return a


@functools.lru_cache(maxsize=None)
def images(kind, c=1, side=28):
    """(X [9], Z [7]), read-only: shared by the tests of every network"""
    X, Z = _uniform(50, N1, c, side), _uniform(51, N2, c, side)
    if kind == "mnist":
        X = _mnist_like(52, N1, c, side)
        Z = X[::-1][:N2].copy()                 # holds the all-zero image too
    elif kind == "tiny":
        X, Z = X * 1e-6, Z * 1e-6
    elif kind == "huge":
        X, Z = X * 1e6, Z * 1e6
    elif kind == "twins":                        # |rho| = 1 off the diagonal, Kxx and Kxz
        X[1] = X[0]
        Z[0] = X[0]
        Z[4] = X[5]
    elif kind == "negative":                     # rho = -1 at the first layer
        X[1] = -X[0]
        Z[0] = -X[2]
        Z[3] = -Z[2]
    for a in (X, Z):
        a.setflags(write=False)
    return X, Z


def build(name):
    if name in net_zoo.NAMES:
        z = net_zoo.zoo()[name]
        return z.build(), z.channels, z.side
    return configs_util.model(name), 1, 28


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    m, c, side = build(name)
    X, Z = images(kind, c, side)
    spec = configs_util.spec_of(m)
    ref = {"Kxz": O.kernel(spec, X, Z, False, False), "Kxx": O.kernel(spec, X)}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def dev(a):
    return torch.tensor(a).to(DEV, torch.float64)


CASES = [(n, k) for n in ("mnist_paper_convnet_gp", "mnist_as_tf") for k in SETS] + \
    [("in14", "uniform"), ("in14", "mnist")]


@pytest.mark.parametrize("name,kind", CASES)
def test_ragged_tiles_match_oracle(name, kind):
    m, c, side = build(name)
    m = m.to(DEV, torch.float64)
    assert m._net_plan(m._plan(side, side), 8) is not None
    X, Z = images(kind, c, side)
    ref = reference(name, kind)
    with torch.no_grad():
        x, z = dev(X), dev(Z)
        got = {"Kxz": m(x, z, False, False).cpu().numpy(), "Kxx": m(x).cpu().numpy()}
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print(f"one-root {name} {kind}: rel err vs oracle {errs}")
    assert np.array_equal(got["Kxx"], got["Kxx"].T)
    for k, e in errs.items():
        assert e < RTOL64["fast"], (name, kind, k, e)


def _rsqrt_batch(src):
    dst = [torch.full_like(s, float("nan")) for s in src]
    k = len(src)
    ps = (ctypes.c_void_p * k)(*[s.data_ptr() for s in src])
    pd = (ctypes.c_void_p * k)(*[d.data_ptr() for d in dst])
    pn = (ctypes.c_int64 * k)(*[s.numel() for s in src])
    N.call("cgp_rsqrt_batch_f64", k, ps, pd, pn, stream())
    return dst


def test_rsqrt_batch_every_buffer():
    """cgp_rsqrt_batch_f64: 1/sqrt(v/8) within 2 ulp of the CPU's float64 rsqrt (each of the
    two is within about 1 ulp of the true value) and +inf exactly at v = 0, over variances
    from 1e-12 to 1e12, for buffers of 784, 1, 0 and 49 elements and more buffers than one
    launch holds (32)"""
    g = torch.Generator().manual_seed(6)
    sizes = [784, 1, 0, 49] * 9                      # 36 buffers: two launches
    src = []
    for n in sizes:
        v = torch.rand(n, generator=g, dtype=torch.float64) * 300
        v *= 10.0 ** torch.randint(-12, 11, (n,), generator=g).double()
        v[torch.rand(n, generator=g) < 0.1] = 0.0
        src.append(v)
    dst = _rsqrt_batch([s.to(DEV) for s in src])
    for s, d in zip(src, dst):
        d = d.cpu()
        want = torch.rsqrt(s / 8)
        zero = s == 0
        assert torch.equal(torch.isinf(d), zero) and bool((d[zero] > 0).all())
        assert bool(((d[~zero] - want[~zero]).abs() <= 4.5e-16 * want[~zero]).all())


def test_bound_maps_equal_the_batch_kernel():
    """the maps a bound build holds (NNGPKernel.image_variances) are the batch kernel's,
    bit for bit, from the build's plain variance maps; in the scaled form there are none"""
    m = configs_util.model("mnist_as_tf").to(DEV, torch.float64)
    X, _ = images("mnist")
    vx = m.image_variances(dev(X))
    assert vx is not None
    net = m._net_plan(m._plan(28, 28), 8)
    if net.var_form() != N.CGP_VAR_FORM_RSQRT:
        assert not vx.mvar and vx.qvar
        return
    used = net.quarter_vars(torch.float64, 0)
    assert used and set(vx.mvar) == used and not vx.qvar
    again = _rsqrt_batch([vx.var[v] for v in sorted(used)])
    for v, a in zip(sorted(used), again):
        assert torch.equal(vx.mvar[v], a)
        assert torch.equal(torch.isinf(a), vx.var[v] == 0)
