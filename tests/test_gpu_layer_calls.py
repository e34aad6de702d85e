"""GPU test of the one executor of the layer path (Plan.run_layer_steps): the library calls of
forward and ntk on four small networks are the calls the commit before it made -- when the
fused op list and the NTK list each had a hand-written executor -- by name and in order;
ntk's K is the unfused layer-path forward's, bit for bit, as it was there.

A call is named by the label N.check gets: the entry point's name, with the dtype suffix where
the call goes through N.call.

The networks are tests/test_layer_lowering_pinned.py's, with set_fused_network(False) so that
every forward takes the layer path; float64, N1 = 3, N2 = 2, 6x6 images of 3 channels."""
import functools

import numpy as np
import pytest
import torch

from cnn_gp import _native as N

from test_layer_lowering_pinned import nets

pytestmark = pytest.mark.gpu

DEV = "cuda"


def images():
    rng = np.random.default_rng(5)
    return tuple(torch.as_tensor(rng.random((n, 3, 6, 6))).to(DEV) for n in (3, 2))


# call -> (fusion, the call)
CALLS = {
    "forward_xz": (True, lambda m, x, z: (m(x, z),)),
    "forward_xx": (True, lambda m, x, z: (m(x),)),
    "forward_diag": (True, lambda m, x, z: (m(x[:2], z, False, True),)),
    "ntk_xz": (True, lambda m, x, z: m.ntk(x, z, False, return_nngp=True)),
    "ntk_xx": (True, lambda m, x, z: (m.ntk(x),)),
    "unfused_xz": (False, lambda m, x, z: (m(x, z),)),
}


@functools.lru_cache(maxsize=None)
def run_case(net, call):
    """(the names N.check sees -- every library call goes through it -- during the call, the
    tensors it returns); the call runs once before the recording, so that plans exist"""
    fusion, fn = CALLS[call]
    model = nets()[net].double().to(DEV).set_fused_network(False).set_fusion(fusion)
    x, z = images()
    seen = []
    real = N.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)

    with torch.no_grad():
        fn(model, x, z)
        N.check = check
        try:
            out = fn(model, x, z)
        finally:
            N.check = real
    torch.cuda.synchronize()
    return seen, tuple(t.cpu() for t in out)


_MV, _MX, _CV, _AX = "cgp_moments_var", "cgp_moments_xy", "cgp_conv", "cgp_axpby_f64"
_R, _E, _G, _A, _RN = "cgp_relu", "cgp_erf", "cgp_gelu", "cgp_abrelu", "cgp_relu_ntk"
_VR, _VE, _VG, _VA = ("cgp_var_relu_f64", "cgp_var_erf_f64", "cgp_var_gelu_f64",
                      "cgp_var_abrelu_f64")
# Recorded on the commit before Plan.run_layer_steps.  The variance pipeline runs every op of
# the unfused program on the per-image maps, of x against z and of x against itself alike (xx
# and yy are adjacent from the input on: one launch per op, and one per term of a sum)
VAR = {
    "chain": [_MV, _CV, _VR, _CV, _VR, _CV],
    "residual": [_MV, _CV, _VR, _CV, _VR, _CV, _AX, _AX, _VR, _CV],
    "mixed": [_MV, _CV, _VE, _CV, _VA, _AX, _AX, _AX, _VG, _CV, _VR, _AX, _AX, _VR, _CV],
    "lead": [_MV, _VR, _CV, _AX, _AX, _VR, _CV],
}
PARENT_CALLS = {}      # filled below: (net, call) -> names


def _pin(net, fused, unfused, ntk):
    for call in ("forward_xz", "forward_xx", "forward_diag"):
        PARENT_CALLS[net, call] = VAR[net] + fused
    PARENT_CALLS[net, "unfused_xz"] = VAR[net] + unfused
    PARENT_CALLS[net, "ntk_xz"] = PARENT_CALLS[net, "ntk_xx"] = VAR[net] + [_MX] + ntk


_pin("chain", [_CV] * 3, [_MX, _CV, _R, _CV, _R, _CV], [_CV, _RN, _CV, _CV, _RN, _CV, _CV])
_pin("residual", [_CV] * 4, [_MX, _CV, _R, _CV, _R, _CV, _AX, _AX, _R, _CV],
     [_CV, _RN, _CV, _CV, _RN, _CV, _CV, _AX, _AX, _AX, _AX, _RN, _CV, _CV])
_pin("mixed", [_MX, _CV, _E, _CV, _A, _AX, _AX, _AX, _G, _CV, _R, _CV],
     [_MX, _CV, _E, _CV, _A, _AX, _AX, _AX, _G, _CV, _R, _AX, _AX, _R, _CV],
     [_CV, _E, _CV, _A, _AX, _AX, _AX, _AX, _AX, _G, _CV, _CV, _RN, _AX, _AX, _AX, _AX, _RN,
      _CV, _CV])
_pin("lead", [_MX, _R, _CV, _CV], [_MX, _R, _CV, _AX, _AX, _R, _CV],
     [_R, _CV, _AX, _AX, _RN, _CV, _CV])

CASES = [(net, call) for net in nets() for call in CALLS]


@pytest.mark.parametrize("net,call", CASES)
def test_calls_are_the_parents(net, call):
    seen, out = run_case(net, call)
    assert seen == PARENT_CALLS[net, call]
    assert all(torch.isfinite(t).all() for t in out)


@pytest.mark.parametrize("net", list(nets()))
def test_ntk_k_is_the_unfused_forwards(net):
    """on the recorded commit the two agreed bit for bit on all four networks"""
    (k,) = run_case(net, "unfused_xz")[1]
    kk, th = run_case(net, "ntk_xz")[1]
    assert torch.equal(kk, k) and not torch.equal(th, k)
    assert run_case(net, "ntk_xx")[1][0].shape == (3, 3)
