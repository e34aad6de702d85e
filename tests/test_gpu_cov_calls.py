"""GPU test of the one executor of position-pair maps (Plan.run_cov_steps): the library calls
of forward, position_covariance, ntk_maps and position_ntk on two small networks are the
calls the commit before it made -- when the forward list and the two-stream list each had an
executor of their own -- by name and in order, with the default workspace and with one that
splits the tile's 6 pairs into 3 chunks.  Chunked and unchunked results are the same bits, and
ntk_maps' K is forward's.

The networks are tests/test_cov_lowering_pinned.py's (every ``fn`` of both lists, a fused
addend, the ("pre", d) buffer, the self pass, "accum"); float64, N1 = 3, N2 = 2, 6x6 images of
3 channels."""
import functools

import numpy as np
import pytest
import torch

from cnn_gp import _native as N

from test_cov_lowering_pinned import nets

pytestmark = pytest.mark.gpu

DEV = "cuda"


def images():
    rng = np.random.default_rng(5)
    return tuple(torch.as_tensor(rng.random((n, 3, 6, 6))).to(DEV) for n in (3, 2))


# case -> (network, fusion of ntk_maps' convs or None, the call, the launch list whose peak
# sizes a chunk)
CASES = {
    "gap_forward_xz": ("residual_gap", None, lambda m, x, z: (m(x, z),), lambda p: p.pool),
    "gap_forward_xx": ("residual_gap", None, lambda m, x, z: (m(x),), lambda p: p.pool),
    "corr_forward_xz": ("corr_body", None, lambda m, x, z: (m(x, z),), lambda p: p.pool),
    "corr_forward_xx": ("corr_body", None, lambda m, x, z: (m(x),), lambda p: p.pool),
    "corr_position_covariance": ("corr_body", None,
                                 lambda m, x, z: (m.position_covariance(x),),
                                 lambda p: p.body_steps()),
    "gap_ntk_maps_fused": ("residual_gap", True,
                           lambda m, x, z: m.ntk_maps(x, z, False, return_nngp=True),
                           lambda p: p.pool_ntk(False, True, 8)),
    "gap_ntk_maps_unfused": ("residual_gap", False,
                             lambda m, x, z: m.ntk_maps(x, z, False, return_nngp=True),
                             lambda p: p.pool_ntk(False, False, 8)),
    "corr_position_ntk": ("corr_body", None, lambda m, x, z: (m.position_ntk(x, z, False),),
                          lambda p: p.pool_ntk(True, True, 8)),
}
MODES = ("whole", "chunked")


@functools.lru_cache(maxsize=None)
def run_case(case, mode):
    """(the names N.check sees -- every library call goes through it -- during the call, the
    tensors it returns); the call runs once before the recording, so that plans and uploads
    exist"""
    net, fused, call, steps = CASES[case]
    model = nets()[net][0].double().to(DEV)
    if fused is not None:
        model.set_ntk_maps_fusion(fused)
    x, z = images()
    if mode == "chunked":
        per_pair = steps(model._plan(6, 6)).peak * x.element_size()
        model.set_pool_workspace(2 * per_pair + per_pair // 2)
    seen = []
    real = N.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)

    with torch.no_grad():
        call(model, x, z)
        N.check = check
        try:
            out = call(model, x, z)
        finally:
            N.check = real
    torch.cuda.synchronize()
    return seen, tuple(t.cpu() for t in out)


# Recorded on the commit before Plan.run_cov_steps (the forward list ran in run_pairs_pool, the
# two-stream list in run_pairs_pool_ntk), one list per call and chunk:
_MO, _CV, _NL, _GE, _PO = ("cgp_cov_moments", "cgp_cov_conv", "cgp_cov_nonlin", "cgp_gelu_cov",
                           "cgp_cov_pool")
_AP, _DG, _CC, _AX = "cgp_covmap_avgpool", "cgp_covmap_diag", "cgp_corrconv", "cgp_axpby_f64"
_CVN, _NLN = "cgp_covntk_conv", "cgp_covntk_nonlin"
# the layer path's variances of the values upstream of the first AvgPool2d / CorrelatedConv2d
VAR_GAP = ["cgp_moments_var_f64", "cgp_conv", "cgp_var_relu_f64"]
VAR_CORR = ["cgp_moments_var_f64", "cgp_conv", "cgp_var_gelu_f64"]
# the self pass of one image set (a chunk of its pairs (i, i)), up to the step self_last
SELF_GAP = [_MO, _CV, _AP, _CV, _DG, _NL, _CV, _DG]
SELF_CORR = [_MO, _CV, _GE, _CC, _DG]
# one chunk of the tile's pairs
FWD_GAP = [_MO, _CV, _AP, _CV, _NL, _CV, _NL, _PO, _CV]
FWD_CORR = [_MO, _CV, _GE, _CC, _NL, _CC]
NTK_GAP_FUSED = [_MO, _CVN, _AP, _AP, _CVN, _NLN, _CVN, _NLN, _PO, _PO, _CVN]
NTK_GAP_UNFUSED = [_MO, _CV, _NLN, _AP, _AP, _CV, _CV, _NLN, _CV, _CV, _AX, _AX, _AX, _AX, _NLN,
                   _PO, _PO, _CV, _CV]
NTK_CORR = [_MO, _CV, _NLN, _CC, _CC, _AX, _NLN, _CC, _CC, _AX]
# whole: x's self pass, then y's unless same, then the tile.  chunked: the workspace holds two
# pairs of the list that sizes it, so the tile's 6 pairs are 3 chunks; the self passes run the
# forward list under the same workspace: x's 3 pairs are 2 chunks of the forward lists and one
# of the (larger) two-stream lists', y's 2 pairs one
PARENT_CALLS = {
    ("gap_forward_xz", "whole"): VAR_GAP + SELF_GAP * 2 + FWD_GAP,
    ("gap_forward_xz", "chunked"): VAR_GAP + SELF_GAP * 3 + FWD_GAP * 3,
    ("gap_forward_xx", "whole"): VAR_GAP + SELF_GAP + FWD_GAP,
    ("gap_forward_xx", "chunked"): VAR_GAP + SELF_GAP * 2 + FWD_GAP * 3,
    ("corr_forward_xz", "whole"): VAR_CORR + SELF_CORR * 2 + FWD_CORR,
    ("corr_forward_xz", "chunked"): VAR_CORR + SELF_CORR * 3 + FWD_CORR * 3,
    ("corr_forward_xx", "whole"): VAR_CORR + SELF_CORR + FWD_CORR,
    ("corr_forward_xx", "chunked"): VAR_CORR + SELF_CORR * 2 + FWD_CORR * 3,
    ("corr_position_covariance", "whole"): VAR_CORR + SELF_CORR + FWD_CORR,
    ("corr_position_covariance", "chunked"): VAR_CORR + SELF_CORR * 2 + FWD_CORR * 3,
    ("gap_ntk_maps_fused", "whole"): VAR_GAP + SELF_GAP * 2 + NTK_GAP_FUSED,
    ("gap_ntk_maps_fused", "chunked"): VAR_GAP + SELF_GAP * 2 + NTK_GAP_FUSED * 3,
    ("gap_ntk_maps_unfused", "whole"): VAR_GAP + SELF_GAP * 2 + NTK_GAP_UNFUSED,
    ("gap_ntk_maps_unfused", "chunked"): VAR_GAP + SELF_GAP * 2 + NTK_GAP_UNFUSED * 3,
    ("corr_position_ntk", "whole"): VAR_CORR + SELF_CORR * 2 + NTK_CORR,
    ("corr_position_ntk", "chunked"): VAR_CORR + SELF_CORR * 2 + NTK_CORR * 3,
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_calls_are_the_parents(case, mode):
    assert run_case(case, mode)[0] == PARENT_CALLS[case, mode]


@pytest.mark.parametrize("case", list(CASES))
def test_chunked_results_are_the_same_bits(case):
    (calls, whole), (chunked_calls, chunked) = (run_case(case, mode) for mode in MODES)
    assert len(chunked_calls) > len(calls)
    assert len(whole) == len(chunked)
    for a, b in zip(whole, chunked):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_ntk_maps_k_is_forwards(mode):
    (k,) = run_case("gap_forward_xz", mode)[1]
    for case in ("gap_ntk_maps_fused", "gap_ntk_maps_unfused"):
        kk, th = run_case(case, mode)[1]
        assert torch.equal(kk, k) and not torch.equal(th, k)
