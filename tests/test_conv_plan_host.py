"""CPU-only tests of cgp_conv_plan_* and cgp_conv_args.max_groups: which conv kernel
cgp_conv_* dispatches, its chunking and its grid, asked of the library without a launch
(the GPU side is tests/test_gpu_layer_walk.py)."""
import ctypes

import pytest
import torch

from cnn_gp import _native as N

import conv_walk_util as U

DTYPES = ["f64", "f32"]


def geo_of(case):
    side, k, stride = case
    return U.geometry(side, side, U.conv_spec(k, stride))


def check_counts(p, nmaps, max_groups):
    kernel, mpc, chunks, groups = p
    assert mpc >= 1 and mpc * (chunks - 1) < nmaps <= mpc * chunks, (p, nmaps)
    if max_groups:
        assert groups == min(chunks, max_groups), (p, max_groups)
    else:
        assert 1 <= groups <= chunks, p
        if not torch.cuda.is_available():
            # no device: one workgroup on each of 256 CUs
            assert groups == min(chunks, 256), p


@pytest.mark.parametrize("dtn", DTYPES)
@pytest.mark.parametrize("case", U.GEOS, ids=lambda c: "-".join(map(str, c)))
def test_plan_reports_the_compiled_kernel_for_every_table_geometry(case, dtn):
    geo = geo_of(case)
    assert len(U.GEO_MODES) == 7
    mpcs = set()
    for mode in U.GEO_MODES:
        for nmaps, n1, n2, diag, cap in [(35, 7, 5, 0, 0), (35, 7, 5, 0, 3), (41, 41, 41, 1, 3),
                                         (1, 1, 1, 0, 3), (3000, 60, 50, 0, 0)]:
            a = U.conv_args(geo, nmaps, n1, n2, mode, diag=diag, max_groups=cap, channels=3)
            p = U.plan(a, dtn)
            assert p[0] == 1, (case, dtn, mode, p)
            check_counts(p, nmaps, cap)
            mpcs.add(p[1])
    assert len(mpcs) == 1          # the chunk size is the geometry's, whatever the fusion


def test_plan_table_is_the_whole_table():
    assert len(U.GEOS) == len(set(U.GEOS)) == 18


# (h, w, spec arguments, mode, extra ConvArgs fields): everything the compiled kernel declines
GENERIC_CASES = {
    "generic_flag": (28, 28, (3,), "post", dict(flags=N.CGP_FLAG_GENERIC_CONV)),
    "exact_relu": (28, 28, (3,), "post", dict(flags=N.CGP_FLAG_EXACT_RELU)),
    "exact_relu_no_relu": (14, 14, (3,), "none", dict(flags=N.CGP_FLAG_EXACT_RELU)),
    "maps_per_block": (28, 28, (3,), "none", dict(mpb=1)),
    "maps_per_block_2": (7, 7, (3,), "post_add", dict(mpb=2)),
    "dilation_2": (28, 28, (3, 1, 2), "none", {}),
    "off_table_12_k5": (12, 12, (5,), "none", {}),
    "off_table_28_k5": (28, 28, (5,), "post", {}),
    "off_table_14_wide": (14, 28, (3,), "none", {}),
    "off_table_28_k3_pad0": (28, 28, (3, 1, 1, 0), "none", {}),
    "prerelu_without_post": (28, 28, (3,), "prerelu", {}),
    "prerelu_post_add": (28, 28, (3,), "prerelu_post_add", {}),
    "prerelu_post_add_7": (7, 7, (3,), "prerelu_post_add", {}),
}


@pytest.mark.parametrize("dtn", DTYPES)
@pytest.mark.parametrize("name", list(GENERIC_CASES))
def test_plan_reports_the_generic_kernel(name, dtn):
    h, w, spec, mode, extra = GENERIC_CASES[name]
    geo = U.geometry(h, w, U.conv_spec(*spec))
    for nmaps, n1, n2, cap in [(35, 7, 5, 0), (35, 7, 5, 3), (2, 2, 1, 3)]:
        a = U.conv_args(geo, nmaps, n1, n2, mode, max_groups=cap, **extra)
        p = U.plan(a, dtn)
        assert p[0] == 0, (name, dtn, p)
        check_counts(p, nmaps, cap)
        if extra.get("mpb"):
            assert p[1] == extra["mpb"]


@pytest.mark.parametrize("dtn", DTYPES)
def test_max_groups_caps_the_grid_and_keeps_the_kernel(dtn):
    for case, flags in [((28, 3, 1), 0), ((7, 3, 1), 0), ((28, 3, 1), N.CGP_FLAG_GENERIC_CONV)]:
        geo = geo_of(case)
        free = U.plan(U.conv_args(geo, 5000, 100, 50, "post_add", flags=flags), dtn)
        for cap in (1, 2, 3, 7, 10 ** 6):
            p = U.plan(U.conv_args(geo, 5000, 100, 50, "post_add", flags=flags,
                                   max_groups=cap), dtn)
            assert p[:3] == free[:3]                 # a cap changes the grid and nothing else
            assert p[0] == (0 if flags else 1)
            assert p[3] == min(free[3], cap)


@pytest.mark.parametrize("dtn", DTYPES)
def test_negative_max_groups_is_rejected_by_plan_and_launch(dtn):
    lib = N.load()
    for case, flags in [((28, 3, 1), 0), ((28, 3, 1), N.CGP_FLAG_GENERIC_CONV)]:
        a = U.conv_args(geo_of(case), 35, 7, 5, "none", flags=flags, max_groups=-1)
        rc, out = U.plan_rc(a, dtn)
        assert rc == U.EINVAL and out == [-1] * 4
        assert b"max_groups" in lib.cgp_last_error()
        # the launch entry point rejects it in the same check, before any device call
        assert getattr(lib, f"cgp_conv_{dtn}")(ctypes.byref(a), None) == U.EINVAL
        assert b"max_groups" in lib.cgp_last_error()


@pytest.mark.parametrize("dtn", DTYPES)
def test_plan_runs_the_checks_of_the_launch(dtn):
    lib = N.load()
    fn = getattr(lib, f"cgp_conv_plan_{dtn}")
    out = (ctypes.c_int32 * 4)()
    assert fn(None, out) == U.EINVAL
    assert fn(ctypes.byref(N.ConvArgs()), out) == U.EINVAL
    assert b"NULL" in lib.cgp_last_error()
    geo = geo_of((28, 3, 1))
    assert fn(ctypes.byref(U.conv_args(geo, 35, 7, 5)), None) == U.EINVAL
    a = U.conv_args(geo, 35, 7, 5)
    a.ho = 30
    assert U.plan_rc(a, dtn)[0] == U.EINVAL
    assert b"inconsistent" in lib.cgp_last_error()
    a = U.conv_args(geo, 35, 7, 6, "post")          # nmaps != n1·n2
    assert U.plan_rc(a, dtn)[0] == U.EINVAL
    a = U.conv_args(geo, 35, 7, 5, "post")
    a.post_yy = None
    assert U.plan_rc(a, dtn)[0] == U.EINVAL
    a = U.conv_args(geo, 35, 7, 5, mpb=-1)
    assert U.plan_rc(a, dtn)[0] == U.EINVAL
    # a map too large for the generic kernel's LDS: the launch's own refusal
    big = U.geometry(200, 200, U.conv_spec(3))
    assert U.plan_rc(U.conv_args(big, 2, 2, 1), dtn)[0] == U.EINVAL
    assert b"LDS" in lib.cgp_last_error()


def test_walk_counts_meet_the_walk_conditions():
    for mpc in range(1, 65):
        for form in ("pairs", "diag", "same"):
            nmaps, n1, n2 = U.walk_counts(mpc, form)
            chunks = -(-nmaps // mpc)
            assert chunks >= 17 and chunks % U.CAP == U.walk_remainder(mpc, form)
            assert mpc == 1 or nmaps % mpc != 0
            assert nmaps == (n1 if form == "diag" else n1 * n2)
            if form == "pairs":
                assert n2 >= 2 and mpc % n2 != 0
