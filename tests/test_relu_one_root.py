"""CPU check of the one-root form of the fp64 closed-form ReLU (csrc/cgp_common.h relu_q_n,
CGP_RELU_ONE_ROOT=1): a restatement of the kernel's op sequence, operation by operation
and with its exact scalings, against the 50-digit map of test_relu_closed_form.py.

    m  = 1/sqrt(v/8)                 per image and pixel (cgp_rsqrt_batch_f64)
    Y  = min(m1·m2, 2^66)            8/sqrt(t); the cap is t = f32_tiny
    x4 = max(fma(-|c/4|, Y, 2), 2^-51)
    z  = (x4·Y)·Y                    256·x/t
    R  = h·fma(-(z·h), h, 3)         h = the hardware estimate of 1/sqrt(z); R = 2/sqrt(z)
    out = fma((x4·x4)·R, P̃(x4), c/4 + |c/4|),   P̃(x4) = P(x4/4)/2 by Horner in fma

Every fma below is a true fused multiply-add (exact product and sum, one rounding), and
the estimate h carries a 5e-8 relative error like v_rsq_f64's."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from oracle import nngp_oracle as O

from conftest import PKG
from test_relu_closed_form import adapt_tables, coeffs, exact_dec

COMMON = os.path.join(PKG, "csrc", "cgp_common.h")
BOUND = 1e-12               # test_relu_closed_form.py's bound of the closed form
EST_ERR = 5e-8              # relative error of the hardware reciprocal square root estimate
Y_MAX = 2.0 ** 66
X4_MIN = 2.0 ** -51


def fma(a, b, c):
    if not all(np.isfinite(v) for v in (a, b, c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def poly_q():
    """kPolyQ of the one-root form as the header states it"""
    txt = open(COMMON).read()
    m = re.search(r"kPolyQ = CGP_RELU_ONE_ROOT \? ([0-9.]+) :", txt)
    assert m and int(re.search(r"#define CGP_RELU_ONE_ROOT (\d)", txt).group(1)) == 1
    return float(m.group(1))


def scaled(p):
    """coefficient k of P̃(x4): p[k]·kPolyQ·4^-k (adapt_coef / poly_q of cgp_common.h)"""
    return [v * poly_q() * 0.25 ** k for k, v in enumerate(p)]


def tables():
    """(xmax, P̃ coefficients) of the three adaptive fits and the full one on [0, 1/2]"""
    return [(xm, scaled(p)) for xm, p in adapt_tables(1)] + [(0.5, scaled(coeffs("D")))]


def rsqrt8(v):
    """the device's var_rsqrt8: an exact scaling, a correctly rounded sqrt and division"""
    with np.errstate(divide="ignore"):
        return float(np.float64(1.0) / np.sqrt(np.float64(v) * 0.125))


def one_root(c, v1, v2, tab, rng):
    """relu_q_n's one-root sequence on one pixel; returns (out, x4)"""
    cq = c * 0.25
    m1, m2 = rsqrt8(v1), rsqrt8(v2)
    Y = min(m1 * m2, Y_MAX)
    u = max(fma(-abs(cq), Y, 2.0), X4_MIN)
    z = (u * Y) * Y
    h = (1.0 / np.sqrt(z)) * (1.0 + EST_ERR * rng.uniform(-1, 1))
    m = z * h
    r2 = h * fma(-m, h, 3.0)
    sx = (u * u) * r2
    p = fma(tab[-1], u, tab[-2])
    for k in range(len(tab) - 3, -1, -1):
        p = fma(p, u, tab[k])
    return fma(sx, p, cq + abs(cq)), u


def table_for(x4, tabs):
    """the shortest polynomial whose interval holds the pixel (the vote of one pixel)"""
    for xm, t in tabs:
        if x4 < 4.0 * xm:
            return t
    return tabs[-1][1]


def check(c, v1, v2, tabs, rng, forced=None):
    t = v1 * v2 + O.F32_TINY
    ref = exact_dec(c, v1, v2)
    # the vote needs x4 first: the kernel computes it before it picks a table
    _, x4 = one_root(c, v1, v2, tabs[-1][1], rng)
    tab = forced if forced is not None else table_for(x4, tabs)
    got, _ = one_root(c, v1, v2, tab, rng)
    assert abs(got - ref) <= BOUND * np.sqrt(t), (c, v1, v2, got, ref)


def test_grid_against_50_digit_map():
    """test_relu_closed_form.py's grid (300 log-normal variance pairs, rho in ±0.999), each
    pixel through the table its x selects"""
    tabs = tables()
    rng = np.random.default_rng(1)
    for _ in range(300):
        v1, v2 = rng.lognormal(0, 1, 2)
        rho = rng.uniform(-0.999, 0.999)
        check(rho * np.sqrt(v1 * v2), v1, v2, tabs, rng)


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_every_table_on_its_interval(idx):
    """each adaptive table, and the full one, on the whole of its own interval (a wave
    takes a table for all its pixels, so small x also runs the long ones)"""
    tabs = tables()
    xmax, tab = tabs[idx]
    rng = np.random.default_rng(10 + idx)
    xs = np.concatenate([np.linspace(0.0, xmax, 65)[1:-1], xmax * 10.0 ** -np.arange(1, 16),
                         [xmax * (1 - 2.0 ** -20)]])
    for x in xs:
        for sign in (1.0, -1.0):
            v1, v2 = rng.lognormal(0, 1, 2)
            c = sign * (1 - 2 * x) * np.sqrt(v1 * v2)
            _, x4 = one_root(c, v1, v2, tab, rng)
            if x4 < 4.0 * xmax or idx == 3:      # the vote would admit this pixel
                check(c, v1, v2, tabs, rng, forced=tab)


def test_near_one_and_ends():
    """1 - |rho| = 10^-k for k = 1..15, rho = ±1 and c = 0, over v from 1e-12 to 1e12"""
    tabs = tables()
    rng = np.random.default_rng(3)
    vs = [1e-12, 1e-6, 0.37, 1.0, 41.0, 1e6, 1e12]
    for v1 in vs:
        for v2 in (v1, 2.9, vs[len(vs) - 1 - vs.index(v1)]):
            s = np.sqrt(v1 * v2)
            for k in range(1, 16):
                for sign in (1.0, -1.0):
                    check(sign * (1 - 10.0 ** -k) * s, v1, v2, tabs, rng)
            for c in (s, -s, 0.0, np.nextafter(s, np.inf), -np.nextafter(s, np.inf)):
                check(c, v1, v2, tabs, rng)


def test_zero_variance_is_exactly_tiny():
    """v1 = 0, v2 = 0 and both: m = +inf, Y capped at 2^66, so t is exactly f32_tiny and
    the map gives sqrt(tiny)/(2 pi), as the reference's `+ f32_tiny` does"""
    tabs = tables()
    rng = np.random.default_rng(4)
    want = np.sqrt(O.F32_TINY) / (2 * np.pi)
    assert abs(want - 1.72556135e-20) / want < 1e-8
    assert (8.0 / Y_MAX) ** 2 == O.F32_TINY
    for v1, v2 in ((0.0, 3.0), (3.0, 0.0), (0.0, 0.0), (0.0, 1e12), (1e-12, 0.0)):
        got, x4 = one_root(0.0, v1, v2, tabs[-1][1], rng)
        assert x4 == 2.0
        assert abs(got - want) / want < 1e-9, (v1, v2, got)


def test_new_entry_points_check_arguments_on_the_host():
    """cgp_rsqrt_batch_f64 refuses bad arguments before any launch (1001, not the 1002 a
    launch without a GPU would give), a bad buffer behind a full first launch included; the
    default build reports the rsqrt map form"""
    import ctypes
    from cnn_gp import _native as N
    lib = N.load()
    assert lib.cgp_net_var_form() == N.CGP_VAR_FORM_RSQRT
    assert lib.cgp_rsqrt_batch_f64(2, None, None, None, None) == 1001
    assert lib.cgp_rsqrt_batch_f64(-1, None, None, None, None) == 1001
    assert lib.cgp_rsqrt_batch_f64(0, None, None, None, None) == 0
    k = 34
    for bad_n, bad_p in ((-1, 16), (5, 0)):
        src = (ctypes.c_void_p * k)(*([16] * (k - 1) + [bad_p]))
        dst = (ctypes.c_void_p * k)(*([32] * k))
        n = (ctypes.c_int64 * k)(*([4] * (k - 1) + [bad_n]))
        assert lib.cgp_rsqrt_batch_f64(k, src, dst, n, None) == 1001
        assert b"buffer 33" in lib.cgp_last_error()
