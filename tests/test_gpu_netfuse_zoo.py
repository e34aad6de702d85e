"""The whole-network kernel (csrc/netfuse.hip) on networks outside the reference configs
(tests/net_zoo.py): op lists that only the op-record interpreter runs — dirty scratch
zero rows, LINEAR and full-map reductions in 4- and 16-pair stages, heads that only load
the moments, halo zeroings in every stage shape — against the CPU oracle, the layer path
and themselves.

Small tiles cannot see stale LDS: a launch has min(occupancy x CUs, groups) workgroups
(rounded up to 8), LDS is zeroed once per workgroup, and a 7 x 17 or 9 x 9 tile has fewer
groups than that, so every pair runs on fresh zeros.  test_zoo_steady_state_walk sizes its
tile from the occupancy so that workgroups must walk on to a second and third group.
"""
import functools
import math

import numpy as np
import pytest
import torch

import configs_util
import net_zoo
from cnn_gp import _native as N
from cnn_gp import netplan
from oracle import nngp_oracle as O

from test_gpu_parity import DEV, RTOL32, RTOL64, rel_err

pytestmark = pytest.mark.gpu


def dev(a, dt=torch.float64):
    return torch.tensor(a).to(DEV, dt)          # a copy: the shared inputs are read-only


ZOO = net_zoo.zoo()
WALK_NETS = ["mix74", "to14blocks", "to16blocks", "in14", "in16mix3", "in8mix", "nested"]
MODES = {"f64-fast": (torch.float64, False, RTOL64["fast"]),
         "f64-exact": (torch.float64, True, RTOL64["exact"]),
         "f32": (torch.float32, False, RTOL32)}


def model_of(name, dt, exact=False):
    """a fresh model on the device (no cached plan or tile recipe)"""
    return ZOO[name].build().to(DEV, dt).set_exact_relu(exact)


def images(name, n, seed):
    """float32-representable images: the float64 oracle on them serves every mode"""
    z = ZOO[name]
    rng = np.random.default_rng(seed)
    a = rng.random((n, z.channels, z.side, z.side), dtype=np.float32).astype(np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def small_case(name):
    """inputs and the oracle's Kxz (7 x 17), Kxx (9 images) and 1 x 1, once per net"""
    X, Z = images(name, 9, 40), images(name, 17, 41)
    spec = configs_util.spec_of(ZOO[name].build())
    ref = {"Kxz": O.kernel(spec, X[:7], Z, False, False), "Kxx": O.kernel(spec, X),
           "K11": O.kernel(spec, X[:1], Z[:1], False, False)}
    for a in ref.values():
        a.setflags(write=False)
    return X, Z, ref


def small_tiles(m, X, Z, dt):
    with torch.no_grad():
        x, z = dev(X, dt), dev(Z, dt)
        return {"Kxz": m(x[:7], z, False, False).cpu().numpy(), "Kxx": m(x).cpu().numpy(),
                "K11": m(x[:1], z[:1], False, False).cpu().numpy()}


@pytest.mark.parametrize("itemsize", [8, 4])
@pytest.mark.parametrize("name", net_zoo.NAMES)
def test_zoo_routes_to_the_fused_kernel(name, itemsize):
    z = ZOO[name]
    m = model_of(name, torch.float64 if itemsize == 8 else torch.float32)
    net = m._net_plan(m._plan(z.side, z.side), itemsize)
    assert net is not None
    assert z.feature(net), (z.purpose, net_zoo.layout(net))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", net_zoo.NAMES)
def test_zoo_small_tiles_match_oracle(name, mode):
    """Kxz 7 x 17, Kxx on 9 images and a 1 x 1 call in the three numerics (the exact ReLU
    runs the unstaged one-pair program)"""
    dt, exact, tol = MODES[mode]
    X, Z, ref = small_case(name)
    m = model_of(name, dt, exact)
    assert m._net_plan(m._plan(X.shape[2], X.shape[3]), 8 if dt == torch.float64 else 4) \
        is not None
    got = small_tiles(m, X, Z, dt)
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print(f"zoo {name} {mode}: worst rel err vs oracle {max(errs.values()):.2e} {errs}")
    assert np.array_equal(got["Kxx"], got["Kxx"].T)
    for k, e in errs.items():
        assert e < tol, (name, mode, k, e)


@pytest.mark.parametrize("name", ["in14", "in8mix"])
def test_zoo_zero_variance_pixels_match_oracle(name):
    """MNIST-like images (zero borders, ~60% zero pixels, an all-zero image) through a
    4-pair and a 16-pair stage: zero-variance pixels of the bias-free convs take the
    f32_tiny path like the reference"""
    z = ZOO[name]
    rng = np.random.default_rng(21)
    X = np.floor(rng.random((6, z.channels, z.side, z.side)) * 256) / 255.0
    X[rng.random(X.shape) < 0.6] = 0.0
    b = z.side // 7
    X[:, :, :b, :] = 0.0
    X[:, :, -b:, :] = 0.0
    X[:, :, :, :b] = 0.0
    X[:, :, :, -b:] = 0.0
    X[3] = 0.0
    Z = X[::-1].copy()
    m = model_of(name, torch.float64)
    spec = configs_util.spec_of(m)
    got = m(dev(X), dev(Z), False, False).cpu().numpy()
    np.testing.assert_allclose(got, O.kernel(spec, X, Z, False, False), rtol=RTOL64["fast"],
                               atol=1e-300)
    gxx = m(dev(X)).cpu().numpy()
    np.testing.assert_allclose(gxx, O.kernel(spec, X), rtol=RTOL64["fast"], atol=1e-300)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", net_zoo.NAMES)
def test_zoo_fused_matches_layer_path(name, dtn):
    """the layer-by-layer pipeline shares no LDS code with the fused kernel: fp64 within
    1e-12, fp32 within RTOL32"""
    dt = torch.float64 if dtn == "f64" else torch.float32
    X, Z, _ = small_case(name)
    a = small_tiles(model_of(name, dt), X, Z, dt)
    b = small_tiles(model_of(name, dt).set_fused_network(False), X, Z, dt)
    for k in a:
        assert rel_err(a[k], b[k]) < (1e-12 if dtn == "f64" else RTOL32), (name, dtn, k)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", net_zoo.NAMES)
def test_zoo_first_stage_pairs_bit_equal(name, dtn, monkeypatch):
    """the head stage on one pair per workgroup and on two one-pair halves: bit-equal"""
    dt = torch.float64 if dtn == "f64" else torch.float32
    X, Z, _ = small_case(name)
    out = {}
    for first in ("1", "2"):
        monkeypatch.setattr(netplan, "FIRST_PAIRS", first)
        m = model_of(name, dt)
        net = m._net_plan(m._plan(X.shape[2], X.shape[3]), 8 if dtn == "f64" else 4)
        assert net is not None and net.stages[0].pairs == int(first)
        out[first] = small_tiles(m, X, Z, dt)
    for k in out["1"]:
        assert np.array_equal(out["1"][k], out["2"][k], equal_nan=True), (name, dtn, k)


# -- a tile large enough that workgroups walk past their first group ------------------------
def walk_need(net, itemsize):
    """units a tile needs so that every stage has at least 3 groups per workgroup of a
    full grid: max over the stages of 3 x grid x units per group, grid = occupancy x CUs
    rounded up to 8 (net_launch)"""
    lib = N.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = []
    for st in net.stages:
        occ = lib.cgp_net_occupancy(st.lds_elems * itemsize, int(itemsize == 8),
                                    N.CGP_FLAG_NET_DUAL if st.dual else 0, st.pairs)
        assert occ > 0, (st.pairs, st.lds_elems)
        grid = -(-occ * cus // 8) * 8
        need.append(3 * grid * lib.cgp_net_units(st.pairs))
    return need


@functools.lru_cache(maxsize=None)
def walk_case(name):
    """the walk tile's side (whole 8 x 8 supertiles, so every unit is a pair that is
    evaluated; the same side for fp64 and fp32: the larger of the two), its images, the
    positions checked against the oracle and the oracle's values there"""
    z = ZOO[name]
    st = N.load().cgp_net_supertile()
    need = {}
    for itemsize in (8, 4):
        m = model_of(name, torch.float64 if itemsize == 8 else torch.float32)
        need[itemsize] = walk_need(m._net_plan(m._plan(z.side, z.side), itemsize), itemsize)
    most = max(max(v) for v in need.values())
    nb = math.isqrt(-(-most // (st * st)) - 1) + 1
    n = st * nb
    X, Z = images(name, n, 50), images(name, n, 51)
    units = nb * nb * st * st
    # corner blocks, and 64 units around every boundary between the 8 XCD ranges (a
    # stage's boundary is units / 8 rounded up to its units per group, at most 15 further)
    ij = [(i0 + a, j0 + b) for i0 in (0, n - 8) for j0 in (0, n - 8)
          for a in range(8) for b in range(8)]
    for x in range(1, 8):
        for u in range(x * units // 8 - 32, x * units // 8 + 32):
            s, q = divmod(u, st * st)
            ij.append((s // nb * st + q // st, s % nb * st + q % st))
    I, J = (np.array(v) for v in zip(*ij))
    ref = O.kernel(configs_util.spec_of(z.build()), X[I], Z[J], False, True)
    ref.setflags(write=False)
    return n, need, X, Z, I, J, ref


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", WALK_NETS)
def test_zoo_steady_state_walk(name, dtn):
    """a Kxz tile with at least 3 groups per workgroup in every stage, so workgroups
    evaluate pairs on the LDS an earlier pair left behind (halo zeroing, scratch zero
    rows, slot reuse, the reduction's partial-sum cells): 64 random entries are bit-equal
    to the same pair evaluated alone (a 1 x 1 call, fresh LDS), the corners and the pairs
    around every XCD range boundary match the oracle, and a same tile of half the side is
    symmetric with the variance chain on its diagonal.

    Observed on an MI355X (256 CUs; profiles/zoo/zoo_alone.log).  Workgroups per CU: 4-5
    in a two-pair head, 8 (fp64) or 10 (fp32) in a 4-pair stage, 6-8 (fp64) or 10 (fp32)
    in a 16-pair stage, so the units needed are at most 7680, 30720 and 122880 and the
    sides 88 (mix74, nested), 176 (to14blocks, to16blocks) and 352 (in14, in16mix3,
    in8mix).  With the halo zeroings of one stage dropped from the plan (a one-off run,
    profiles/zoo/zoo_mutation.log) the small tiles still matched the oracle to 7e-15 and
    36 to 55 of the 64 entries here differed from their 1 x 1 call."""
    z = ZOO[name]
    dt = torch.float64 if dtn == "f64" else torch.float32
    itemsize = 8 if dtn == "f64" else 4
    n, need, X, Z, I, J, ref = walk_case(name)
    m = model_of(name, dt)
    net = m._net_plan(m._plan(z.side, z.side), itemsize)
    assert z.feature(net)
    units = net.units(n, n, False)
    print(f"zoo walk {name} {dtn}: side {n}, units {units}, needed per stage "
          f"{dict(zip(net_zoo.pairs(net), need[itemsize]))}")
    assert all(units >= v for v in need[itemsize]) and n <= 512, (n, units, need)
    tol = RTOL64["fast"] if dtn == "f64" else RTOL32
    with torch.no_grad():
        x, y = dev(X, dt), dev(Z, dt)
        K = m(x, y, False, False)
        rng = np.random.default_rng(52)
        for a, b in rng.integers(0, n, size=(64, 2)):
            one = m(x[a:a + 1], y[b:b + 1], False, False)
            assert torch.equal(K[a:a + 1, b:b + 1], one), (a, b, K[a, b].item(), one.item())
        err = rel_err(K.cpu().numpy()[I, J], ref)
        print(f"zoo walk {name} {dtn}: worst rel err vs oracle on {len(I)} pairs {err:.2e}")
        assert err < tol
        h = n // 2
        Kxx = m(x[:h])
        assert torch.equal(Kxx, Kxx.T)
        d = m(x[:h], x[:h], True, True)
        assert rel_err(torch.diagonal(Kxx).cpu().numpy(), d.cpu().numpy()) < 1e-13


def test_zoo_chunked_state_bit_equal(monkeypatch):
    """in16mix3's walk tile with the state buffers cut into at least 3 launch groups (a
    unit range and a range-relative state index per launch): bit-equal to one group"""
    name = "in16mix3"
    z = ZOO[name]
    n, _, X, Z, _, _, _ = walk_case(name)
    with torch.no_grad():
        x, y = dev(X), dev(Z)
        whole = model_of(name, torch.float64)(x, y, False, False)
        m = model_of(name, torch.float64)
        net = m._net_plan(m._plan(z.side, z.side), 8)
        units = net.units(n, n, False)
        assert net.chunk_units(8, units) == units
        stride = max(max(st.load_stride, st.store_stride) for st in net.stages)
        monkeypatch.setattr(netplan, "CHUNK_BYTES", units // 3 // 64 * 64 * stride * 8)
        chunk = net.chunk_units(8, units)
        assert -(-units // chunk) >= 3
        cut = m(x, y, False, False)
    assert torch.equal(whole, cut)
