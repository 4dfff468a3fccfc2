"""Device noise generator of the vertex model (option noise_mode = 1: k_n_noise in kernels_node.hip, msomn_noise_draw).

The draw is held to the numpy restatement of the generator (philox_ref.py: the cell-centred model's k_noise with layer 0 on a
grid N cells wide), its ghost ring and the filter to the vertex oracle given the device's draw, a hand-composed stochastic
predictor-corrector pair to the oracle given the device's filtered noise (the oracle's own step draws from rand()), and the
handles to each other.  strict build: bit-exact (np.array_equal); product build: the tolerance stated per test."""
import ctypes

import numpy as np
import pytest

import orn
import philox_ref as ph
from msom_amd import MsomError, NodeQG
from test_gpu_node_parity import same

pytestmark = pytest.mark.gpu

AMP, SEED = 0.3, 5


def params(N, L_filt=8.0):
    return orn.node_params(N, 1, bc_fac=1.0, extra=f"gp_low = 0.02\namp_stoch = {AMP}\nL_filt = {L_filt}\n")


def handle(N, L_filt=8.0, strict=False, seed=SEED, mode=1, seed_first=True):
    g = NodeQG(params(N, L_filt), strict=strict)
    for k, v in (("quiet", 1), ("stochastic", 1), ("TOLERANCE", 1e-9)):
        g.set_option(k, v)
    for k, v in (("seed", seed), ("noise_mode", mode)) if seed_first else (("noise_mode", mode), ("seed", seed)):
        g.set_option(k, v)
    g.set("PSI", orn.node_psi(1, N))
    g.set_const()
    return g


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("N", [8, 32, 128])
def test_draws_against_the_numpy_reference(N, strict):
    """draws 0, 1, 2 elementwise: |n - ref| <= 1e-14 amp (a + 1), a the Box-Muller radius (the bound of
    test_gpu_oracle_legs.py::check_noise: device log / cos may differ from the host's by an ulp; a wrong counter, key or draw
    differs by O(amp)); the draw counter counts, and set_const rewinds it"""
    g = handle(N, strict=strict)
    assert (g.param("noise_mode"), g.param("seed")) == (1.0, float(SEED))
    seq = []
    for draw in range(3):
        assert g.param("noise_draw") == draw
        g.noise_draw(filter=False)
        n = g.noise()
        ref, a = ph.noise(np.ones((1, N, N)), AMP, SEED, draw, radius=True)
        d = np.abs(n - ref[0]) / (AMP * (a[0] + 1))
        print(f"N={N} strict={strict} draw {draw}: max |n - ref| / (amp (a + 1)) = {d.max():.3g}")
        assert np.all(d <= 1e-14), (draw, float(d.max()))
        seq.append(n)
    assert g.param("noise_draw") == 3
    assert np.abs(seq[1] - seq[0]).max() > AMP and np.abs(seq[2] - seq[1]).max() > AMP
    g.set_const()
    assert g.param("noise_draw") == 0
    for draw in range(3):
        g.noise_draw(filter=False)
        assert np.array_equal(g.noise(), seq[draw])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("N,L_filt", [(64, 8.0), (32, 20.0), (128, 1e6)])
def test_ghost_ring_and_filter_against_the_oracle(N, L_filt, strict):
    """the filtered draw against the oracle's filter of the same unfiltered draw (tolerance of test_stochastic_forcing); the
    reconstruction reads ghost cells, so the strict build is bit-exact only if k_n_noise's ring is the one the ghost fill writes"""
    o = orn.NodeOracle(params(N, L_filt), smoother=orn.GS_RB, quiet=1, stochastic=1, TOLERANCE=1e-9)
    o.set(orn.PSI, orn.node_psi(1, N))
    o.set_const()
    g = handle(N, L_filt, strict)
    g.noise_draw(filter=False)
    n0 = g.noise()
    o.set_noise(n0); o.filter_noise()
    g2 = handle(N, L_filt, strict)
    g2.noise_draw(filter=True)
    same(g2.noise(), o.noise(), strict, 1e-13)
    assert np.abs(o.noise()).max() > 0


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("N", [32, 64])
def test_stochastic_rk2_pair_against_the_oracle(N, strict):
    """three predictor-corrector steps composed from update / advance on both sides.  GPU: stochastic = 1, noise_mode = 1 (the
    first advance of a step draws, both add).  Oracle: stochastic = 0; after each advance the test adds the device's filtered
    noise of that step to layer 0 with the weights of qg-node/qg.h:306-320 (sqrt(dt/2)/sqrt(2), sqrt(dt)), vertex N <- cell N-1"""
    o = orn.NodeOracle(params(N), smoother=orn.GS_RB, quiet=1, TOLERANCE=1e-9)
    o.set(orn.PSI, orn.node_psi(1, N))
    o.set_const()
    g = handle(N, strict=strict)

    def add_noise(field, dts):
        q = o.get(field)
        q[0] += np.pad(g.noise(), ((0, 1), (0, 1)), mode="edge") * dts
        o.set(field, q)

    for step in range(3):
        dt_o, dt_g = o.update(orn.Q, orn.DQ), g.update("Q", "DQ")
        assert dt_g == dt_o or not strict
        g.advance("QPRED", "Q", "DQ", dt_g / 2)
        assert g.param("noise_draw") == step + 1
        o.advance(orn.QPRED, orn.Q, orn.DQ, dt_o / 2)
        add_noise(orn.QPRED, np.sqrt(dt_o / 2) / np.sqrt(2))
        o.update(orn.QPRED, orn.DQ); g.update("QPRED", "DQ")
        g.advance("Q", "Q", "DQ", dt_g)
        assert g.param("noise_draw") == step + 1
        o.advance(orn.Q, orn.Q, orn.DQ, dt_o)
        add_noise(orn.Q, np.sqrt(dt_o))
    same(g.get("Q"), o.get(orn.Q), strict, 1e-7)
    same(g.get("PSI"), o.get(orn.PSI), strict, 1e-7)
    assert np.abs(g.noise()).max() > 0


def test_handles_do_not_share_a_stream():
    """two handles with the same seed drawn in interleaved order give the same sequence bit for bit (whatever the order of the
    options seed and noise_mode), another seed another one; only noise_mode 0 and 1 exist"""
    N = 32
    a, b, c = handle(N), handle(N, seed_first=False), handle(N, seed=SEED + 1)
    sa, sb = [], []
    for h, s in ((a, sa), (b, sb), (b, sb), (a, sa), (a, sa), (b, sb)):
        h.noise_draw(filter=False)
        s.append(h.noise())
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    assert np.abs(sa[1] - sa[0]).max() > AMP
    c.noise_draw(filter=False)
    assert np.abs(c.noise() - sa[0]).max() > AMP
    with pytest.raises(MsomError):
        a.set_option("noise_mode", 2)
    assert a.param("noise_mode") == 1


@pytest.mark.parametrize("strict", [True, False])
def test_mode_0_is_the_rand_stream_as_before(strict):
    """noise_mode = 0 set explicitly: the serial rand() stream parity of test_stochastic_forcing, four steps from srand(11)"""
    libc = ctypes.CDLL(None)
    N, L_filt = 32, 20.0
    o = orn.NodeOracle(params(N, L_filt), smoother=orn.GS_RB, quiet=1, stochastic=1, TOLERANCE=1e-9)
    o.set(orn.PSI, orn.node_psi(1, N))
    o.set_const()
    g = handle(N, L_filt, strict, mode=0)
    for m in (o, g):
        libc.srand(11)
        for _ in range(4):
            m.step(True)
    assert g.param("noise_draw") == 0
    same(g.noise(), o.noise(), strict, 1e-13)
    same(g.get("Q"), o.get(orn.Q), strict, 1e-7)
    same(g.get("PSI"), o.get(orn.PSI), strict, 1e-7)
    assert np.abs(g.noise()).max() > 0
    # msomn_noise_draw in mode 0 draws from the same host stream
    libc.srand(3)
    g.noise_draw(filter=False)
    n = g.noise()
    libc.srand(3)
    g.noise_draw(filter=False)
    assert np.array_equal(g.noise(), n) and np.abs(n).max() > 0 and g.param("noise_draw") == 0


def test_moments():
    """sanity beside the elementwise test: z = n / amp of draws 0..2 at N = 256 (k = N^2 samples).  |mean| sqrt(k),
    |var - 1| sqrt(k / 2) and the mean lag-1 products in x and in y times sqrt(k) are each about N(0, 1): bound 4.  Fixed seed:
    philox_ref alone gives at most 2.4 for these twelve numbers on the CPU"""
    N = 256
    k = N * N
    g = handle(N)
    for draw in range(3):
        g.noise_draw(filter=False)
        z = g.noise() / AMP
        stats = (abs(z.mean()) * np.sqrt(k), abs(z.var() - 1) * np.sqrt(k / 2), abs((z[:, 1:] * z[:, :-1]).mean()) * np.sqrt(k),
                 abs((z[1:] * z[:-1]).mean()) * np.sqrt(k))
        print(f"draw {draw}: mean, var, lag-1 x, lag-1 y in sigmas: " + ", ".join(f"{s:.2f}" for s in stats))
        assert max(stats) <= 4, (draw, stats)
