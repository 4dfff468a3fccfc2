"""Known answers of the two things the device-noise oracle case (test_gpu_oracle_legs.py) rests on: the numpy Philox-4x32-10
reference (tests/philox_ref.py) against the published Random123 answers, and the oracle's noise_given option, under which
advance_qg takes the NOISE field as set instead of drawing it from the serial rand() stream."""
import numpy as np
import pytest

import golden_cases as gc
import orc
import philox_ref as ph


# Random123's kat_vectors, philox4x32 with 10 rounds: counter, key -> output
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    assert tuple(int(w) for w in ph.philox4x32_10(ctr, key)) == want


def test_philox_reference_vectorised_equals_scalar():
    """the array form (one counter per cell) gives what the scalar form gives cell by cell"""
    cells = np.array([0, 1, 4095, 2 ** 24 + 3, 0xffffffff], dtype=np.uint64)
    got = ph.philox4x32_10((cells, 2, 5, ph.CTR_W), (7, ph.KEY_1))
    for n, c in enumerate(cells):
        one = ph.philox4x32_10((int(c), 2, 5, ph.CTR_W), (7, ph.KEY_1))
        assert [int(w[n]) for w in got] == [int(w) for w in one]


def test_noise_reference_tile_offsets_and_moments():
    """a tile at (gx0, gy0) is the same window of the global field; counters of other layers, draws and seeds differ"""
    nl, n = 3, 64
    sig = np.ones((nl, n, n))
    full = ph.noise(sig, 1.0, 7, 0)
    tile = ph.noise(sig[:, :32, :16], 1.0, 7, 0, gx0=48, gy0=32, gnx=n)
    assert np.array_equal(tile, full[:, 32:, 48:])
    for other in (ph.noise(sig, 1.0, 7, 1), ph.noise(sig, 1.0, 8, 0)):
        assert np.abs(other - full).max() > 1.0
    assert np.abs(full[0] - full[1]).max() > 1.0
    assert abs(full.mean()) < 5 / np.sqrt(full.size) and abs(full.var() - 1) < 5 * np.sqrt(2 / full.size)


def test_oracle_noise_given_off_reproduces_the_srand7_golden():
    """with noise_given = 0 (the default) the stochastic run is unchanged: the committed serial-rand() fixture, bit for bit"""
    got, exp = gc.run_case("stochastic_srand7_16x16x3", lambda txt, **o: gc.OracleModel(txt, noise_given=0, **o))
    gc.compare(got, exp, exact=True)


def test_oracle_noise_given_advance():
    """noise_given = 1: the predictor advance is in + dq dt + n dts with dts = float(sqrt(dt)) / sqrt(2) rounded to float
    (msqg/qg_stochastic.h:128-149), the corrector uses float(sqrt(dt)); NOISE is used as set and not redrawn"""
    N, nl, dt = 16, 3, 0.0123
    o = orc.Oracle(orc.double_gyre_params(N, nl, extra="tr_stoch = 50\namp_stoch = 1e-5\n"), quiet=1, stochastic=1)
    o.set(orc.PSI, orc.synthetic_psi(nl, N, N))
    o.set_const()
    rng = np.random.default_rng(31)
    q0, dq, n = (rng.standard_normal((nl, N, N)) for _ in range(3))
    o.set_noise(n)
    o.set(orc.Q, q0)
    o.set(orc.DQ, dq)
    o.advance(orc.Q, orc.Q, orc.DQ, dt)
    q1 = o.get(orc.Q)
    dts = np.float64(np.float32(np.float64(np.float32(np.sqrt(dt))) / np.sqrt(2.0)))
    assert np.array_equal(q1, q0 + dq * dt + n * dts)
    assert np.array_equal(o.get(orc.NOISE), n)
    o.advance(orc.Q, orc.Q, orc.DQ, dt)
    assert np.array_equal(o.get(orc.Q), q1 + dq * dt + n * np.float64(np.float32(np.sqrt(dt))))
    # the option matters: without it the predictor draws new noise
    o.option("noise_given", 0)
    o.advance(orc.Q, orc.Q, orc.DQ, dt)
    assert not np.array_equal(o.get(orc.NOISE), n)
