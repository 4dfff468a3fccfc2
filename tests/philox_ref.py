"""Plain numpy reference of the device noise generator (noise_mode = 1, k_noise in kernels_rhs.hip).  Test infrastructure only.

Philox-4x32-10 as defined by Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11): ten
rounds of two 32x32 -> 64-bit multiplications with the multipliers 0xD2511F53 / 0xCD9E8D57; the key is bumped by the Weyl
constants 0x9E3779B9 / 0xBB67AE85 between rounds.  The noise of one cell-layer uses the counter
(global cell j * gnx + i, layer, draw, 0x6d736f6d) and the key (seed, 0x4d493335), and then the reference's Box-Muller
formula (msqg/qg_stochastic.h:9) on the top 31 bits of the first two output words, i.e. on rand()-sized uniforms."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
CTR_W = 0x6d736f6d      # "msom"
KEY_1 = 0x4d493335      # "MI35"
RAND_MAX = 2147483647


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2 words; returns the 4 output words as uint64 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k0, k1 = (np.uint64(int(k) & MASK) for k in key)
    m0, m1, w0, w1, mask = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1), np.uint64(MASK)
    for r in range(10):
        if r:
            k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
        p0, p1 = m0 * c[0], m1 * c[2]         # < 2^64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
    return c


def noise(sigma, amp, seed, draw, gx0=0, gy0=0, gnx=None, radius=False):
    """amp * sigma * N(0, 1) on a tile [nl, ny, nx] whose first cell is global cell (gx0, gy0) of a grid gnx cells wide;
    radius: also the Box-Muller radius sqrt(-2 log u) of every cell-layer"""
    nl, ny, nx = sigma.shape
    gnx = nx if gnx is None else gnx
    j, i = np.meshgrid(np.arange(ny, dtype=np.uint64), np.arange(nx, dtype=np.uint64), indexing="ij")
    cell = ((np.uint64(gy0) + j) * np.uint64(gnx) + np.uint64(gx0) + i) & np.uint64(MASK)
    out, rad = np.empty((nl, ny, nx)), np.empty((nl, ny, nx))
    for l in range(nl):
        w = philox4x32_10((cell, l, draw, CTR_W), (seed, KEY_1))
        r1 = (w[0] >> np.uint64(1)).astype(np.float64)
        r2 = (w[1] >> np.uint64(1)).astype(np.float64)
        rad[l] = np.sqrt(-2.0 * np.log((r1 + 1.0) / (RAND_MAX + 2.0)))
        out[l] = amp * sigma[l] * (rad[l] * np.cos(2 * np.pi * r2 / RAND_MAX))
    return (out, rad) if radius else out
