"""Plain numpy restatement of the running statistics of the vertex model (msomn_stats_*, include/msom.h) in the expression order the
header documents.  No GPU, no library: test infrastructure for tests/test_gpu_node_stats.py.

    u = ((psi[j-1][i] - psi[j+1][i]) / (2 D)) * mask[j][i],   v = ((psi[j][i+1] - psi[j][i-1]) / (2 D)) * mask[j][i]
    u = v = 0 on the boundary ring (i or j in {0, N}); 2 D formed once
    acc = acc + w * x,   x = psi, q, psi*psi, q*q, 0.5 * (u*u + v*v), u*q, v*q,   W = W + w
    mean = acc / W;   um, vm: the same masked differences of the mean psi with psi_bc on its ring
    EKE = mean(KE) - 0.5 * (um*um + vm*vm);   UQ_EDDY = mean(uq) - um * mean(q);   VQ_EDDY = mean(vq) - vm * mean(q)
"""
import numpy as np

ACC = ("PSI", "Q", "PSI2", "Q2", "KE", "UQ", "VQ")
DERIVED = ("EKE", "UQ_EDDY", "VQ_EDDY")
NEEDS = dict(EKE=("PSI", "KE"), UQ_EDDY=("PSI", "Q", "UQ"), VQ_EDDY=("PSI", "Q", "VQ"))


def velocities(psi, mask, D2):
    """masked centred differences on the interior vertices, exactly 0 on the boundary ring; psi [nl][n][n], mask [1][n][n]"""
    u, v = np.zeros(psi.shape), np.zeros(psi.shape)
    m = mask[:, 1:-1, 1:-1]
    u[:, 1:-1, 1:-1] = ((psi[:, :-2, 1:-1] - psi[:, 2:, 1:-1]) / D2) * m
    v[:, 1:-1, 1:-1] = ((psi[:, 1:-1, 2:] - psi[:, 1:-1, :-2]) / D2) * m
    return u, v


class NodeStats:
    """the accumulators of the whole (one-tile) grid; D2 = 2 * (L0 / N), mask [1][N + 1][N + 1]"""

    def __init__(self, nl, N, mask, D2, psi_bc=0.0):
        self.S = {n: np.zeros((nl, N + 1, N + 1)) for n in ACC}
        self.W, self.mask, self.D2, self.psi_bc = 0.0, np.array(mask, dtype=np.float64), D2, psi_bc

    def sample(self, psi, q, w):
        u, v = velocities(psi, self.mask, self.D2)
        x = dict(PSI=psi, Q=q, PSI2=psi * psi, Q2=q * q, KE=0.5 * (u * u + v * v), UQ=u * q, VQ=v * q)
        for n in ACC:
            self.S[n] = self.S[n] + w * x[n]
        self.W = self.W + w

    def get(self, name):
        if name in ACC:
            return self.S[name] / self.W
        pm = self.S["PSI"] / self.W
        pm[:, 0, :] = pm[:, -1, :] = pm[:, :, 0] = pm[:, :, -1] = self.psi_bc      # the handle's boundary rule for psi
        um, vm = velocities(pm, self.mask, self.D2)
        if name == "EKE":
            return self.S["KE"] / self.W - 0.5 * (um * um + vm * vm)
        return self.S[name[:2]] / self.W - (um if name == "UQ_EDDY" else vm) * (self.S["Q"] / self.W)
