// noise_inl.h -- device arithmetic of the counter-based noise generator, shared by k_noise (kernels_rhs.hip) and
// k_n_noise (kernels_node.hip).  tests/philox_ref.py is its numpy restatement.
#ifndef MSOM_NOISE_INL_H
#define MSOM_NOISE_INL_H

#include "kernels.h"

// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): counter c, key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// N(0, 1) of one cell-layer: counter (cell, layer, draw, "msom"), key (seed, "MI35"), then the reference's Box-Muller formula
// (msqg/qg_stochastic.h:9, qg-node/qg_stochastic.h:13) on two uniforms quantised to rand()'s 31 bits
__device__ __forceinline__ double philox_normal(uint32_t cell, uint32_t layer, uint32_t draw, uint32_t seed) {
  uint32_t c[4] = {cell, layer, draw, 0x6d736f6du};
  philox4x32_10(c, seed, 0x4d493335u);
  const double r1 = (double)(c[0] >> 1), r2 = (double)(c[1] >> 1), RM = 2147483647.;  // RAND_MAX
  const double a = sqrt(-2. * log((r1 + 1.) / (RM + 2.)));
  return a * cos(2 * 3.14159265358979323846 * r2 / RM);
}

#endif
