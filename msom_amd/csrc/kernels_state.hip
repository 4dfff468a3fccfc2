// kernels_state.hip -- the device side of the state file (msom_state.hip): one pass over rows of a natural field that packs them into
// a contiguous staging chunk (save), unpacks such a chunk into the natural layout (load), or only reads the natural layout, and sums
// the record digest of what it touched
//   D = sum_k mix64(bits(x_k) + 0x9E3779B97F4A7C15 (k + 1))  mod 2^64,   k the element's C-order index in the record of the GLOBAL grid.
// The sum is a modular integer sum: any order, any block schedule and any tiling give the same number, so it ends in one 64-bit
// integer atomic per block (per wave by shuffles, per block through LDS) and is still reproducible.
#include <hip/hip_runtime.h>

#include "kernels.h"

enum { ST_PACK = 0, ST_UNPACK = 1, ST_DIGEST = 2 };
#define ST_THREADS 256

__device__ __forceinline__ unsigned long long st_mix64(unsigned long long z) {
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ULL;
  z ^= z >> 27; z *= 0x94d049bb133111ebULL;
  z ^= z >> 31;
  return z;
}

// Elements e = 0 .. rows * tw - 1 of the chunk: record row yy = y0 + e / tw, tile column xi = e % tw (both count the ring where the
// record has one).  Every (yy, xi) lies inside this tile's array: the host clips y0 .. y0 + rows to the tile.
template <int MODE>
__global__ __launch_bounds__(ST_THREADS) void k_state_rows(double *nat, double *stage, StateChunk c, unsigned long long *digest) {
  const int tw = c.g.nx + 2 * c.ring;
  const long long n = (long long)c.rows * tw;
  unsigned long long d = 0;
  for (long long e = (long long)blockIdx.x * ST_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * ST_THREADS) {
    const int ry = (int)(e / tw), xi = (int)(e - (long long)ry * tw);
    const int yy = c.y0 + ry;
    const size_t ni = nat_idx(c.g, c.layer, yy - c.ring - c.oy, xi - c.ring);
    const size_t si = (size_t)ry * c.sw + (size_t)(c.ox + xi - c.sx0);
    double v;
    if (MODE == ST_UNPACK) {
      v = stage[si];
      nat[ni] = v;
    } else {
      v = nat[ni];
      if (MODE == ST_PACK) stage[si] = v;
      const unsigned long long k = ((unsigned long long)c.layer * c.gH + yy) * c.gW + (unsigned long long)(c.ox + xi);
      d += st_mix64((unsigned long long)__double_as_longlong(v) + 0x9E3779B97F4A7C15ULL * (k + 1));
    }
  }
  if (MODE == ST_UNPACK) return;
  for (int o = warpSize / 2; o > 0; o >>= 1) d += (unsigned long long)__shfl_down((long long)d, o);
  __shared__ unsigned long long part[ST_THREADS / 32];
  const int lane = threadIdx.x % warpSize, w = threadIdx.x / warpSize;
  if (lane == 0) part[w] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int k = 0; k < ST_THREADS / warpSize; k++) s += part[k];
    atomicAdd(digest, s);
  }
}

static int st_blocks(const StateChunk &c) {
  const long long n = (long long)c.rows * (c.g.nx + 2 * c.ring);
  long long b = (n + ST_THREADS - 1) / ST_THREADS;
  const long long cap = 8LL * device_cu_count();
  if (b > cap) b = cap;
  return b < 1 ? 1 : (int)b;
}
void launch_state_pack(hipStream_t st, const double *nat, double *stage, const StateChunk &c, unsigned long long *digest) {
  if (c.rows < 1) return;
  hipLaunchKernelGGL(k_state_rows<ST_PACK>, dim3(st_blocks(c)), dim3(ST_THREADS), 0, st, const_cast<double *>(nat), stage, c, digest);
}
void launch_state_unpack(hipStream_t st, const double *stage, double *nat, const StateChunk &c) {
  if (c.rows < 1) return;
  hipLaunchKernelGGL(k_state_rows<ST_UNPACK>, dim3(st_blocks(c)), dim3(ST_THREADS), 0, st, nat, const_cast<double *>(stage), c, nullptr);
}
void launch_state_digest(hipStream_t st, const double *nat, const StateChunk &c, unsigned long long *digest) {
  if (c.rows < 1) return;
  hipLaunchKernelGGL(k_state_rows<ST_DIGEST>, dim3(st_blocks(c)), dim3(ST_THREADS), 0, st, const_cast<double *>(nat), nullptr, c, digest);
}

// test aid of msom_state_dbg_flip: the lowest mantissa bit of one element
__global__ void k_state_flip(double *nat, size_t idx) {
  if (blockIdx.x == 0 && threadIdx.x == 0) nat[idx] = __longlong_as_double(__double_as_longlong(nat[idx]) ^ 1LL);
}
void launch_state_flip(hipStream_t st, double *nat, size_t idx) { hipLaunchKernelGGL(k_state_flip, dim3(1), dim3(64), 0, st, nat, idx); }
