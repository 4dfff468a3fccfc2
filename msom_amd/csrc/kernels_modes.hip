// kernels_modes.hip -- vertical normal modes of the stretching operator (msom_modes_*), gfx950 / CDNA4, fp64.
//
// Reference: the per-column decomposition of msqg/eigmode.h (eigmod :65-308, compiled out there by MODE_PV_INVERT 0) and the
// layer <-> mode products of msqg/qg.h:117-131,143-157.  Arrays of one decomposition, `ols` doubles apart:
//   0 .. nl*nl - 1   M2L, array k*nl + m = vr[k][m] (layer k from mode m)
//   nl*nl .. + nl-1  iBu_m = -lambda_m, iBu_0 = 0
// either one natural padded layer each (the general form, one eigenproblem per column) or one double each (the compact form of a
// stratification that is the same in every column; the other kernels then get the numbers by value in a ModeCoef).
// L2M[m][k] = dhf[k] * M2L[k][m] (the left vectors of eigmode.h:223-231; htotal = 1) and Rd_m = sqrt(-1 / iBu_m) are formed where
// they are needed and never stored.
//
// Arithmetic: the products are accumulated in the documented order, acc = 0; acc = acc + c * x for the inner index ascending --
// unfused in the strict build, as one explicit chain of fused multiply-adds in the product build, so that the compact and the general
// instantiation of a kernel round alike in both.
#include "kernels.h"

#ifdef MSOM_STRICT
#define DIVC(x, c, rc) ((x) / (c))
#define MADD(c, x, acc) ((acc) + (c) * (x))
#else
#define DIVC(x, c, rc) ((x) * (rc))
#define MADD(c, x, acc) fma((c), (x), (acc))
#endif

#define BX 64
#define BY 4
static inline dim3 grid2d(int nx, int ny) { return dim3((nx + BX - 1) / BX, (ny + BY - 1) / BY); }
static inline dim3 block2d() { return dim3(BX, BY); }

// ------------------------------------------------------------------ the decomposition

// One thread per column of an ncx x ncy grid (the tile, or 1 x 1 for the compact form: cell (0, 0)); 64 threads per workgroup.
// NL <= MSOM_FASTNL: the vector matrix in registers; above: in LDS, element e of lane t at [e * 64 + t] (conflict-free, and a lane
// only ever touches its own slots, so there is no barrier).  Output index: array * ols + (per_column ? cell : 0).
// A column whose S is not positive and finite, whose iteration hits the sweep cap, or whose first baroclinic eigenvalue is below the
// rounding level of the matrix (MODES_WEAK, modes_inl.h) ORs its status into *flag and writes nothing.
template <int NL>
__global__ void __launch_bounds__(64) k_modes_eig(const double *__restrict__ S, NatGeom g, int ncx, int ncy, double *__restrict__ out, size_t ols,
                                                  int per_column, ModesLayers lay, int *flag) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
  if (i >= ncx || j >= ncy) return;
  const size_t c = nat_idx(g, 0, j, i), oc = per_column ? c : 0;
  double s[NL > 1 ? NL - 1 : 1];
#pragma unroll
  for (int l = 0; l < NL - 1; l++) s[l] = S[c + (size_t)l * g.ls];
  double d[NL];
  int rank[NL], st;
  if constexpr (NL <= MSOM_FASTNL) {
    ModesRegV<NL> V;
    st = modes_eig_column<NL>(s, lay, V, d, rank);
    if (st == MODES_OK) {
#pragma unroll
      for (int m = 0; m < NL; m++) {
#pragma unroll
        for (int k = 0; k < NL; k++) out[(size_t)(k * NL + rank[m]) * ols + oc] = V.get(k * NL + m);
      }
    }
  } else {
    __shared__ double lds[(NL * NL + 2 * NL) * 64];   // nl = 16: 144 KB of the 160 KB a workgroup may have
    ModesMemV<NL> V{lds + threadIdx.x, 64};
    st = modes_eig_column<NL>(s, lay, V, d, rank);
    if (st == MODES_OK) {
#pragma unroll
      for (int m = 0; m < NL; m++) {
#pragma unroll
        for (int k = 0; k < NL; k++) out[(size_t)(k * NL + rank[m]) * ols + oc] = V.get(k * NL + m);
      }
    }
  }
  if (st != MODES_OK) { atomicOr(flag, st); return; }
#pragma unroll
  for (int m = 0; m < NL; m++) out[(size_t)(NL * NL + rank[m]) * ols + oc] = rank[m] == 0 ? 0. : -d[m];   // eigmode.h:256-266
}

int launch_modes_eig(hipStream_t st, const double *S, const NatGeom &g, int nl, int ncx, int ncy, double *out, size_t ols, int per_column,
                     const ModesLayers &l, int *flag) {
  const dim3 gr((ncx + 63) / 64, ncy);
  if (!with_int<1, MSOM_MAXNL>(nl, [&](auto N) { hipLaunchKernelGGL(k_modes_eig<N()>, gr, dim3(64), 0, st, S, g, ncx, ncy, out, ols, per_column, l, flag); }))
    return -1;
  return 0;
}

// ------------------------------------------------------------------ coefficient sources of the other kernels

// number e of the decomposition at a cell: e = k * NL + m for M2L, NL * NL + m for iBu
struct CoefColumn {    // general form: one padded layer per number; c = nat_idx of the cell
  const double *md;
  size_t ls;
  __device__ __forceinline__ double at(int e, size_t c) const { return md[e * ls + c]; }
  __device__ __forceinline__ void reread() {}
};
struct CoefCompact {   // compact form: the numbers by value (kernel arguments) ...
  ModeCoef mc;
};
struct CoefLds {       // ... which a workgroup first copies to LDS: every later read is a broadcast, whatever the index
  const double *cs;
  int off;   // 0
  __device__ __forceinline__ double at(int e, size_t) const { return cs[e + off]; }
  // the compiler may no longer assume that `off` is the value it knew: the reads that follow are issued where they stand instead of
  // all nl*nl + nl of them being held in registers across a loop
  __device__ __forceinline__ void reread() { asm volatile("" : "+v"(off)); }
};
template <bool COMPACT> using CoefOf = std::conditional_t<COMPACT, CoefCompact, CoefColumn>;
template <bool COMPACT>
static CoefOf<COMPACT> make_coef(const double *md, const NatGeom &g, const ModeCoef *mc) {
  if constexpr (COMPACT) return CoefCompact{*mc};
  else return CoefColumn{md, g.ls};
}
// called by every thread of the workgroup before any of them leaves
template <int NL>
__device__ __forceinline__ CoefColumn coef_stage(const CoefColumn &cf, double *) { return cf; }
template <int NL>
__device__ __forceinline__ CoefLds coef_stage(const CoefCompact &cf, double *cs) {
  if (threadIdx.x == 0 && threadIdx.y == 0) {   // constant indices into the kernel arguments
#pragma unroll
    for (int e = 0; e < NL * NL; e++) cs[e] = cf.mc.m2l[e];
#pragma unroll
    for (int e = 0; e < NL; e++) cs[NL * NL + e] = cf.mc.ibu[e];
  }
  __syncthreads();
  return CoefLds{cs, 0};
}
#define MODES_COEF(co, cf)                                   \
  __shared__ double cs__[COMPACT ? NL * NL + NL : 1];        \
  auto co = coef_stage<NL>(cf, cs__)

// ------------------------------------------------------------------ msom_modes_get

// `cnt` arrays starting at array `first` of `which`, written contiguously [cnt][ny][nx] (the staging layout)
template <int NL, bool COMPACT>
__global__ void __launch_bounds__(BX *BY) k_modes_get(double *__restrict__ out, CoefOf<COMPACT> cf, NatGeom g, ModesLayers lay, int which, int first,
                                                      int cnt) {
  MODES_COEF(co, cf);
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const size_t c = nat_idx(g, 0, j, i), n = (size_t)g.nx * g.ny;
  size_t o = (size_t)j * g.nx + i;
  for (int a = first; a < first + cnt; a++, o += n) {
    double v;
    if (which == MSOM_MD_IBU) v = co.at(NL * NL + a, c);
    else if (which == MSOM_MD_RD) v = a == 0 ? 0. : sqrt(-1. / co.at(NL * NL + a, c));   // eigmode.h:284
    else if (which == MSOM_MD_M2L) v = co.at(a, c);
    else {                      // array m*nl + k = dhf[k] * M2L[k*nl + m]
      const int m = a / NL, k = a - m * NL;
      double dk = 0.;
#pragma unroll
      for (int p = 0; p < NL; p++)
        if (p == k) dk = lay.dhf[p];
      v = dk * co.at(k * NL + m, c);
    }
    out[o] = v;
  }
}
int launch_modes_get(hipStream_t st, double *out, const double *md, const ModeCoef *mc, const NatGeom &g, int nl, const ModesLayers &l, int which,
                     int first, int cnt) {
  bool ok = false;
  with_bool(mc != nullptr, [&](auto C) {
    ok = with_int<1, MSOM_MAXNL>(nl, [&](auto N) {
      hipLaunchKernelGGL((k_modes_get<N(), C()>), grid2d(g.nx, g.ny), block2d(), 0, st, out, make_coef<C()>(md, g, mc), g, l, which, first, cnt);
    });
  });
  return ok ? 0 : -1;
}
// MSOM_RD = Rd of one mode, interior cells of the natural field (boundary() follows)
template <int NL, bool COMPACT>
__global__ void __launch_bounds__(BX *BY) k_modes_rd(double *__restrict__ rd, CoefOf<COMPACT> cf, NatGeom g, int mode) {
  MODES_COEF(co, cf);
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const size_t c = nat_idx(g, 0, j, i);
  rd[c] = sqrt(-1. / co.at(NL * NL + mode, c));
}
int launch_modes_rd(hipStream_t st, double *rd, const double *md, const ModeCoef *mc, const NatGeom &g, int nl, int mode) {
  bool ok = false;
  with_bool(mc != nullptr, [&](auto C) {
    ok = with_int<1, MSOM_MAXNL>(nl, [&](auto N) {
      hipLaunchKernelGGL((k_modes_rd<N(), C()>), grid2d(g.nx, g.ny), block2d(), 0, st, rd, make_coef<C()>(md, g, mc), g, mode);
    });
  });
  return ok ? 0 : -1;
}

// ------------------------------------------------------------------ msom_modes_project

// in / out: contiguous [nl][ny][nx] (caller's device arrays or the staging buffer), in == out allowed: a thread owns its column
// and loads it before it stores.  Streams 2 nl layers (+ nl^2 coefficient layers in the general form).
template <int NL, bool COMPACT>
__global__ void __launch_bounds__(BX *BY) k_modes_project(const double *in, double *out, CoefOf<COMPACT> cf, NatGeom g, ModesLayers lay, int to_modes) {
  MODES_COEF(co, cf);
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const size_t c = nat_idx(g, 0, j, i), n = (size_t)g.nx * g.ny, o = (size_t)j * g.nx + i;
  double x[NL], y[NL];
#pragma unroll
  for (int k = 0; k < NL; k++) x[k] = in[o + (size_t)k * n];
  if (to_modes) {
#pragma unroll
    for (int m = 0; m < NL; m++) {
      double acc = 0.;
#pragma unroll
      for (int k = 0; k < NL; k++) acc = MADD(lay.dhf[k] * co.at(k * NL + m, c), x[k], acc);
      y[m] = acc;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NL; k++) {
      double acc = 0.;
#pragma unroll
      for (int m = 0; m < NL; m++) acc = MADD(co.at(k * NL + m, c), x[m], acc);
      y[k] = acc;
    }
  }
#pragma unroll
  for (int k = 0; k < NL; k++) out[o + (size_t)k * n] = y[k];
}
int launch_modes_project(hipStream_t st, const double *in, double *out, const double *md, const ModeCoef *mc, const NatGeom &g, int nl,
                         const ModesLayers &l, int to_modes) {
  bool ok = false;
  with_bool(mc != nullptr, [&](auto C) {
    ok = with_int<1, MSOM_MAXNL>(nl, [&](auto N) {
      hipLaunchKernelGGL((k_modes_project<N(), C()>), grid2d(g.nx, g.ny), block2d(), 0, st, in, out, make_coef<C()>(md, g, mc), g, l, to_modes);
    });
  });
  return ok ? 0 : -1;
}

// ------------------------------------------------------------------ msom_modes_energy

// ke[m] = sum 0.5 (u_m^2 + v_m^2) Delta^2, pe[m] = sum 0.5 (-iBu_m) psi_m^2 Delta^2 with u, v of the msom_stats_* block and
// x_m = sum_k l2m[m][k] x_k, in one pass over psi (ghost values included).  A thread marches MODES_EROWS rows of one x with the psi rows
// j - 1, j, j + 1 of every layer in registers; a workgroup of 64 x 4 threads covers 4 * MODES_EROWS rows and leaves one partial sum per
// quantity: partial[q * stride + block], q = m (ke) and NL + m (pe).  The second stage is launch_sum_final's.
#define MODES_EROWS 8
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
template <int NL, bool COMPACT>
__global__ void __launch_bounds__(BX *BY) k_modes_energy(const double *__restrict__ psi, CoefOf<COMPACT> cf, NatGeom g, ModesLayers lay, double *partial,
                                                         int stride, double D2, double rD2, double sqD) {
  MODES_COEF(co, cf);
  const int i = blockIdx.x * BX + threadIdx.x, j0 = (blockIdx.y * BY + threadIdx.y) * MODES_EROWS;
  double ke[NL], pe[NL];
#pragma unroll
  for (int m = 0; m < NL; m++) ke[m] = pe[m] = 0.;
  if (i < g.nx && j0 < g.ny) {
    double pm[NL], pc[NL], pp[NL];   // rows j - 1, j, j + 1
    size_t c = nat_idx(g, 0, j0, i);
#pragma unroll
    for (int k = 0; k < NL; k++) {
      pm[k] = psi[c + (size_t)k * g.ls - g.pitch];
      pc[k] = psi[c + (size_t)k * g.ls];
    }
    const int j1 = min(j0 + MODES_EROWS, g.ny);
    for (int j = j0; j < j1; j++, c += g.pitch) {
      co.reread();
      double u[NL], v[NL];
#pragma unroll
      for (int k = 0; k < NL; k++) {
        const size_t ck = c + (size_t)k * g.ls;
        pp[k] = psi[ck + g.pitch];
        u[k] = DIVC(pm[k] - pp[k], D2, rD2);
        v[k] = DIVC(psi[ck + 1] - psi[ck - 1], D2, rD2);
      }
#pragma unroll
      for (int m = 0; m < NL; m++) {
        double um = 0., vm = 0., qm = 0.;
#pragma unroll
        for (int k = 0; k < NL; k++) {
          const double l2m = lay.dhf[k] * co.at(k * NL + m, c);
          um = MADD(l2m, u[k], um);
          vm = MADD(l2m, v[k], vm);
          qm = MADD(l2m, pc[k], qm);
        }
        ke[m] += 0.5 * (um * um + vm * vm) * sqD;
        pe[m] += 0.5 * (-co.at(NL * NL + m, c)) * (qm * qm) * sqD;
      }
#pragma unroll
      for (int k = 0; k < NL; k++) { pm[k] = pc[k]; pc[k] = pp[k]; }
    }
  }
  __shared__ double sm[2 * NL][BY];
#pragma unroll
  for (int m = 0; m < NL; m++) {
    const double a = wave_sum(ke[m]), b = wave_sum(pe[m]);
    if (threadIdx.x == 0) { sm[m][threadIdx.y] = a; sm[NL + m][threadIdx.y] = b; }
  }
  __syncthreads();
  const int t = threadIdx.y * BX + threadIdx.x;
  if (t < 2 * NL) {
    double s = 0.;
    for (int k = 0; k < BY; k++) s += sm[t][k];
    partial[(size_t)t * stride + blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}
static dim3 energy_grid(const NatGeom &g) { return dim3((g.nx + BX - 1) / BX, (g.ny + BY * MODES_EROWS - 1) / (BY * MODES_EROWS)); }
int modes_energy_blocks(const NatGeom &g) {
  const dim3 gr = energy_grid(g);
  return gr.x * gr.y;
}
int modes_energy_stride(const NatGeom &g) { return modes_energy_blocks(g) + 64; }   // room for the chunk sums of launch_sum_final
int launch_modes_energy(hipStream_t st, const double *psi, const double *md, const ModeCoef *mc, const NatGeom &g, int nl, const ModesLayers &l,
                        double *partial, double *out, double D) {
  const int nb = modes_energy_blocks(g), stride = modes_energy_stride(g);
  bool ok = false;
  with_bool(mc != nullptr, [&](auto C) {
    ok = with_int<1, MSOM_MAXNL>(nl, [&](auto N) {
      hipLaunchKernelGGL((k_modes_energy<N(), C()>), energy_grid(g), block2d(), 0, st, psi, make_coef<C()>(md, g, mc), g, l, partial, stride, 2. * D,
                         1. / (2. * D), D * D);
    });
  });
  if (!ok) return -1;
  for (int q = 0; q < 2 * nl; q++) launch_sum_final(st, partial + (size_t)q * stride, out + q, nb);
  return 0;
}
