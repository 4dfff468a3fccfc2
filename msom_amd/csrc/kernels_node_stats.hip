// kernels_node_stats.hip -- running time means and eddy statistics of the VERTEX-grid model (msomn_stats_*): the
// twin of k_stats_acc / k_stats_mean / k_stats_derive of kernels_rhs.hip on the vertices a handle (or a tile) holds.
//
// What the vertex grid changes: u and v carry the land mask of the vertex, u = ((psi[j-1][i] - psi[j+1][i]) / (2 D)) * mask[j][i],
// v = ((psi[j][i+1] - psi[j][i-1]) / (2 D)) * mask[j][i]; on a vertex of the DOMAIN boundary (global i or j equal to 0 or N) both are
// exactly 0 and the neighbour beyond the wall is not read; on a tile's interior edge the neighbour is the halo.  "Domain boundary" is
// decided from the tile's global offsets, so every holder of a shared vertex takes the same branch on the same operands.
#include "kernels.h"

#ifdef MSOM_STRICT
#define DIVC(x, c, rc) ((x) / (c))
#else
#define DIVC(x, c, rc) ((x) * (rc))
#endif
#define BX 64
#define BY 4
static inline dim3 grid2d(int nx, int ny) { return dim3((nx + BX - 1) / BX, (ny + BY - 1) / BY); }
static inline dim3 block2d() { return dim3(BX, BY); }

// one sample: for every selected accumulator k of every held vertex and layer
//   s_k = s_k + w * x_k,   x = psi, q, psi*psi, q*q, 0.5 * (u*u + v*v), u*q, v*q   (MSOM_ST_PSI .. MSOM_ST_VQ)
// The strict build keeps this expression order with true divisions, the product build multiplies by 1 / (2 D) and may contract.
// Shaped like k_stats_acc: one thread owns two x-adjacent vertices of every layer, 16-byte accesses (rows start 128-byte aligned and
// the pair starts on an even vertex); a held row has an odd number of vertices, so the last one goes alone through the same body with
// its second lane masked off -- the row is not padded.  Instantiated on the mask: what is not selected is neither read nor written;
// psi's neighbour rows and the land mask are loaded only where a selected quantity needs them (PSI | Q reads neither).  Every vertex
// owns its accumulators: no atomics, no reductions, the same bits on every run.
template <int K, unsigned MASK>
__device__ __forceinline__ void nstats_add(const StatsAcc &a, size_t c, bool pair, double w, double x0, double x1) {
  if constexpr ((MASK >> K) & 1u) {
    double *s = a.s[K] + c;
    if (pair) {
      double2 t = *reinterpret_cast<const double2 *>(s);
      t.x = t.x + w * x0;
      t.y = t.y + w * x1;
      *reinterpret_cast<double2 *>(s) = t;
    } else
      s[0] = s[0] + w * x0;
  }
}
template <unsigned MASK>
__global__ void __launch_bounds__(BX *BY) k_n_stats_acc(const double *__restrict__ psi, const double *__restrict__ q, const double *__restrict__ mk,
                                                        StatsAcc a, NatGeom g, int nl, NStatsTile t, double w, double D2, double rD2) {
  constexpr unsigned B_PSI = 1u << MSOM_ST_PSI, B_Q = 1u << MSOM_ST_Q, B_PSI2 = 1u << MSOM_ST_PSI2, B_Q2 = 1u << MSOM_ST_Q2,
                     B_KE = 1u << MSOM_ST_KE, B_UQ = 1u << MSOM_ST_UQ, B_VQ = 1u << MSOM_ST_VQ;
  constexpr bool NU = (MASK & (B_KE | B_UQ)) != 0, NV = (MASK & (B_KE | B_VQ)) != 0;   // which velocity components are needed
  constexpr bool NP = (MASK & (B_PSI | B_PSI2)) != 0 || NV, NQ = (MASK & (B_Q | B_Q2 | B_UQ | B_VQ)) != 0;
  const int i = 2 * (blockIdx.x * BX + threadIdx.x), j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const bool pair = i + 1 < g.nx;   // false: the tail vertex of an odd row, lane y masked
  const int gi = t.ox + i, gj = t.oy + j;
  // vertices with a velocity: not on the domain boundary.  in0 / in1: of the two lanes; the row decides both
  const bool row_in = gj > 0 && gj < t.N, in0 = row_in && gi > 0 && gi < t.N, in1 = row_in && pair && gi + 1 < t.N;
  size_t c = nat_idx(g, 0, j, i);
  double2 m = make_double2(0., 0.);
  if (NU || NV) {
    if (in0) m.x = mk[c];
    if (in1) m.y = mk[c + 1];
  }
  for (int l = 0; l < nl; l++, c += g.ls) {
    double2 p = make_double2(0., 0.), vq = make_double2(0., 0.), u = make_double2(0., 0.), v = make_double2(0., 0.);
    if (NP) { if (pair) p = *reinterpret_cast<const double2 *>(psi + c); else p.x = psi[c]; }
    if (NQ) { if (pair) vq = *reinterpret_cast<const double2 *>(q + c); else vq.x = q[c]; }
    if (NU && row_in) {   // rows j - 1 and j + 1 are held, or the halo of a tile's interior edge
      double2 s = make_double2(0., 0.), n = make_double2(0., 0.);
      if (pair) { s = *reinterpret_cast<const double2 *>(psi + c - g.pitch); n = *reinterpret_cast<const double2 *>(psi + c + g.pitch); }
      else { s.x = psi[c - g.pitch]; n.x = psi[c + g.pitch]; }
      if (in0) u.x = DIVC(s.x - n.x, D2, rD2) * m.x;
      if (in1) u.y = DIVC(s.y - n.y, D2, rD2) * m.y;
    }
    if (NV) {
      // lane x: neighbours i - 1 (a scalar load) and i + 1 (lane y, or a scalar load behind the tail vertex of a tile's row)
      if (in0) v.x = DIVC((pair ? p.y : psi[c + 1]) - psi[c - 1], D2, rD2) * m.x;
      if (in1) v.y = DIVC(psi[c + 2] - p.x, D2, rD2) * m.y;
    }
    nstats_add<MSOM_ST_PSI, MASK>(a, c, pair, w, p.x, p.y);
    nstats_add<MSOM_ST_Q, MASK>(a, c, pair, w, vq.x, vq.y);
    nstats_add<MSOM_ST_PSI2, MASK>(a, c, pair, w, p.x * p.x, p.y * p.y);
    nstats_add<MSOM_ST_Q2, MASK>(a, c, pair, w, vq.x * vq.x, vq.y * vq.y);
    nstats_add<MSOM_ST_KE, MASK>(a, c, pair, w, 0.5 * (u.x * u.x + v.x * v.x), 0.5 * (u.y * u.y + v.y * v.y));
    nstats_add<MSOM_ST_UQ, MASK>(a, c, pair, w, u.x * vq.x, u.y * vq.y);
    nstats_add<MSOM_ST_VQ, MASK>(a, c, pair, w, v.x * vq.x, v.y * vq.y);
  }
}
int launch_n_stats_acc(hipStream_t st, unsigned mask, const double *psi, const double *q, const double *mk, const StatsAcc &a, const NatGeom &g,
                       int nl, const NStatsTile &t, double w, double D2) {
  const dim3 gr(((g.nx + 1) / 2 + BX - 1) / BX, (g.ny + BY - 1) / BY);
  const bool ok = with_int<1, (1 << MSOM_ST_NACC) - 1>((int)mask, [&](auto M) {
    hipLaunchKernelGGL((k_n_stats_acc<(unsigned)decltype(M)::value>), gr, block2d(), 0, st, psi, q, mk, a, g, nl, t, w, D2, 1. / D2);
  });
  return ok ? 0 : -1;
}

// msomn_stats_get: mean = s / W (a true division in both builds) into a natural field, every held vertex
__global__ void __launch_bounds__(BX *BY) k_n_stats_mean(double *__restrict__ out, const double *__restrict__ s, double W, NatGeom g, int nl) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  size_t c = nat_idx(g, 0, j, i);
  for (int l = 0; l < nl; l++, c += g.ls) out[c] = s[c] / W;
}
void launch_n_stats_mean(hipStream_t st, double *out, const double *s, double W, const NatGeom &g, int nl) {
  hipLaunchKernelGGL(k_n_stats_mean, grid2d(g.nx, g.ny), block2d(), 0, st, out, s, W, g, nl);
}
// the derived statistics from pm = the mean psi with the boundary rule of psi on its sides (and, on tiles, its halo exchanged), the
// same masked differences um, vm as the sample, and the accumulators sa (KE, or UQ / VQ) and sq (Q):
//   MSOM_ST_EKE     = sa / W - 0.5 * (um * um + vm * vm)
//   MSOM_ST_UQ_EDDY = sa / W - um * (sq / W),   MSOM_ST_VQ_EDDY = sa / W - vm * (sq / W)
// into a natural field (out is not pm: the differences read pm's neighbours)
__global__ void __launch_bounds__(BX *BY) k_n_stats_derive(double *__restrict__ out, const double *__restrict__ pm, const double *__restrict__ mk,
                                                           const double *__restrict__ sa, const double *__restrict__ sq, double W, NatGeom g, int nl,
                                                           int which, NStatsTile t, double D2, double rD2) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const int gi = t.ox + i, gj = t.oy + j;
  const bool in = gi > 0 && gi < t.N && gj > 0 && gj < t.N;
  size_t c = nat_idx(g, 0, j, i);
  const double m = in ? mk[c] : 0.;
  for (int l = 0; l < nl; l++, c += g.ls) {
    double um = 0., vm = 0.;
    if (in) {
      um = DIVC(pm[c - g.pitch] - pm[c + g.pitch], D2, rD2) * m;
      vm = DIVC(pm[c + 1] - pm[c - 1], D2, rD2) * m;
    }
    const double ma = sa[c] / W;
    if (which == MSOM_ST_EKE) out[c] = ma - 0.5 * (um * um + vm * vm);
    else out[c] = ma - (which == MSOM_ST_UQ_EDDY ? um : vm) * (sq[c] / W);
  }
}
void launch_n_stats_derive(hipStream_t st, double *out, const double *pm, const double *mk, const double *sa, const double *sq, double W,
                           const NatGeom &g, int nl, int which, const NStatsTile &t, double D2) {
  hipLaunchKernelGGL(k_n_stats_derive, grid2d(g.nx, g.ny), block2d(), 0, st, out, pm, mk, sa, sq, W, g, nl, which, t, D2, 1. / D2);
}
