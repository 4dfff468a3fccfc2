// kernels_node_floats.hip -- Lagrangian floats of the vertex-grid model (msomn_floats_*): one float per lane,
// structure of arrays.  The arithmetic is the vertex part of floats_inl.h, shared with the host check; a kernel adds the four gathers
// of the cell's corner vertices from the natural layout of the level-0 fields (vertex indices lie in [0, N] by construction, whatever
// the position's bits: no ghost and no pad column is read) and the stores.  The floats are not sorted; the gathers are left to L2.
// On tiles the same per-float bodies run over the slots of a rank (the *_tiled kernels, "On tiles" in section 8l); the floats move
// between the tiles with the kernels of kernels_floats.hip.
#include <hip/hip_runtime.h>

#include "kernels.h"

#define FL_THREADS 256

// the four corners P00, P10, P01, P11 of the grid cell c in layer l; PG: psi + psipg summed per corner
template <bool PG>
__device__ __forceinline__ void nfl_corners(const double *__restrict__ f, const double *__restrict__ pg, const NatGeom &g, int l, const FloatsCell &c,
                                            double P[4]) {
  const size_t o = nat_idx(g, l, c.j0, c.i0);
  P[0] = f[o];
  P[1] = f[o + 1];
  P[2] = f[o + g.pitch];
  P[3] = f[o + g.pitch + 1];
  if constexpr (PG) {
    P[0] = P[0] + pg[o];
    P[1] = P[1] + pg[o + 1];
    P[2] = P[2] + pg[o + g.pitch];
    P[3] = P[3] + pg[o + g.pitch + 1];
  }
}

// STAGE 1: (xh, yh) = (x, y) + dt / 2 U(x, y); STAGE 2: (x, y) += dt U(xh, yh).  A float whose position is not finite reads nothing
// and stays NaN; it is counted when it becomes so, that is once.  REC (stage 2): 0 no record, 1 the new position into rec [2][n],
// 2 also the bilinear value of rf at the new position, in the float's layer, into rec [3][n] (NaN for a lost float).  One float: slot
// k, record entry rk of n.  TILED: fg is the global geometry, (tx0, ty0) the tile's vertex origin, taken off the located indices: the
// corners are vertices the tile holds (floats_inl.h), and a float whose corners are not reads nothing and becomes NaN; the record is
// [3][n] by id, x, y and a presence word (REC 2 has no tiled form: the new position may be another tile's).  One tile: rk = k
template <bool PG, int STAGE, int REC, bool TILED>
__device__ __forceinline__ void nfl_stage_one(const FloatsDev &d, int k, size_t rk, size_t n, const double *__restrict__ psi, const double *__restrict__ pg,
                                              const NatGeom &g, const FloatsGeom &fg, double dt, double *__restrict__ rec, const double *__restrict__ rf,
                                              int tx0, int ty0) {
  static_assert(!(TILED && REC == 2), "the recorded field is sampled behind the migration pass");
  const double bx = d.x[k], by = d.y[k];
  const double px = STAGE == 1 ? bx : d.xh[k], py = STAGE == 1 ? by : d.yh[k];
  FloatsCell c = nfloats_locate(px, py, fg);
  if constexpr (TILED) {
    if (!nfloats_local(&c, tx0, ty0, g.nx - 1, g.ny - 1)) c.ok = 0;
  }
  const int l = d.layer[k];
  double ox = NAN, oy = NAN;
  int flag = 0;
  if (c.ok) {
    double P[4], u, v;
    nfl_corners<PG>(psi, pg, g, l, c, P);
    floats_uv(P[0], P[1], P[2], P[3], c.a, c.b, fg.idx, &u, &v);
    flag = floats_move(bx, by, u, v, STAGE == 1 ? dt / 2. : dt, fg, &ox, &oy);
    if (!floats_finite(bx) || !floats_finite(by)) flag = 0;   // lost before this stage
  } else if (floats_finite(bx) && floats_finite(by) && floats_finite(px) && floats_finite(py))
    flag = 2;   // a finite position whose cell coordinate overflows
  if constexpr (STAGE == 1) {
    d.xh[k] = ox;
    d.yh[k] = oy;
  } else {
    d.x[k] = ox;
    d.y[k] = oy;
    if constexpr (REC >= 1) {
      rec[rk] = ox;
      rec[n + rk] = oy;
      if constexpr (TILED) rec[2 * n + rk] = 1.;
    }
    if constexpr (REC == 2) {
      double s = NAN;
      const FloatsCell e = nfloats_locate(ox, oy, fg);
      if (e.ok) {
        double Q[4];
        nfl_corners<false>(rf, nullptr, g, l, e, Q);
        s = floats_bilinear(Q[0], Q[1], Q[2], Q[3], e.a, e.b);
      }
      rec[2 * n + rk] = s;
    }
  }
  if (flag & 1) atomicAdd(&d.cnt[0], 1ull);
  if (flag & 2) atomicAdd(&d.cnt[1], 1ull);
}

template <bool PG, int STAGE, int REC>
__global__ void __launch_bounds__(FL_THREADS) k_nfloats_stage(FloatsDev d, int n, const double *__restrict__ psi, const double *__restrict__ pg, NatGeom g,
                                                              FloatsGeom fg, double dt, double *__restrict__ rec, const double *__restrict__ rf) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n) return;
  nfl_stage_one<PG, STAGE, REC, false>(d, k, (size_t)k, (size_t)n, psi, pg, g, fg, dt, rec, rf, 0, 0);
}
// on tiles: over the n slots; lanes beyond the high-water mark and empty slots leave
template <bool PG, int STAGE, int REC>
__global__ void __launch_bounds__(FL_THREADS) k_nfloats_stage_tiled(FloatsDev d, FloatsTileDev t, int n, const double *__restrict__ psi,
                                                                    const double *__restrict__ pg, NatGeom g, FloatsGeom fg, double dt, double *__restrict__ rec) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n || k >= *t.hw || !t.live[k]) return;
  const int id = t.id[k];
  if ((unsigned)id >= (unsigned)n) return;
  nfl_stage_one<PG, STAGE, REC, true>(d, k, (size_t)id, (size_t)n, psi, pg, g, fg, dt, rec, nullptr, t.ox, t.oy);
}

// VEL: r0 = u, r1 = v at (x, y); else r0 = the bilinear value of f there.  A lost float gives NaN, and on tiles a float that is not
// at home
template <bool PG, bool VEL, bool TILED>
__device__ __forceinline__ void nfl_interp_one(const FloatsDev &d, int k, const double *__restrict__ f, const double *__restrict__ pg, const NatGeom &g,
                                               const FloatsGeom &fg, int tx0, int ty0, double *r0, double *r1) {
  FloatsCell c = nfloats_locate(d.x[k], d.y[k], fg);
  if constexpr (TILED) {
    if (!nfloats_local(&c, tx0, ty0, g.nx - 1, g.ny - 1)) c.ok = 0;
  }
  *r0 = *r1 = NAN;
  if (c.ok) {
    double P[4];
    nfl_corners<PG>(f, pg, g, d.layer[k], c, P);
    if constexpr (VEL) floats_uv(P[0], P[1], P[2], P[3], c.a, c.b, fg.idx, r0, r1);
    else *r0 = floats_bilinear(P[0], P[1], P[2], P[3], c.a, c.b);
  }
}
template <bool PG, bool VEL>
__global__ void __launch_bounds__(FL_THREADS) k_nfloats_interp(FloatsDev d, int n, const double *__restrict__ f, const double *__restrict__ pg, NatGeom g,
                                                               FloatsGeom fg, double *__restrict__ o0, double *__restrict__ o1) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n) return;
  double r0, r1;
  nfl_interp_one<PG, VEL, false>(d, k, f, pg, g, fg, 0, 0, &r0, &r1);
  o0[k] = r0;
  if constexpr (VEL) o1[k] = r1;
}
// on tiles: the results go to the id-indexed arrays out[0 .. n), out[n .. 2n) with the presence word out[2n + id] = 1
template <bool PG, bool VEL>
__global__ void __launch_bounds__(FL_THREADS) k_nfloats_interp_tiled(FloatsDev d, FloatsTileDev t, int n, const double *__restrict__ f,
                                                                     const double *__restrict__ pg, NatGeom g, FloatsGeom fg, double *__restrict__ out) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n || k >= *t.hw || !t.live[k]) return;
  const int id = t.id[k];
  if ((unsigned)id >= (unsigned)n) return;
  double r0, r1;
  nfl_interp_one<PG, VEL, true>(d, k, f, pg, g, fg, t.ox, t.oy, &r0, &r1);
  out[id] = r0;
  if constexpr (VEL) out[(size_t)n + id] = r1;
  out[2 * (size_t)n + id] = 1.;
}

// *out += `land` over the lanes of the launch.  One atomic per wavefront that has any: an island holds thousands of floats, and they
// would all queue on the one word
__device__ __forceinline__ void nfl_count(bool land, unsigned long long *__restrict__ out) {
  const unsigned long long b = __ballot(land);
  if (land && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(out, (unsigned long long)__popcll(b));
}
// the float of slot k is not lost and its current cell has mask == 0 at all four corners (mk: one layer)
template <bool TILED>
__device__ __forceinline__ bool nfl_land_one(const FloatsDev &d, int k, const double *__restrict__ mk, const NatGeom &g, const FloatsGeom &fg, int tx0, int ty0) {
  FloatsCell c = nfloats_locate(d.x[k], d.y[k], fg);
  if constexpr (TILED) {
    if (!nfloats_local(&c, tx0, ty0, g.nx - 1, g.ny - 1)) c.ok = 0;
  }
  if (!c.ok) return false;
  double M[4];
  nfl_corners<false>(mk, nullptr, g, 0, c, M);
  return M[0] == 0. && M[1] == 0. && M[2] == 0. && M[3] == 0.;
}
// *out += the floats on land
__global__ void __launch_bounds__(FL_THREADS) k_nfloats_on_land(FloatsDev d, int n, const double *__restrict__ mk, NatGeom g, FloatsGeom fg,
                                                                unsigned long long *__restrict__ out) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  nfl_count(k < n && nfl_land_one<false>(d, k, mk, g, fg, 0, 0), out);
}
// on tiles: over the live slots of the rank; the caller sums over the ranks
__global__ void __launch_bounds__(FL_THREADS) k_nfloats_on_land_tiled(FloatsDev d, FloatsTileDev t, int n, const double *__restrict__ mk, NatGeom g,
                                                                      FloatsGeom fg, unsigned long long *__restrict__ out) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  nfl_count(k < n && k < *t.hw && t.live[k] && nfl_land_one<true>(d, k, mk, g, fg, t.ox, t.oy), out);
}

void launch_nfloats_stage(hipStream_t st, int stage, const FloatsDev &d, int n, const double *psi, const double *pg, const NatGeom &g,
                          const FloatsGeom &fg, double dt, double *rec, const double *rf, const FloatsTileDev *t) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS), bl(FL_THREADS);
  with_bool(pg != nullptr, [&](auto PG) {
    if (t) {   // rec: [3][n] by id; the recorded field is the caller's business
      if (stage == 1) hipLaunchKernelGGL((k_nfloats_stage_tiled<PG.value, 1, 0>), gr, bl, 0, st, d, *t, n, psi, pg, g, fg, dt, rec);
      else if (!rec) hipLaunchKernelGGL((k_nfloats_stage_tiled<PG.value, 2, 0>), gr, bl, 0, st, d, *t, n, psi, pg, g, fg, dt, rec);
      else hipLaunchKernelGGL((k_nfloats_stage_tiled<PG.value, 2, 1>), gr, bl, 0, st, d, *t, n, psi, pg, g, fg, dt, rec);
    } else if (stage == 1) hipLaunchKernelGGL((k_nfloats_stage<PG.value, 1, 0>), gr, bl, 0, st, d, n, psi, pg, g, fg, dt, rec, rf);
    else if (!rec) hipLaunchKernelGGL((k_nfloats_stage<PG.value, 2, 0>), gr, bl, 0, st, d, n, psi, pg, g, fg, dt, rec, rf);
    else if (!rf) hipLaunchKernelGGL((k_nfloats_stage<PG.value, 2, 1>), gr, bl, 0, st, d, n, psi, pg, g, fg, dt, rec, rf);
    else hipLaunchKernelGGL((k_nfloats_stage<PG.value, 2, 2>), gr, bl, 0, st, d, n, psi, pg, g, fg, dt, rec, rf);
  });
}

void launch_nfloats_interp(hipStream_t st, const FloatsDev &d, int n, const double *f, const double *pg, const NatGeom &g, const FloatsGeom &fg,
                           double *o0, double *o1, const FloatsTileDev *t) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS), bl(FL_THREADS);
  with_bool(pg != nullptr, [&](auto PG) {
    if (t) {   // o0 is the id-indexed [3][n] array; o1 only says which of the two kernels
      if (o1) hipLaunchKernelGGL((k_nfloats_interp_tiled<PG.value, true>), gr, bl, 0, st, d, *t, n, f, pg, g, fg, o0);
      else hipLaunchKernelGGL((k_nfloats_interp_tiled<PG.value, false>), gr, bl, 0, st, d, *t, n, f, pg, g, fg, o0);
    } else if (o1) hipLaunchKernelGGL((k_nfloats_interp<PG.value, true>), gr, bl, 0, st, d, n, f, pg, g, fg, o0, o1);
    else hipLaunchKernelGGL((k_nfloats_interp<PG.value, false>), gr, bl, 0, st, d, n, f, pg, g, fg, o0, o1);
  });
}

void launch_nfloats_on_land(hipStream_t st, const FloatsDev &d, int n, const double *mk, const NatGeom &g, const FloatsGeom &fg,
                            unsigned long long *out, const FloatsTileDev *t) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS), bl(FL_THREADS);
  if (t) hipLaunchKernelGGL(k_nfloats_on_land_tiled, gr, bl, 0, st, d, *t, n, mk, g, fg, out);
  else hipLaunchKernelGGL(k_nfloats_on_land, gr, bl, 0, st, d, n, mk, g, fg, out);
}
