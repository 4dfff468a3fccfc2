// kernels_floats.hip -- Lagrangian floats (msom_floats_*): one float per lane, structure of arrays.  The
// arithmetic is floats_inl.h, shared with the host check; a kernel adds the four gathers of the dual cell's corners from the natural
// layout (ghost ring included: corner indices lie in [-1, n] by construction, whatever the position's bits) and the stores.  The
// floats are not sorted: neighbours in space stay neighbours for many steps and the gathers are left to L2.  On tiles the same per-float
// bodies run over the slots of a rank (the *_tiled kernels), and k_floats_emigrate / k_floats_immigrate move floats between the tiles.
#include <hip/hip_runtime.h>

#include "kernels.h"

#define FL_THREADS 256

// the four corners P00, P10, P01, P11 of the dual cell c in layer l; PG: psi + psipg summed per corner
template <bool PG>
__device__ __forceinline__ void fl_corners(const double *__restrict__ f, const double *__restrict__ pg, const NatGeom &g, int l, const FloatsCell &c,
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

// STAGE 1: (xh, yh) = (x, y) + dt / 2 U(x, y); STAGE 2: (x, y) += dt U(xh, yh), and the record slot when one is due.  A float whose
// position is not finite reads nothing and stays NaN; it is counted when it becomes so, that is once.  One float: slot k, record
// entry rk of n.  TILED: fg is the global geometry, (tx0, ty0) the tile's origin, taken off the located indices: the corners are the
// tile's own cells or its ghost ring (floats_inl.h); the record carries a presence word per id.  One rank: tx0 = ty0 = 0, rk = k
template <bool PG, bool PERIODIC, int STAGE, bool TILED>
__device__ __forceinline__ void fl_stage_one(const FloatsDev &d, int k, size_t rk, size_t n, const double *__restrict__ psi, const double *__restrict__ pg,
                                             const NatGeom &g, const FloatsGeom &fg, double dt, double *__restrict__ rec, int tx0, int ty0) {
  const double bx = d.x[k], by = d.y[k];
  const double px = STAGE == 1 ? bx : d.xh[k], py = STAGE == 1 ? by : d.yh[k];
  FloatsCell c = floats_locate(px, py, fg);
  if constexpr (TILED) {   // the owner's corners lie in its ghost ring by the owner rule; a float that is not at home is not read
    c.i0 -= tx0;
    c.j0 -= ty0;
    if (c.i0 < -1 || c.i0 > g.nx - 1 || c.j0 < -1 || c.j0 > g.ny - 1) c.ok = 0;
  }
  double ox = NAN, oy = NAN;
  int flag = 0;
  if (c.ok) {
    double P[4], u, v;
    fl_corners<PG>(psi, pg, g, d.layer[k], c, P);
    floats_uv(P[0], P[1], P[2], P[3], c.a, c.b, fg.idx, &u, &v);
    flag = floats_move(bx, by, u, v, STAGE == 1 ? dt / 2. : dt, fg, &ox, &oy);
    if (!floats_finite(bx) || !floats_finite(by)) flag = 0;   // lost before this stage
  } else if (floats_finite(bx) && floats_finite(by) && floats_finite(px) && floats_finite(py))
    flag = 2;   // a finite position whose cell coordinate overflows
  if (STAGE == 1) {
    d.xh[k] = ox;
    d.yh[k] = oy;
  } else {
    d.x[k] = ox;
    d.y[k] = oy;
    if (rec) {
      rec[rk] = ox;
      rec[n + rk] = oy;
      if constexpr (TILED) rec[2 * n + rk] = 1.;
    }
  }
  if (flag & 1) atomicAdd(&d.cnt[0], 1ull);
  if (flag & 2) atomicAdd(&d.cnt[1], 1ull);
}

template <bool PG, bool PERIODIC, int STAGE>
__global__ void __launch_bounds__(FL_THREADS) k_floats_stage(FloatsDev d, int n, const double *__restrict__ psi, const double *__restrict__ pg, NatGeom g,
                                                             FloatsGeom fg, double dt, double *__restrict__ rec) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n) return;
  fg.periodic = PERIODIC;
  fl_stage_one<PG, PERIODIC, STAGE, false>(d, k, (size_t)k, (size_t)n, psi, pg, g, fg, dt, rec, 0, 0);
}
// on tiles: over the n slots; lanes beyond the high-water mark and empty slots leave
template <bool PG, bool PERIODIC, int STAGE>
__global__ void __launch_bounds__(FL_THREADS) k_floats_stage_tiled(FloatsDev d, FloatsTileDev t, int n, const double *__restrict__ psi,
                                                                   const double *__restrict__ pg, NatGeom g, FloatsGeom fg, double dt, double *__restrict__ rec) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n || k >= *t.hw || !t.live[k]) return;
  const int id = t.id[k];
  if ((unsigned)id >= (unsigned)n) return;
  fg.periodic = PERIODIC;
  fl_stage_one<PG, PERIODIC, STAGE, true>(d, k, (size_t)id, (size_t)n, psi, pg, g, fg, dt, rec, t.ox, t.oy);
}

// VEL: r0 = u, r1 = v at (x, y); else r0 = the bilinear value of f there
template <bool PG, bool PERIODIC, bool VEL, bool TILED>
__device__ __forceinline__ void fl_interp_one(const FloatsDev &d, int k, const double *__restrict__ f, const double *__restrict__ pg, const NatGeom &g,
                                              const FloatsGeom &fg, int tx0, int ty0, double *r0, double *r1) {
  FloatsCell c = floats_locate(d.x[k], d.y[k], fg);
  if constexpr (TILED) {   // the owner's corners lie in its ghost ring by the owner rule; a float that is not at home is not read
    c.i0 -= tx0;
    c.j0 -= ty0;
    if (c.i0 < -1 || c.i0 > g.nx - 1 || c.j0 < -1 || c.j0 > g.ny - 1) c.ok = 0;
  }
  *r0 = *r1 = NAN;
  if (c.ok) {
    double P[4];
    fl_corners<PG>(f, pg, g, d.layer[k], c, P);
    if constexpr (VEL) floats_uv(P[0], P[1], P[2], P[3], c.a, c.b, fg.idx, r0, r1);
    else *r0 = floats_bilinear(P[0], P[1], P[2], P[3], c.a, c.b);
  }
}
template <bool PG, bool PERIODIC, bool VEL>
__global__ void __launch_bounds__(FL_THREADS) k_floats_interp(FloatsDev d, int n, const double *__restrict__ f, const double *__restrict__ pg, NatGeom g,
                                                              FloatsGeom fg, double *__restrict__ o0, double *__restrict__ o1) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n) return;
  fg.periodic = PERIODIC;
  double r0, r1;
  fl_interp_one<PG, PERIODIC, VEL, false>(d, k, f, pg, g, fg, 0, 0, &r0, &r1);
  o0[k] = r0;
  if constexpr (VEL) o1[k] = r1;
}
// on tiles: the results go to the id-indexed arrays out[0 .. n), out[n .. 2n) with the presence word out[2n + id] = 1
template <bool PG, bool PERIODIC, bool VEL>
__global__ void __launch_bounds__(FL_THREADS) k_floats_interp_tiled(FloatsDev d, FloatsTileDev t, int n, const double *__restrict__ f,
                                                                    const double *__restrict__ pg, NatGeom g, FloatsGeom fg, double *__restrict__ out) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n || k >= *t.hw || !t.live[k]) return;
  const int id = t.id[k];
  if ((unsigned)id >= (unsigned)n) return;
  fg.periodic = PERIODIC;
  double r0, r1;
  fl_interp_one<PG, PERIODIC, VEL, true>(d, k, f, pg, g, fg, t.ox, t.oy, &r0, &r1);
  out[id] = r0;
  if constexpr (VEL) out[(size_t)n + id] = r1;
  out[2 * (size_t)n + id] = 1.;
}

// ---- migration between tiles ("On tiles"): one pass of two phases behind every stage, x then y.
// k_floats_emigrate, phase x (YPH = 0) or y: every live slot finds the tile that owns the position its next stage evaluates -- (xh, yh)
// after stage 1 (half), else (x, y) -- and, when that is a neighbour along the phase's axis, takes a record of the message of its
// direction (lo: W / S, hi: E / N) with one atomicAdd, clears its live flag and pushes its slot on the free stack.  A float that finds
// the message full, or whose owner is farther than a neighbour, is made lost here: NaN, resident, counted in cnt[2].  A float that is
// lost already (a position that cannot be located) stays where it is.  NODE: the vertex grid (msomn_floats_*, section 8l): its cell and
// its owner rule, walls on every side
__device__ __forceinline__ void fl_make_lost(const FloatsMig &s, int k) {
  s.x[k] = s.y[k] = s.xh[k] = s.yh[k] = NAN;
  atomicAdd(&s.cnt[2], 1ull);
}
template <bool YPH, bool NODE>
__global__ void __launch_bounds__(FL_THREADS) k_floats_emigrate(FloatsMig s, int n, FloatsGeom fg, FloatsTiling t, int half, double *__restrict__ mlo,
                                                                double *__restrict__ mhi, int K) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n || k >= *s.hw || !s.live[k]) return;
  const double hx = half ? s.xh[k] : s.x[k], hy = half ? s.yh[k] : s.y[k];
  const FloatsCell c = NODE ? nfloats_locate(hx, hy, fg) : floats_locate(hx, hy, fg);
  if (!c.ok) return;
  int col, row;
  if constexpr (NODE) nfloats_owner(c, t, &col, &row);
  else floats_owner(c, t, &col, &row);
  const int per = NODE ? 0 : fg.periodic;
  const int hop = YPH ? floats_hop(row, t.iy, t.py, per) : floats_hop(col, t.ix, t.px, per);
  if (hop == 0) return;
  double *msg = hop == 1 ? mhi : hop == -1 ? mlo : nullptr;
  const int r = msg ? atomicAdd(&s.msgcnt[hop == 1], 1) : K;
  if (r >= K) {
    fl_make_lost(s, k);
    return;
  }
  double *rec = msg + 1 + 6 * (size_t)r;
  rec[0] = (double)s.id[k];
  rec[1] = s.x[k];
  rec[2] = s.y[k];
  rec[3] = s.xh[k];
  rec[4] = s.yh[k];
  rec[5] = (double)s.layer[k];
  s.live[k] = 0;
  s.free[atomicAdd(s.nfree, 1)] = k;
}
// the header word of both messages (the number of records), the count of records sent, and the counters of the next phase at zero
__global__ void k_floats_header(FloatsMig s, double *mlo, double *mhi, int K) {
  if (blockIdx.x || threadIdx.x) return;
  double *m[2] = {mlo, mhi};
  for (int d = 0; d < 2; d++) {
    const int c = s.msgcnt[d] < K ? s.msgcnt[d] : K;
    if (m[d]) {
      m[d][0] = (double)c;
      s.cnt[3] += (unsigned long long)c;
    }
    s.msgcnt[d] = 0;
  }
}
// every record of the two received messages pops a free slot, or takes the next one at the high-water mark when the stack is empty.
// Live floats never exceed n, so n slots suffice; pushes (k_floats_emigrate) and pops never share a launch
__global__ void __launch_bounds__(FL_THREADS) k_floats_immigrate(FloatsMig s, int n, int nl, const double *__restrict__ rlo, const double *__restrict__ rhi, int K) {
  const int t = blockIdx.x * FL_THREADS + threadIdx.x;
  if (t >= 2 * K) return;
  const double *msg = t < K ? rlo : rhi;
  const int r = t < K ? t : t - K;
  if (!msg) return;
  const double h = msg[0];
  if (!(h >= 1. && h <= (double)K) || r >= (int)h) return;
  const double *rec = msg + 1 + 6 * (size_t)r;
  int old = *(volatile int *)s.nfree, k = -1;
  while (old > 0) {
    const int was = atomicCAS(s.nfree, old, old - 1);
    if (was == old) { k = s.free[old - 1]; break; }
    old = was;
  }
  if (k < 0) k = atomicAdd(s.hw, 1);
  if (k >= n) return;   // cannot happen: at most n floats are alive
  const int id = (int)rec[0], l = (int)rec[5];
  s.id[k] = id;
  s.x[k] = rec[1];
  s.y[k] = rec[2];
  s.xh[k] = rec[3];
  s.yh[k] = rec[4];
  s.layer[k] = l < 0 ? 0 : l >= nl ? nl - 1 : l;
  s.live[k] = 1;
}

// ---- readouts on tiles: every rank scatters what it holds by id, the ranks' arrays are gathered and every id is taken from the
// rank that holds it.  out [3][n]: a, b and the presence word (zeroed before)
__global__ void __launch_bounds__(FL_THREADS) k_floats_scatter(const double *__restrict__ a, const double *__restrict__ b, FloatsTileDev t, int n,
                                                               double *__restrict__ out) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n || k >= *t.hw || !t.live[k]) return;
  const int id = t.id[k];
  if ((unsigned)id >= (unsigned)n) return;
  out[id] = a[k];
  out[(size_t)n + id] = b[k];
  out[2 * (size_t)n + id] = 1.;
}
// all [nranks][3][n] -> o0, o1 [n] (o1 may be null).  Every id is resident on exactly one rank; an id nobody holds gives NaN
__global__ void __launch_bounds__(FL_THREADS) k_floats_select(const double *__restrict__ all, int nranks, int n, double *__restrict__ o0,
                                                              double *__restrict__ o1) {
  const int id = blockIdx.x * FL_THREADS + threadIdx.x;
  if (id >= n) return;
  double a = NAN, b = NAN;
  for (int r = 0; r < nranks; r++) {
    const double *p = all + (size_t)r * 3 * n;
    if (p[2 * (size_t)n + id] != 0.) {
      a = p[id];
      b = p[(size_t)n + id];
    }
  }
  o0[id] = a;
  if (o1) o1[id] = b;
}

void launch_floats_stage(hipStream_t st, int stage, const FloatsDev &d, int n, const double *psi, const double *pg, const NatGeom &g,
                         const FloatsGeom &fg, double dt, double *rec, const FloatsTileDev *t) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS);
  with_bool(pg != nullptr, [&](auto PG) {
    with_bool(fg.periodic != 0, [&](auto PER) {
      if (t) {
        if (stage == 1) hipLaunchKernelGGL((k_floats_stage_tiled<PG.value, PER.value, 1>), gr, dim3(FL_THREADS), 0, st, d, *t, n, psi, pg, g, fg, dt, rec);
        else hipLaunchKernelGGL((k_floats_stage_tiled<PG.value, PER.value, 2>), gr, dim3(FL_THREADS), 0, st, d, *t, n, psi, pg, g, fg, dt, rec);
      } else if (stage == 1) hipLaunchKernelGGL((k_floats_stage<PG.value, PER.value, 1>), gr, dim3(FL_THREADS), 0, st, d, n, psi, pg, g, fg, dt, rec);
      else hipLaunchKernelGGL((k_floats_stage<PG.value, PER.value, 2>), gr, dim3(FL_THREADS), 0, st, d, n, psi, pg, g, fg, dt, rec);
    });
  });
}

void launch_floats_interp(hipStream_t st, const FloatsDev &d, int n, const double *f, const double *pg, const NatGeom &g, const FloatsGeom &fg,
                          double *o0, double *o1, const FloatsTileDev *t) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS);
  with_bool(pg != nullptr, [&](auto PG) {
    with_bool(fg.periodic != 0, [&](auto PER) {
      if (t) {   // o0 is the id-indexed [3][n] array; o1 only says which of the two kernels
        if (o1) hipLaunchKernelGGL((k_floats_interp_tiled<PG.value, PER.value, true>), gr, dim3(FL_THREADS), 0, st, d, *t, n, f, pg, g, fg, o0);
        else hipLaunchKernelGGL((k_floats_interp_tiled<PG.value, PER.value, false>), gr, dim3(FL_THREADS), 0, st, d, *t, n, f, pg, g, fg, o0);
      } else if (o1) hipLaunchKernelGGL((k_floats_interp<PG.value, PER.value, true>), gr, dim3(FL_THREADS), 0, st, d, n, f, pg, g, fg, o0, o1);
      else hipLaunchKernelGGL((k_floats_interp<PG.value, PER.value, false>), gr, dim3(FL_THREADS), 0, st, d, n, f, pg, g, fg, o0, o1);
    });
  });
}

void launch_floats_emigrate(hipStream_t st, const FloatsMig &s, int n, const FloatsGeom &fg, const FloatsTiling &t, int yphase, int half, double *mlo,
                            double *mhi, int K, bool node) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS);
  with_bool(yphase != 0, [&](auto YPH) {
    with_bool(node, [&](auto NODE) {
      hipLaunchKernelGGL((k_floats_emigrate<YPH.value, NODE.value>), gr, dim3(FL_THREADS), 0, st, s, n, fg, t, half, mlo, mhi, K);
    });
  });
  hipLaunchKernelGGL(k_floats_header, dim3(1), dim3(64), 0, st, s, mlo, mhi, K);
}
void launch_floats_immigrate(hipStream_t st, const FloatsMig &s, int n, int nl, const double *rlo, const double *rhi, int K) {
  hipLaunchKernelGGL(k_floats_immigrate, dim3((2 * K + FL_THREADS - 1) / FL_THREADS), dim3(FL_THREADS), 0, st, s, n, nl, rlo, rhi, K);
}
void launch_floats_scatter(hipStream_t st, const double *a, const double *b, const FloatsTileDev &t, int n, double *out) {
  hipLaunchKernelGGL(k_floats_scatter, dim3((n + FL_THREADS - 1) / FL_THREADS), dim3(FL_THREADS), 0, st, a, b, t, n, out);
}
void launch_floats_select(hipStream_t st, const double *all, int nranks, int n, double *o0, double *o1) {
  hipLaunchKernelGGL(k_floats_select, dim3((n + FL_THREADS - 1) / FL_THREADS), dim3(FL_THREADS), 0, st, all, nranks, n, o0, o1);
}
