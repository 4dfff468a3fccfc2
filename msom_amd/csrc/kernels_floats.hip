// kernels_floats.hip -- Lagrangian floats (msom_floats_*): one float per lane, structure of arrays.  The
// arithmetic is floats_inl.h, shared with the host check; a kernel adds the four gathers of the dual cell's corners from the natural
// layout (ghost ring included: corner indices lie in [-1, n] by construction, whatever the position's bits) and the stores.  The
// floats are not sorted: neighbours in space stay neighbours for many steps and the gathers are left to L2.
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
// position is not finite reads nothing and stays NaN; it is counted when it becomes so, that is once
template <bool PG, bool PERIODIC, int STAGE>
__global__ void __launch_bounds__(FL_THREADS) k_floats_stage(FloatsDev d, int n, const double *__restrict__ psi, const double *__restrict__ pg, NatGeom g,
                                                             FloatsGeom fg, double dt, double *__restrict__ rec) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n) return;
  fg.periodic = PERIODIC;
  const double bx = d.x[k], by = d.y[k];
  const double px = STAGE == 1 ? bx : d.xh[k], py = STAGE == 1 ? by : d.yh[k];
  const FloatsCell c = floats_locate(px, py, fg);
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
      rec[k] = ox;
      rec[(size_t)n + k] = oy;
    }
  }
  if (flag & 1) atomicAdd(&d.cnt[0], 1ull);
  if (flag & 2) atomicAdd(&d.cnt[1], 1ull);
}

// VEL: o0 = u, o1 = v at (x, y); else o0 = the bilinear value of f there
template <bool PG, bool PERIODIC, bool VEL>
__global__ void __launch_bounds__(FL_THREADS) k_floats_interp(FloatsDev d, int n, const double *__restrict__ f, const double *__restrict__ pg, NatGeom g,
                                                              FloatsGeom fg, double *__restrict__ o0, double *__restrict__ o1) {
  const int k = blockIdx.x * FL_THREADS + threadIdx.x;
  if (k >= n) return;
  fg.periodic = PERIODIC;
  const FloatsCell c = floats_locate(d.x[k], d.y[k], fg);
  double r0 = NAN, r1 = NAN;
  if (c.ok) {
    double P[4];
    fl_corners<PG>(f, pg, g, d.layer[k], c, P);
    if constexpr (VEL) floats_uv(P[0], P[1], P[2], P[3], c.a, c.b, fg.idx, &r0, &r1);
    else r0 = floats_bilinear(P[0], P[1], P[2], P[3], c.a, c.b);
  }
  o0[k] = r0;
  if constexpr (VEL) o1[k] = r1;
}

void launch_floats_stage(hipStream_t st, int stage, const FloatsDev &d, int n, const double *psi, const double *pg, const NatGeom &g,
                         const FloatsGeom &fg, double dt, double *rec) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS);
  with_bool(pg != nullptr, [&](auto PG) {
    with_bool(fg.periodic != 0, [&](auto PER) {
      if (stage == 1) hipLaunchKernelGGL((k_floats_stage<PG.value, PER.value, 1>), gr, dim3(FL_THREADS), 0, st, d, n, psi, pg, g, fg, dt, rec);
      else hipLaunchKernelGGL((k_floats_stage<PG.value, PER.value, 2>), gr, dim3(FL_THREADS), 0, st, d, n, psi, pg, g, fg, dt, rec);
    });
  });
}

void launch_floats_interp(hipStream_t st, const FloatsDev &d, int n, const double *f, const double *pg, const NatGeom &g, const FloatsGeom &fg,
                          double *o0, double *o1) {
  const dim3 gr((n + FL_THREADS - 1) / FL_THREADS);
  with_bool(pg != nullptr, [&](auto PG) {
    with_bool(fg.periodic != 0, [&](auto PER) {
      if (o1) hipLaunchKernelGGL((k_floats_interp<PG.value, PER.value, true>), gr, dim3(FL_THREADS), 0, st, d, n, f, pg, g, fg, o0, o1);
      else hipLaunchKernelGGL((k_floats_interp<PG.value, PER.value, false>), gr, dim3(FL_THREADS), 0, st, d, n, f, pg, g, fg, o0, o1);
    });
  });
}
