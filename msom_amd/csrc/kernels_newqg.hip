// kernels_newqg.hip -- the PV tendency of the cell-centred one-layer model (newqg/qg.h), gfx950 / CDNA4, fp64.
//
// k_nq_rhs: one pass from psi to the tendency (update_qg after the inversion, newqg/qg.h:276-281: comp_del2 -> advection_pv ->
// dissip -> ekman_friction -> surface_forcing, and optionally advance_qg :249-261), in the mapping of kernels_lpw.hip without
// what one layer does not need:
//  * a wavefront owns a strip of 64 columns, 60 of which produce output (2 on each side are the halo: zeta at x +- 1 needs psi at
//    x +- 2) and marches up the rows of a chunk;
//  * zeta = lap(psi), lap(zeta) and the Arakawa Jacobian come from sliding register windows: a lane keeps its own column of psi
//    (5 rows) and zeta (3 rows), the x +- 1 neighbours come from the adjacent lanes by whole-wave DPP shifts;
//  * no vertical coupling, hence no LDS and no barrier: a workgroup is four independent wavefronts on adjacent strips;
//  * wall ghosts of zeta (newqg/qg.h:310-313; corners by the y rule over the x-ghost column) are produced in the lane / row that
//    holds the ghost position, from psi's ghosts; on the doubly periodic domain psi carries wrapped copies two cells deep and the
//    Laplacian at a ghost position is the wrapped copy, bit for bit: the instantiation without ghost code;
//  * psi rows, q_in and the forcing are requested one interval of NQ_R rows ahead.
//
// Expression order (the contract of the strict build, include/msom.h; E / W = x +- 1, N / S = y +- 1, D = Delta):
//   z    = ((((pE + pW) + pN) + pS) - 4*p) / (D*D)
//   J    = ((pE-pW)*(zN-zS) + (pS-pN)*(zE-zW) + pE*(zNE-zSE) - pW*(zNW-zSW) - pN*(zNE-zNW) + pS*(zSE-zSW)
//           + zN*(pNE-pNW) - zS*(pSE-pSW) - zE*(pNE-pSE) + zW*(pNW-pSW)) / ((12.*D)*D)          summed left to right
//   dq   = 0 + ((-J) - (beta*(pE - pW)) / (2*D))                     (`updates` zeroed, then +=, newqg/qg.h:267-270,200)
//   dq   = dq + nu * (((((zE + zW) + zN) + zS) - 4*z) / (D*D))
//   dq   = dq - ((hEkb*f0) / (2*dh0)) * z
//   dq   = dq + qforc
//   qout = qin + dq*dt
// The Jacobian is mjac9 of rhs_inl.h with the arguments exchanged: -J_msqg(p, q) of msqg/qg.h:252-262 is term by term the
// jacobian(q, p) macro of newqg/qg.h:128-138.
#include "rhs_inl.h"

// Product build: no automatic contraction in this file, every fused multiply-add is written out.  The kernel exists in
// instantiations with and without the ghost code and a cell must round alike in either (kernels_lpw.hip has the measurement).
#pragma clang fp contract(off)

#define NQ_W 60   // output columns of a strip (64 lanes - 2 x 2 halo)
#define NQ_R 4    // rows per prefetch interval
#define NQ_WAVES 4

struct NqArgs {
  const double *psi, *q_in, *qforc;
  double *zeta, *dq, *q_out;   // q_out != 0: q_out = q_in + dt * dq, dq not stored
  NatGeom g;
  int H;                       // rows per chunk
  double dt, D, beta, nu, cek, bc_fac;
  double rD2, rD12, rD2x;      // product build: 1 / (D*D), 1 / ((12 D) D), 1 / (2 D), formed once on the host
};

// WALLS: the four sides are walls (ghost code); QF: forcing present; ADV: advance fused
template <bool WALLS, bool QF, bool ADV>
__global__ void __launch_bounds__(64 * NQ_WAVES) k_nq_rhs(NqArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nx = a.g.nx, ny = a.g.ny;
  const ptrdiff_t pitch = a.g.pitch;
  const int strip = blockIdx.x * NQ_WAVES + wv, nstrips = (nx + NQ_W - 1) / NQ_W;
  if (strip >= nstrips) return;   // no barrier in this kernel: a wavefront may leave
  const int x0 = strip * NQ_W, y0 = blockIdx.y * a.H, y1 = min(ny, y0 + a.H);
  const int gi = x0 - 2 + lane, gic = min(gi, nx + 1);   // lanes past the ghost column re-read it (never stored, never used)
  const bool out_ok = lane >= 2 && lane <= 61 && gi < nx;
  // lanes that hold the ghost column of an x wall
  const int lW = (WALLS && x0 == 0) ? 1 : -1;
  const int eL = nx - x0 + 2;
  const int lE = (WALLS && eL <= 63) ? eL : -1;
  const double D = a.D, D2 = D * D, D12 = 12. * D * D, D2x = 2 * D;
  const double rD2 = a.rD2, rD12 = a.rD12, rD2x = a.rD2x;
  const double bc = a.bc_fac;
  const double *pP = a.psi + nat_idx(a.g, 0, 0, gic);
  // rows -2 .. ny + 1 exist (3 pad rows); the prefetch of a chunk's last interval is clamped to them
  auto ld = [&](int j) -> double { return pP[(ptrdiff_t)min(j, ny + 1) * pitch]; };
#ifdef MSOM_STRICT
  auto lap5 = [&](double c, double w, double e, double n, double s) -> double { return DIVC(e + w + n + s - 4 * c, D2, rD2); };
#else
  auto lap5 = [&](double c, double w, double e, double n, double s) -> double { return fma(-4., c, e + w + n + s) * rD2; };
#endif

  // register windows: P[k] = psi row j - 2 + k, Z[k] = zeta row j - 1 + k of the current output row j; L / R the lanes below / above
  double P[5], PL[3], PR[3], Z[3], ZL[3], ZR[3];   // PL[k], PR[k]: row j - 1 + k
#pragma unroll
  for (int k = 0; k < 5; k++) P[k] = 0.;
#pragma unroll
  for (int k = 0; k < 3; k++) PL[k] = PR[k] = Z[k] = ZL[k] = ZR[k] = 0.;

  // one marching step: psi row j + 2 enters, zeta row j + 1 is built
  auto step = [&](int j, double pnew) {
#pragma unroll
    for (int k = 0; k < 4; k++) P[k] = P[k + 1];
    P[4] = pnew;
#pragma unroll
    for (int k = 0; k < 2; k++) { PL[k] = PL[k + 1]; PR[k] = PR[k + 1]; Z[k] = Z[k + 1]; ZL[k] = ZL[k + 1]; ZR[k] = ZR[k + 1]; }
    PL[2] = lane_below(P[3]); PR[2] = lane_above(P[3]);
    double z = lap5(P[3], PL[2], PR[2], P[4], P[2]);
    if (WALLS) {
      // x walls: bc_fac * (psi[interior] - psi[ghost]), newqg/qg.h:310-311; then the y rule over every column, the x-ghost
      // columns included (:312-313 applied after them: a corner is bc_fac * (psi[x-ghost, interior row] - psi[corner]))
      if (lane == lW) z = bc * (PR[2] - P[3]);
      if (lane == lE) z = bc * (PL[2] - P[3]);
      const int r = j + 1;
      if (r == ny) z = bc * (P[2] - P[3]);
      if (r == -1) z = bc * (P[4] - P[3]);
    }
    Z[2] = z; ZL[2] = lane_below(z); ZR[2] = lane_above(z);
  };
  // the tendency of row j from the windows; returns the value to store (q_out or dq)
  auto centre = [&](double qin, double fq) -> double {
    double p[3][3], zz[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p[k][0] = PL[k]; p[k][1] = P[k + 1]; p[k][2] = PR[k];
      zz[k][0] = ZL[k]; zz[k][1] = Z[k]; zz[k][2] = ZR[k];
    }
    const double J = mjac9(zz, p, D12, rD12);
    const double be = DIVC(a.beta * (p[1][2] - p[1][0]), D2x, rD2x);
    const double lapz = lap5(Z[1], ZL[1], ZR[1], Z[2], Z[0]);
    double dq = 0. + (-J - be);
#ifdef MSOM_STRICT
    dq = dq + a.nu * lapz;
    dq = dq - a.cek * Z[1];
    if (QF) dq = dq + fq;
    return ADV ? qin + dq * a.dt : dq;
#else
    dq = fma(a.nu, lapz, dq);
    dq = fma(-a.cek, Z[1], dq);
    if (QF) dq = dq + fq;
    return ADV ? fma(dq, a.dt, qin) : dq;
#endif
  };

  // rows of the first interval start travelling before the warm-up
  double pnext[NQ_R], qreg[NQ_R], fqreg[NQ_R];
#pragma unroll
  for (int r = 0; r < NQ_R; r++) { pnext[r] = ld(y0 + r + 2); qreg[r] = fqreg[r] = 0.; }
  // warm-up: psi rows y0 - 2 .. y0 + 1 fill the windows below the chunk (zeta rows y0 - 1, y0)
  {
    double wp[4];
#pragma unroll
    for (int k = 0; k < 4; k++) wp[k] = ld(y0 - 2 + k);
#pragma unroll
    for (int k = 0; k < 4; k++) step(y0 - 4 + k, wp[k]);
  }
  double *const outp = ADV ? a.q_out : a.dq;
  // Rows past the end of a ragged chunk are computed on clamped addresses and never stored
  for (int j0 = y0; j0 < y1; j0 += NQ_R) {
#pragma unroll
    for (int r = 0; r < NQ_R; r++) {
      const size_t c = nat_idx(a.g, 0, min(j0 + r, ny - 1), gic);
      if (ADV) qreg[r] = a.q_in[c];
      if (QF) fqreg[r] = a.qforc[c];
    }
#pragma unroll
    for (int r = 0; r < NQ_R; r++) {
      const int j = j0 + r;
      const double pn = pnext[r];
      pnext[r] = ld(j + NQ_R + 2);
      step(j, pn);
      const double v = centre(qreg[r], fqreg[r]);
      if (out_ok && j < y1) {
        const size_t c = nat_idx(a.g, 0, j, gic);
        a.zeta[c] = Z[1];
        outp[c] = v;
      }
    }
  }
}

// wavefronts of k_nq_rhs a CU holds: the runtime's answer for the instantiation with the most registers (forcing and advance), asked
// once -- no LDS, so it is the register count that decides (product build 90 VGPRs: 5 per SIMD, 20 per CU)
static int nq_waves_per_cu() {
  static int waves = 0;
  if (!waves) {
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_nq_rhs<true, true, true>, 64 * NQ_WAVES, 0) != hipSuccess || blocks < 1) blocks = 2;
    waves = blocks * NQ_WAVES;
  }
  return waves;
}
int nq_rhs_rows(const NatGeom &g, int rows) {
  int H = rows;
  if (H <= 0) {
    // a launch takes ceil(wavefronts / resident wavefronts) rounds of H + 4 row steps (4 warm-up rows per chunk): the chunk
    // height that minimises that product, as launch_rhs_lpw chooses it, with this kernel's own occupancy as the capacity
    const int strips = (g.nx + NQ_W - 1) / NQ_W;
    const double cap = (double)nq_waves_per_cu() * device_cu_count();
    double best = -1.;
    for (int h = 64; h >= 8; h -= 8) {
      const double r = (double)strips * ((g.ny + h - 1) / h) / cap, cost = (r <= 3. ? ceil(r) : r + 0.5) * (h + 4);
      if (best < 0. || cost < best) { best = cost; H = h; }
    }
  }
  if (H < NQ_R) H = NQ_R;
  return H;
}

void launch_nq_rhs(hipStream_t st, const double *psi, const double *qforc, double *zeta, double *dq, const NatGeom &g, int walls, double D,
                   double beta, double nu, double cek, double bc_fac, const double *q_in, double *q_out, double dt, int rows) {
  NqArgs a;
  a.psi = psi; a.q_in = q_in; a.qforc = qforc; a.zeta = zeta; a.dq = dq; a.q_out = q_out; a.g = g; a.dt = dt;
  a.D = D; a.beta = beta; a.nu = nu; a.cek = cek; a.bc_fac = bc_fac;
  a.rD2 = 1. / (D * D); a.rD12 = 1. / (12. * D * D); a.rD2x = 1. / (2 * D);
  a.H = nq_rhs_rows(g, rows);
  const int strips = (g.nx + NQ_W - 1) / NQ_W;
  const dim3 gr((strips + NQ_WAVES - 1) / NQ_WAVES, (g.ny + a.H - 1) / a.H), bl(64 * NQ_WAVES);
  with_bool(!(walls & WALL_PER), [&](auto W) {
    with_bool(qforc != nullptr, [&](auto Q) {
      constexpr bool WL = decltype(W)::value, QF = decltype(Q)::value;
      if (q_out) hipLaunchKernelGGL((k_nq_rhs<WL, QF, true>), gr, bl, 0, st, a);
      else hipLaunchKernelGGL((k_nq_rhs<WL, QF, false>), gr, bl, 0, st, a);
    });
  });
}

// ------------------------------------------------------------------ the validation chain (option nq_fused = 0): one launch per loop

#define BX 64
#define BY 4

// ghost ring of zeta / q on a walled domain, newqg/qg.h:310-318: f[ghost] = bc_fac * (psi[interior] - psi[ghost]); x sides first,
// then the y sides over the x-ghost columns (corners by the y rule).  f's interior is not read.
__global__ void k_nq_ghost(const double *__restrict__ psi, double *f, NatGeom g, double bc_fac) {
  const int per = 2 * g.ny + 2 * (g.nx + 2);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= per) return;
  int i, j, ii, ji;   // ghost cell (i, j), its interior-side neighbour (ii, ji)
  if (t < 2 * g.ny) {
    j = ji = t >> 1;
    if (t & 1) { i = g.nx; ii = g.nx - 1; } else { i = -1; ii = 0; }
  } else {
    const int q = t - 2 * g.ny;
    i = ii = (q >> 1) - 1;
    if (q & 1) { j = g.ny; ji = g.ny - 1; } else { j = -1; ji = 0; }
  }
  f[nat_idx(g, 0, j, i)] = bc_fac * (psi[nat_idx(g, 0, ji, ii)] - psi[nat_idx(g, 0, j, i)]);
}
void launch_nq_ghost(hipStream_t st, const double *psi, double *f, const NatGeom &g, double bc_fac) {
  const int n = 2 * g.ny + 2 * (g.nx + 2);
  hipLaunchKernelGGL(k_nq_ghost, dim3((n + 255) / 256), dim3(256), 0, st, psi, f, g, bc_fac);
}

// advection_pv, newqg/qg.h:199-200 on zeroed updates: dq = 0 + ((-J(psi, zeta)) - beta_effect(psi)); zeta with its ghost ring
__global__ void __launch_bounds__(BX *BY) k_nq_adv(const double *__restrict__ psi, const double *__restrict__ zeta, double *dq, NatGeom g,
                                                   double beta, double D12, double rD12, double D2x, double rD2x) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const size_t c = nat_idx(g, 0, j, i);
  const ptrdiff_t pitch = g.pitch;
  double p[3][3], zz[3][3];
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      p[dy + 1][dx + 1] = psi[(ptrdiff_t)c + dy * pitch + dx];
      zz[dy + 1][dx + 1] = zeta[(ptrdiff_t)c + dy * pitch + dx];
    }
  const double J = mjac9(zz, p, D12, rD12);
  const double be = DIVC(beta * (p[1][2] - p[1][0]), D2x, rD2x);
  dq[c] = 0. + (-J - be);
}
void launch_nq_adv(hipStream_t st, const double *psi, const double *zeta, double *dq, const NatGeom &g, double D, double beta) {
  const double D12 = 12. * D * D, D2x = 2 * D;
  hipLaunchKernelGGL(k_nq_adv, dim3((g.nx + BX - 1) / BX, (g.ny + BY - 1) / BY), dim3(BX, BY), 0, st, psi, zeta, dq, g, beta, D12, 1. / D12, D2x,
                     1. / D2x);
}
