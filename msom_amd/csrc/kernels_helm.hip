// kernels_helm.hip -- smoother and residual of the modal PV inversion (option mode_pv_invert), gfx950 / CDNA4, fp64.
//
// Reference: the MODE_PV_INVERT body of invertq, msqg/qg.h:136-141: nl calls of Basilisk's poisson(pm, qm, lambda = iBu), i.e.
// nl independent problems  lap(a_m) + iBu_m a_m = b_m  with no vertical coupling.  Here a "layer" of the multigrid arrays is a mode,
// every mode of a level goes in one launch, and everything else of the cycle (launch_restrict, launch_prolong, launch_correct, the
// ghost rules of split_write_ghosts) is the layered solver's, unchanged.
//
// Layout and colouring as in kernels_mg.hip: x-parity split rows, red = (i + j) even first; a colour half-sweep reads the other
// colour's half rows and its own half rows of the right-hand side, and writes its own half rows -- contiguous 64-lane accesses.
// A sweep (two half-sweeps) moves 3 w in the compact form: a read once as neighbours and written once, b read once (+ 1 w of iBu in
// the general form); the neighbour reads of rows j -+ 1 and of the other half row are the same lines and meet in L2.
//
// Per-mode sweep counts come by value: mode m takes part in sweep s while cnt.n[m] > s.  The test is uniform over the launch, so a
// mode that is out issues no load and no store.  The loop over the modes is unrolled (NL is a template argument, constant indices
// into the kernel arguments): no private segment.
//
// Arithmetic in the documented order (include/msom.h): strict build as written with true divisions, product build with the two
// pinned fused multiply-adds and the reciprocal of the diagonal (host-made in the compact form, 1 / helm_diag per cell in the general
// form: the same IEEE division, so the two forms give the same bits on a uniform table).
#include "kernels.h"
#include "mg_inl.h"
#include "rhs_inl.h"   // DIVC

#define BX 64
#define BY 4
static inline dim3 grid2d(int nx, int ny) { return dim3((nx + BX - 1) / BX, (ny + BY - 1) / BY); }
static inline dim3 block2d() { return dim3(BX, BY); }

__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

HelmCoef helm_coef(const double *ibu, int nl, double sqD) {
  HelmCoef hc = {};
  for (int m = 0; m < nl; m++) {
    hc.ibu[m] = ibu[m];
    hc.rd[m] = 1. / helm_diag(ibu[m], sqD);
  }
  return hc;
}

// ------------------------------------------------------------------ relax

struct HelmRelaxArgs {
  double *da;
  const double *res, *ibu;   // ibu: split layout of this level, nl layers (general form)
  SplitGeom g;
  int color, sweep, walls;
  double sqD;
  HelmCoef hc;
  HelmCount cnt;
};

template <int NL, bool COMPACT>
__global__ void __launch_bounds__(BX *BY) k_helm_relax(HelmRelaxArgs p) {
  const int kx = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (kx >= p.g.hk || j >= p.g.ny) return;
  const int px = (j + p.color) & 1;   // x parity of this colour's points in row j
  const int i = 2 * kx + px;
  const int hp = p.g.hp, rp = p.g.rp;
  const size_t ls = p.g.ls;
  // own cell; W / E in the other half of row j, S / N in the same half of rows j -+ 1 (k_relax_color)
  const size_t own = (size_t)(j + 1) * rp + px * hp + MSOM_SP + kx;
  const size_t oth = (size_t)(j + 1) * rp + (1 - px) * hp + MSOM_SP + kx;
  const size_t iw = oth - 1 + px, ie = oth + px, is = own - rp, in = own + rp;
  const double sqD = p.sqD;
  const bool edge = ((i == 0) | (i == p.g.nx - 1) | (j == 0) | (j == p.g.ny - 1)) && p.walls;
#pragma unroll
  for (int m = 0; m < NL; m++) {
    if (p.cnt.n[m] <= p.sweep) continue;   // this mode's sweeps are used up (or it is frozen)
    const size_t o = (size_t)m * ls;
    const double b = p.res[own + o];
    const double ae = p.da[ie + o], aw = p.da[iw + o], an = p.da[in + o], as = p.da[is + o];
#ifdef MSOM_STRICT
    const double ibu = COMPACT ? p.hc.ibu[m] : p.ibu[own + o];
    double n = -sqD * b;
    n = n + (ae + aw);
    n = n + (an + as);
    const double x = n / helm_diag(ibu, sqD);
#else
    double rd;
    if constexpr (COMPACT) rd = p.hc.rd[m];
    else rd = 1. / helm_diag(p.ibu[own + o], sqD);
    double n = fma(-sqD, b, ae + aw);
    n = n + (an + as);
    const double x = n * rd;
#endif
    p.da[own + o] = x;
    if (edge) split_write_ghosts(p.da, p.g, m, j, i, x, p.walls);
  }
}

int launch_helm_relax(hipStream_t st, double *da, const double *res, const double *ibu_sp, const HelmCoef *hc, const SplitGeom &sg, int nl,
                      double sqD, int color, int sweep, const HelmCount &cnt, int walls) {
  HelmRelaxArgs p = {};
  p.da = da; p.res = res; p.ibu = ibu_sp; p.g = sg; p.color = color; p.sweep = sweep; p.walls = walls; p.sqD = sqD; p.cnt = cnt;
  if (hc) p.hc = *hc;
  bool ok = false;
  with_bool(hc != nullptr, [&](auto C) {
    ok = with_int<1, MSOM_MAXNL>(nl, [&](auto N) { hipLaunchKernelGGL((k_helm_relax<N(), C()>), grid2d(sg.hk, sg.ny), block2d(), 0, st, p); });
  });
  return ok ? 0 : -1;
}

// ------------------------------------------------------------------ residual

// A workgroup of 64 x 4 threads covers 64 columns x HELM_RROWS * 4 rows: a thread takes HELM_RROWS rows, 4 apart, so that there is
// one atomic per mode and workgroup for 1024 cells (the maxima are non-negative: atomicMax on the bit pattern is order-independent).
#define HELM_RROWS 4
struct HelmResArgs {
  const double *a, *b, *ibu;   // a, b natural; ibu split (level 0, general form)
  double *res, *maxres, *sum_partial;
  NatGeom g;
  SplitGeom sg;
  int stride, want_sum;
  double D;
  HelmCoef hc;
};

template <int NL, bool COMPACT>
__global__ void __launch_bounds__(BX *BY) k_helm_residual(HelmResArgs p) {
  const int i = blockIdx.x * BX + threadIdx.x, j0 = blockIdx.y * (BY * HELM_RROWS) + threadIdx.y;
  double mx[NL], bs[NL];
#pragma unroll
  for (int m = 0; m < NL; m++) mx[m] = bs[m] = 0.;
  const double D = p.D, rD = 1. / D;
  if (i < p.g.nx) {
    for (int r = 0; r < HELM_RROWS; r++) {
      const int j = j0 + r * BY;
      if (j >= p.g.ny) break;
      const size_t c0 = nat_idx(p.g, 0, j, i), s0 = split_idx(p.sg, 0, j, i);
#pragma unroll
      for (int m = 0; m < NL; m++) {
        const size_t c = c0 + (size_t)m * p.g.ls, s = s0 + (size_t)m * p.sg.ls;
        const double b = p.b[c], a1 = p.a[c];
        const double aw = p.a[c - 1], ae = p.a[c + 1], as = p.a[c - p.g.pitch], an = p.a[c + p.g.pitch];
        double ibu;
        if constexpr (COMPACT) ibu = p.hc.ibu[m];
        else ibu = p.ibu[s];
#ifdef MSOM_STRICT
        double res = b - ibu * a1;
#else
        double res = fma(-ibu, a1, b);
#endif
        res += DIVC(DIVC(a1 - aw, D, rD) - DIVC(ae - a1, D, rD), D, rD);
        res += DIVC(DIVC(a1 - as, D, rD) - DIVC(an - a1, D, rD), D, rD);
        p.res[s] = res;
        mx[m] = fmax(mx[m], fabs(res));
        bs[m] += b;
      }
    }
  }
  __shared__ double smm[NL][BY], sms[NL][BY];
#pragma unroll
  for (int m = 0; m < NL; m++) {
    const double v = wave_max(mx[m]);
    if (threadIdx.x == 0) smm[m][threadIdx.y] = v;
    if (p.want_sum) {
      const double w = wave_sum(bs[m]);
      if (threadIdx.x == 0) sms[m][threadIdx.y] = w;
    }
  }
  __syncthreads();
  const int t = threadIdx.y * BX + threadIdx.x;
  if (t < NL) {
    double mm = smm[t][0];
    for (int k = 1; k < BY; k++) mm = fmax(mm, smm[t][k]);
    atomicMax((unsigned long long *)(p.maxres + t), (unsigned long long)__double_as_longlong(mm));
    if (p.want_sum) {
      double ss = sms[t][0];
      for (int k = 1; k < BY; k++) ss += sms[t][k];
      p.sum_partial[(size_t)t * p.stride + blockIdx.y * gridDim.x + blockIdx.x] = ss;
    }
  }
}

static dim3 residual_grid(const NatGeom &g) { return dim3((g.nx + BX - 1) / BX, (g.ny + BY * HELM_RROWS - 1) / (BY * HELM_RROWS)); }
int helm_residual_blocks(const NatGeom &g) {
  const dim3 gr = residual_grid(g);
  return gr.x * gr.y;
}
int launch_helm_residual(hipStream_t st, const double *a, const double *b, const double *ibu_sp, const HelmCoef *hc, const NatGeom &g, double *res,
                         const SplitGeom &sg, int nl, double D, double *maxres, double *sum_partial, int stride, int want_sum) {
  HelmResArgs p = {};
  p.a = a; p.b = b; p.ibu = ibu_sp; p.res = res; p.maxres = maxres; p.sum_partial = sum_partial; p.g = g; p.sg = sg; p.stride = stride;
  p.want_sum = want_sum; p.D = D;
  if (hc) p.hc = *hc;
  bool ok = false;
  with_bool(hc != nullptr, [&](auto C) {
    ok = with_int<1, MSOM_MAXNL>(nl, [&](auto N) { hipLaunchKernelGGL((k_helm_residual<N(), C()>), residual_grid(g), block2d(), 0, st, p); });
  });
  return ok ? 0 : -1;
}
