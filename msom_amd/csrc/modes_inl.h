// modes_inl.h -- the per-column eigenproblem of the vertical-mode decomposition (msqg/eigmode.h), as one function that
// compiles for the device (k_modes_eig) and for the host (a stand-alone check of the arithmetic needs no GPU).
//
// The stretching matrix amat of eigmode.h:86-109 is D^-1 T with D = diag(dhf) and T symmetric, so its eigenproblem is that
// of the symmetric tridiagonal D^1/2 amat D^-1/2: same diagonal, off-diagonal -S_l / (dhc_l sqrt(dhf_l dhf_l+1)).  It is
// solved by cyclic Jacobi rotations with the threshold strategy of Rutishauser (Handbook for Automatic Computation II/1,
// "The Jacobi method for real symmetric matrices", 1966; the corrections of a sweep are summed apart from the diagonal, and
// an off-diagonal that no longer changes either diagonal entry in floating point is set to zero): every loop has constant
// bounds, the sweep loop ends after MODES_MAXSWEEP sweeps whatever the data are, and once unrolled every array index is a
// constant, so the matrix stays in registers.  The vector matrix and the two work vectors sit behind the accessor VS
// (registers or LDS).
#ifndef MSOM_MODES_INL_H
#define MSOM_MODES_INL_H

#include <math.h>

#include <utility>

#ifndef MODES_HD
#define MODES_HD __host__ __device__ __forceinline__
#endif
#ifndef MODES_MAXNL
#define MODES_MAXNL 16
#endif
// Passes of the sweep loop, the last of which only finds the off-diagonal sum zero, on the columns of tools/modes_host_check.cpp
// (graded, nearly unstratified, thin layers; contracted or not): nl = 2: 2, nl = 3: 5 .. 7, nl = 6 .. 16: 7 .. 11.  The cap only ends
// a run on data that cannot converge (NaN)
#define MODES_MAXSWEEP 40

// f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}): a loop whose index is a constant in every body,
// whatever the optimiser's unrolling limits are (the rotation loop of 16 layers is 120 bodies)
template <int... I, class F>
MODES_HD void modes_static_for_impl(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
MODES_HD void modes_static_for(F &&f) {
  modes_static_for_impl(std::make_integer_sequence<int, N>{}, f);
}
// pair number t = 0 .. NL (NL - 1) / 2 - 1 of the row-cyclic order (0,1) (0,2) ... (NL-2,NL-1)
constexpr int modes_pair_p(int t, int nl) { int p = 0; while (t >= nl - 1 - p) { t -= nl - 1 - p; p++; } return p; }
constexpr int modes_pair_q(int t, int nl) { int p = 0; while (t >= nl - 1 - p) { t -= nl - 1 - p; p++; } return p + 1 + t; }

enum { MODES_OK = 0, MODES_BAD_S = 1, MODES_NOCONV = 2, MODES_WEAK = 4 };   // bits: k_modes_eig ORs them into one word

struct ModesLayers {
  double dhf[MODES_MAXNL], dhc[MODES_MAXNL];
};

// vector matrix in registers: every index is a constant after unrolling
template <int NL>
struct ModesRegV {
  double v[NL * NL], w[2 * NL];   // w: the work vectors b (0 .. NL-1) and z (NL .. 2 NL - 1) of the iteration
  MODES_HD double wget(int i) const { return w[i]; }
  MODES_HD void wset(int i, double x) { w[i] = x; }
  MODES_HD double get(int i) const { return v[i]; }
  MODES_HD void set(int i, double x) { v[i] = x; }
  // columns p, q (constants) of every row: (g, h) -> (g - s (h + g tau), h + s (g - h tau))
  MODES_HD void rotate(int p, int q, double s, double tau) {
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const double g_ = v[j * NL + p], h_ = v[j * NL + q];
      v[j * NL + p] = g_ - s * (h_ + g_ * tau);
      v[j * NL + q] = h_ + s * (g_ - h_ * tau);
    }
  }
};
// vector matrix in memory, element i of this column at p[i * stride] (LDS: stride = threads of the block)
template <int NL>
struct ModesMemV {
  double *p;      // NL * NL + 2 NL elements: the matrix, then the work vectors b and z of the iteration
  int stride;
  MODES_HD double get(int i) const { return p[(size_t)i * stride]; }
  MODES_HD void set(int i, double x) { p[(size_t)i * stride] = x; }
  MODES_HD double wget(int i) const { return get(NL * NL + i); }
  MODES_HD void wset(int i, double x) { set(NL * NL + i, x); }
  // memory takes a run-time index: two rows in flight keep the registers for the matrix
  MODES_HD void rotate(int cp, int cq, double s, double tau) {
#pragma unroll 2
    for (int j = 0; j < NL; j++) {
      const double g_ = get(j * NL + cp), h_ = get(j * NL + cq);
      set(j * NL + cp, g_ - s * (h_ + g_ * tau));
      set(j * NL + cq, h_ + s * (g_ - h_ * tau));
    }
  }
};

// S[l] = (Fr_l / Ro)^2 of the nl - 1 interfaces of one column.  On MODES_OK: d[m] = eigenvalue lambda_m of amat, V(k * NL + m) =
// vr[k][m] with Flierl's normalisation sum_k dhf_k vr_km^2 = htotal (= 1, eigmode.h:70) and vr[0][m] >= 0 (sign(x) = x > 0 ? 1 : -1;
// a mode may vanish at the surface), rank[m] = position of mode m in ascending order of the eigenvalues (ties by index).
// MODES_BAD_S: an S that is not positive and finite.  MODES_NOCONV: the sweep cap.  MODES_WEAK: with e0 <= e1 <= ... <= emax the computed
// eigenvalues, NL >= 2 and e1 <= 8 NL 2^-52 emax -- the eigenvalue error bound of the method, so neither the sign of lambda_1 nor which
// of the two near-null vectors is the barotropic one is determined (an interface too weakly stratified for fp64; a matrix entry that
// overflowed to inf ends here as well, emax = inf, or in MODES_NOCONV).  On any of the three nothing of d, V, rank is meaningful.
template <int NL, class VS>
MODES_HD int modes_eig_column(const double *S, const ModesLayers &lay, VS &V, double (&d)[NL], int (&rank)[NL]) {
  const double htotal = 1.;
  double a[NL * NL];   // upper triangle used: a[p * NL + q], p < q
#pragma unroll
  for (int p = 0; p < NL; p++) {
#pragma unroll
    for (int q = 0; q < NL; q++) {
      a[p * NL + q] = 0.;
      V.set(p * NL + q, p == q ? 1. : 0.);
    }
  }
  bool bad = false;
#pragma unroll
  for (int l = 0; l < NL; l++) {
    double lo = 0., up = 0.;   // amat[l][l-1], amat[l][l+1] (eigmode.h:91-105)
    if (l > 0) lo = -S[l - 1] / (lay.dhc[l - 1] * lay.dhf[l]);
    if (l < NL - 1) {
      const double s = S[l];
      bad = bad || !(s > 0.) || !(s <= 1.7976931348623157e308);
      up = -s / (lay.dhc[l] * lay.dhf[l]);
      a[l * NL + l + 1] = -s / (lay.dhc[l] * sqrt(lay.dhf[l] * lay.dhf[l + 1]));
    }
    d[l] = -lo - up;
    V.wset(l, d[l]);
    V.wset(NL + l, 0.);
  }
  if (bad) return MODES_BAD_S;

  bool done = NL == 1;
#pragma unroll 1
  for (int sweep = 1; sweep <= MODES_MAXSWEEP && !done; sweep++) {
    double sm = 0.;
#pragma unroll
    for (int p = 0; p < NL - 1; p++) {
#pragma unroll
      for (int q = p + 1; q < NL; q++) sm += fabs(a[p * NL + q]);
    }
    if (sm == 0.) { done = true; break; }
    const double tresh = sweep < 4 ? 0.2 * sm / (NL * NL) : 0.;
    modes_static_for<NL * (NL - 1) / 2>([&](auto T) __attribute__((always_inline)) {
      constexpr int p = modes_pair_p(T(), NL), q = modes_pair_q(T(), NL);
      {
        const double apq = a[p * NL + q], g = 100. * fabs(apq);
        if (sweep > 4 && fabs(d[p]) + g == fabs(d[p]) && fabs(d[q]) + g == fabs(d[q])) {
          a[p * NL + q] = 0.;
        } else if (fabs(apq) > tresh) {
          double h = d[q] - d[p], t;
          if (fabs(h) + g == fabs(h)) t = apq / h;
          else {
            const double theta = 0.5 * h / apq;
            t = 1. / (fabs(theta) + sqrt(1. + theta * theta));
            if (theta < 0.) t = -t;
          }
          const double c = 1. / sqrt(1. + t * t), s = t * c, tau = s / (1. + c);
          h = t * apq;
          V.wset(NL + p, V.wget(NL + p) - h);
          V.wset(NL + q, V.wget(NL + q) + h);
          d[p] -= h; d[q] += h;
          a[p * NL + q] = 0.;
#define MODES_ROT(X, Y)                       \
  do {                                        \
    const double g_ = (X), h_ = (Y);          \
    (X) = g_ - s * (h_ + g_ * tau);           \
    (Y) = h_ + s * (g_ - h_ * tau);           \
  } while (0)
#pragma unroll
          for (int j = 0; j < NL; j++) {
            if (j < p) MODES_ROT(a[j * NL + p], a[j * NL + q]);
            else if (j > p && j < q) MODES_ROT(a[p * NL + j], a[j * NL + q]);
            else if (j > q) MODES_ROT(a[p * NL + j], a[q * NL + j]);
          }
          V.rotate(p, q, s, tau);
#undef MODES_ROT
        }
      }
    });
#pragma unroll
    for (int p = 0; p < NL; p++) {
      const double bp = V.wget(p) + V.wget(NL + p);   // b += z; d = b; z = 0
      V.wset(p, bp);
      d[p] = bp;
      V.wset(NL + p, 0.);
    }
  }
  if (!done) {   // the last sweep may have finished the job
    double sm = 0.;
#pragma unroll
    for (int p = 0; p < NL - 1; p++) {
#pragma unroll
      for (int q = p + 1; q < NL; q++) sm += fabs(a[p * NL + q]);
    }
    if (!(sm == 0.)) return MODES_NOCONV;
  }
  int st = MODES_OK;
  if (NL >= 2) {   // the two smallest and the largest eigenvalue, without an indexed read of d
    double e0 = d[0], e1 = HUGE_VAL, emax = d[0];
#pragma unroll
    for (int m = 1; m < NL; m++) {
      e1 = fmin(e1, fmax(e0, d[m]));
      e0 = fmin(e0, d[m]);
      emax = fmax(emax, d[m]);
    }
    if (e1 <= 8. * NL * 2.220446049250313e-16 * emax) st = MODES_WEAK;
  }

  // back to the vectors of amat (D^-1/2), Flierl's normalisation and the surface sign, eigmode.h:213-222
#pragma unroll
  for (int k = 0; k < NL; k++) {
    const double r = sqrt(lay.dhf[k]);
#pragma unroll
    for (int m = 0; m < NL; m++) V.set(k * NL + m, V.get(k * NL + m) / r);
  }
#pragma unroll
  for (int m = 0; m < NL; m++) {
    double dotp = 0.;
#pragma unroll
    for (int k = 0; k < NL; k++) dotp += lay.dhf[k] * V.get(k * NL + m) * V.get(k * NL + m);
    const double flfac = (V.get(m) > 0. ? 1. : -1.) * sqrt(htotal / dotp);
#pragma unroll
    for (int k = 0; k < NL; k++) V.set(k * NL + m, flfac * V.get(k * NL + m));
  }
#pragma unroll
  for (int m = 0; m < NL; m++) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) r += (d[j] < d[m] || (d[j] == d[m] && j < m)) ? 1 : 0;
    rank[m] = r;
  }
  return st;
}

#endif
