// modes_host_check.cpp -- stand-alone driver of the per-column eigen solver of the vertical modes (msom_amd/csrc/modes_inl.h), no GPU.
//
// The routine k_modes_eig runs per thread is compiled for the host and fed the columns where an eigen solver goes wrong: graded
// stratification, a nearly unstratified interface (near-degenerate pairs), thin layers (modes that vanish at the surface), the uniform
// column with its closed form, columns that must be refused (MODES_WEAK, MODES_BAD_S), the ends of the fp64 range and data that cannot
// converge.  NL = 1, 2, 3, 6, 8 run with the register accessor ModesRegV, NL = 9, 16 with ModesMemV over a heap array of exactly
// (NL^2 + 2 NL) * 64 doubles at lane 37 of stride 64, as a lane of the kernel's LDS block: a wrong stride is a finding of
// AddressSanitizer, a neighbour's slot a changed sentinel.  The criteria are evaluated in long double against the symmetric
// tridiagonal T = D^1/2 amat D^-1/2 of the same S and dh; reference eigenvalues come from bisection on its Sturm counts.
// Build with -fsanitize=address,undefined, once with -ffp-contract=off and once with -march=native -ffp-contract=fast (the product
// build contracts the rotations) -- tests/test_modes_host.py does; one ": ok" / "FAIL" line per check, exit status 0 = all ok.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define MODES_HD inline
#include "../msom_amd/csrc/modes_inl.h"

typedef long double ld;
static const double EPS = 2.220446049250313e-16, S0 = 5000.;
static const int STRIDE = 64, LANE = 37;
static const double SENTINEL = -7.25e11;

struct Col {
  int nl;
  std::vector<double> dh, S;
};
struct Out {
  int st;
  std::vector<double> d, V;   // as the routine leaves them: V[k * nl + m]
  std::vector<int> rank;
  bool neighbours_touched;
};

template <int NL>
static Out solve(const Col &c, bool nan_dhc) {
  ModesLayers lay = {};
  for (int k = 0; k < NL; k++) lay.dhf[k] = c.dh[k];
  for (int k = 0; k < NL - 1; k++) lay.dhc[k] = 0.5 * (c.dh[k] + c.dh[k + 1]);
  if (nan_dhc) lay.dhc[0] = NAN;
  std::vector<double> S(c.S.begin(), c.S.begin() + (NL - 1));   // exactly NL - 1 numbers on the heap
  double d[NL];
  int rank[NL];
  Out o;
  o.neighbours_touched = false;
  o.V.resize(NL * NL);
  if constexpr (NL <= 8) {
    ModesRegV<NL> V;
    o.st = modes_eig_column<NL>(S.data(), lay, V, d, rank);
    for (int e = 0; e < NL * NL; e++) o.V[e] = V.get(e);
  } else {
    std::vector<double> buf((size_t)(NL * NL + 2 * NL) * STRIDE, SENTINEL);
    ModesMemV<NL> V{buf.data() + LANE, STRIDE};
    o.st = modes_eig_column<NL>(S.data(), lay, V, d, rank);
    for (int e = 0; e < NL * NL; e++) o.V[e] = V.get(e);
    for (size_t i = 0; i < buf.size(); i++)
      if ((int)(i % STRIDE) != LANE && buf[i] != SENTINEL) o.neighbours_touched = true;
  }
  o.d.assign(d, d + NL);
  o.rank.assign(rank, rank + NL);
  return o;
}
static Out run(const Col &c, bool nan_dhc = false) {
  switch (c.nl) {
    case 1: return solve<1>(c, nan_dhc);
    case 2: return solve<2>(c, nan_dhc);
    case 3: return solve<3>(c, nan_dhc);
    case 6: return solve<6>(c, nan_dhc);
    case 8: return solve<8>(c, nan_dhc);
    case 9: return solve<9>(c, nan_dhc);
    case 16: return solve<16>(c, nan_dhc);
  }
  abort();
}

// ---- columns

static std::vector<double> dh_eq(int nl) { return std::vector<double>(nl, 1. / nl); }
static std::vector<double> dh_thin(int nl) {   // geometric, the bottom layer 1e3 times the top one, sum 1
  std::vector<double> dh(nl, 1.);
  double sum = 0.;
  for (int k = 0; k < nl; k++) sum += dh[k] = nl > 1 ? pow(1e3, (double)k / (nl - 1)) : 1.;
  for (int k = 0; k < nl; k++) dh[k] /= sum;
  return dh;
}
static Col graded(int nl, double t) {
  Col c{nl, dh_eq(nl), {}};
  for (int l = 0; l < nl - 1; l++) c.S.push_back(S0 * pow(10., -8. * t * l / std::max(nl - 2, 1)));
  return c;
}
static Col weak_middle(int nl, bool thin, double factor) {
  Col c{nl, thin ? dh_thin(nl) : dh_eq(nl), std::vector<double>(std::max(nl - 1, 0), S0)};
  if (nl > 1) c.S[(nl - 1) / 2] = S0 * factor;
  return c;
}
static Col uniform(int nl, bool thin, double s) { return Col{nl, thin ? dh_thin(nl) : dh_eq(nl), std::vector<double>(std::max(nl - 1, 0), s)}; }

// ---- the long double side

struct Tri {
  std::vector<ld> a, b;   // diagonal, off-diagonal of T
  ld frob, gersh;
};
static Tri tri_of(const Col &c) {
  const int nl = c.nl;
  Tri T;
  T.a.assign(nl, 0);
  T.b.assign(std::max(nl - 1, 0), 0);
  for (int l = 0; l < nl - 1; l++) {
    const ld dhc = 0.5 * (c.dh[l] + c.dh[l + 1]), s = c.S[l];   // dhc as the handle holds it: rounded to double
    T.a[l] += s / (dhc * c.dh[l]);
    T.a[l + 1] += s / (dhc * c.dh[l + 1]);
    T.b[l] = -s / (dhc * sqrtl((ld)c.dh[l] * c.dh[l + 1]));
  }
  ld f = 0;
  T.gersh = 0;
  for (int l = 0; l < nl; l++) {
    f += T.a[l] * T.a[l];
    ld g = fabsl(T.a[l]);
    if (l > 0) g += fabsl(T.b[l - 1]);
    if (l < nl - 1) { g += fabsl(T.b[l]); f += 2 * T.b[l] * T.b[l]; }
    T.gersh = std::max(T.gersh, g);
  }
  T.frob = sqrtl(f);
  return T;
}
// eigenvalues of T below x: the signs of the pivots of T - x = L D L^T
static int sturm(const Tri &T, ld x) {
  int cnt = 0;
  ld q = 1;
  for (size_t i = 0; i < T.a.size(); i++) {
    q = T.a[i] - x - (i ? T.b[i - 1] * T.b[i - 1] / q : 0);
    if (q == 0) q = -LDBL_EPSILON * LDBL_EPSILON * (T.gersh > 0 ? T.gersh : 1);
    if (q < 0) cnt++;
  }
  return cnt;
}
static ld eig_ref(const Tri &T, int k) {   // eigenvalue k (ascending, 0-based) by bisection
  ld lo = -T.gersh, hi = T.gersh;
  for (int it = 0; it < 300; it++) {
    const ld mid = 0.5 * (lo + hi);
    if (sturm(T, mid) >= k + 1) hi = mid;
    else lo = mid;
  }
  return 0.5 * (lo + hi);
}

struct Worst {
  ld b = 0, c = 0, d = 0;   // worst ratio over its bound of the criteria (b) as a distance, (c), (d)
  int fails = 0;
  std::string why;
  void fail(const std::string &s) { fails++; if (why.empty()) why = s; }
};

// outputs of an accepted column: rank a permutation consistent with d, surface entries >= 0, everything finite
static void check_outputs(const Col &c, const Out &o, Worst &w) {
  const int nl = c.nl;
  std::vector<int> seen(nl, 0);
  for (int m = 0; m < nl; m++) {
    if (!std::isfinite(o.d[m])) w.fail("d not finite");
    int r = 0;
    for (int j = 0; j < nl; j++) r += (o.d[j] < o.d[m] || (o.d[j] == o.d[m] && j < m)) ? 1 : 0;
    if (o.rank[m] != r || r < 0 || r >= nl) w.fail("rank not the position in ascending order");
    else seen[r]++;
    if (!(o.V[m] >= 0.)) w.fail("(e) a surface entry is negative");
    for (int k = 0; k < nl; k++)
      if (!std::isfinite(o.V[k * nl + m])) w.fail("V not finite");
  }
  for (int m = 0; m < nl; m++)
    if (seen[m] != 1) w.fail("rank is no permutation");
  if (o.neighbours_touched) w.fail("a neighbouring lane's slot was written");
}

// the criteria (a) .. (e) of tests/test_gpu_modes_hard.py for one accepted column
static void check_column(const Col &c, const Out &o, Worst &w) {
  const int nl = c.nl;
  if (o.st != MODES_OK) { w.fail("status " + std::to_string(o.st) + " on a column that must succeed"); return; }
  check_outputs(c, o, w);
  if (w.fails) return;
  const Tri T = tri_of(c);
  std::vector<int> at(nl);   // at[r] = the routine's column of mode r
  for (int m = 0; m < nl; m++) at[o.rank[m]] = m;
  const ld lmax = nl > 1 ? eig_ref(T, nl - 1) : 0, tol = 8 * nl * (ld)EPS * lmax;
  if (nl > 1 && !(eig_ref(T, 1) >= 16 * tol)) w.fail("the column is no fair case: reference lambda_1 < 16 * 8 nl eps lambda_max");
  for (int r = 0; r < nl; r++) {
    const int m = at[r];
    const ld lam = r == 0 ? 0 : (ld)o.d[m];   // the kernel stores iBu_0 = 0, iBu_r = -d
    if (r >= 1) {
      // (a) iBu < 0 and Rd = sqrt(-1 / iBu) finite
      if (!(o.d[m] > 0.) || !std::isfinite(sqrt(1. / o.d[m]))) w.fail("(a) a baroclinic eigenvalue is not positive");
      // (b) Sturm counts
      if (sturm(T, lam - tol) > r || sturm(T, lam + tol) < r + 1) w.fail("(b) eigenvalue " + std::to_string(r) + " outside 8 nl eps lambda_max");
      w.b = std::max(w.b, fabsl(lam - eig_ref(T, r)) / tol);
    }
    // (c) residual
    std::vector<ld> y(nl);
    ld ny = 0, nr = 0;
    for (int k = 0; k < nl; k++) { y[k] = sqrtl((ld)c.dh[k]) * o.V[k * nl + m]; ny += y[k] * y[k]; }
    for (int k = 0; k < nl; k++) {
      ld res = (T.a[k] - lam) * y[k];
      if (k > 0) res += T.b[k - 1] * y[k - 1];
      if (k < nl - 1) res += T.b[k] * y[k + 1];
      nr += res * res;
    }
    const ld bc = 8 * nl * (ld)EPS * T.frob * sqrtl(ny);
    if (!(sqrtl(nr) <= bc)) w.fail("(c) residual of mode " + std::to_string(r));
    if (bc > 0) w.c = std::max(w.c, sqrtl(nr) / bc);
    // (d) D-orthonormality
    for (int r2 = 0; r2 < nl; r2++) {
      ld g = r2 == r ? -1 : 0;
      for (int k = 0; k < nl; k++) g += (ld)o.V[k * nl + m] * c.dh[k] * o.V[k * nl + at[r2]];
      if (!(fabsl(g) <= 8 * nl * (ld)EPS)) w.fail("(d) M2L^T D M2L - I");
      w.d = std::max(w.d, fabsl(g) / (8 * nl * (ld)EPS));
    }
  }
}

static int report(const char *what, int nl, const Worst &w, const char *extra = "") {
  if (w.fails) printf("nl = %d, %s: FAIL (%s)%s\n", nl, what, w.why.c_str(), extra);
  else printf("nl = %d, %s: ok%s\n", nl, what, extra);
  return w.fails;
}
static int report_abcd(const char *what, int nl, const Worst &w) {
  char buf[200];
  snprintf(buf, sizeof buf, "   worst over its bound: eigenvalue %.3Lf, residual %.3Lf, orthonormality %.3Lf", w.b, w.c, w.d);
  return report(what, nl, w, buf);
}

int main() {
  int fails = 0;
  const double ts[4] = {0., 1. / 3, 2. / 3, 1.};
  for (int nl : {1, 2, 3, 6, 8, 9, 16}) {
    // ---- the families that must succeed
    for (int fam = 0; fam < 3; fam++) {
      Worst w;
      for (double t : ts) {
        const Col c = fam == 0 ? graded(nl, t) : weak_middle(nl, fam == 2, pow(10., -8. * t));
        check_column(c, run(c), w);
      }
      fails += report_abcd(fam == 0 ? "graded, equal layers" : fam == 1 ? "weak middle, equal layers" : "weak middle, thin layers", nl, w);
    }
    // ---- the uniform column against its closed form
    {
      Worst w;
      const Col c = uniform(nl, false, S0);
      const Out o = run(c);
      check_column(c, o, w);
      ld worst_l = 0, worst_v = 0;
      if (!w.fails && nl > 1) {
        const ld pi = acosl(-1.L);
        std::vector<ld> lam(nl);
        for (int m = 0; m < nl; m++) lam[m] = 4 * (ld)S0 * nl * nl * powl(sinl(m * pi / (2 * nl)), 2);
        ld gap = lam[nl - 1];
        for (int m = 1; m < nl; m++) gap = std::min(gap, lam[m] - lam[m - 1]);
        gap /= lam[nl - 1];
        for (int m = 0; m < nl; m++) {
          const int r = o.rank[m];
          const ld el = fabsl((ld)o.d[m] - lam[r]) / (8 * nl * (ld)EPS * lam[nl - 1]);
          worst_l = std::max(worst_l, el);
          for (int k = 0; k < nl; k++) {
            const ld want = (r == 0 ? 1 : sqrtl(2.L)) * cosl((k + 0.5L) * r * pi / nl);
            worst_v = std::max(worst_v, fabsl((ld)o.V[k * nl + m] - want) / (4 * nl * (ld)EPS / gap * sqrtl(2.L)));
          }
        }
        if (!(worst_l <= 1)) w.fail("eigenvalues off the closed form");
        if (!(worst_v <= 1)) w.fail("vectors off the closed form");
      }
      char buf[200];
      snprintf(buf, sizeof buf, "   worst over its bound: eigenvalue %.3Lf, vector %.3Lf", worst_l, worst_v);
      fails += report("uniform column against 4 S nl^2 sin^2(m pi / 2 nl), cos((k + 1/2) m pi / nl)", nl, w, buf);
    }
    // ---- the ends of the fp64 range: never MODES_OK with a non-finite number
    {
      Worst w;
      std::string sts;
      for (double s : {1e-300, 1e-150, 1e150, 1e300, 1e306})
        for (int thin = 0; thin < 2; thin++) {
          const Col c = uniform(nl, thin != 0, s);
          const Out o = run(c);
          sts += " " + std::to_string(o.st);
          if (o.neighbours_touched) w.fail("a neighbouring lane's slot was written");
          if (o.st != MODES_OK) continue;
          check_outputs(c, o, w);
        }
      fails += report("S = 1e-300 .. 1e306 on every interface, both thickness sets", nl, w, ("   status:" + sts).c_str());
    }
    if (nl < 2) continue;
    // ---- sign and NaN in S
    {
      Worst w;
      for (int l = 0; l < nl - 1; l++)
        for (double bad : {0., -0., -1., -1e-300, (double)NAN, (double)INFINITY, -(double)INFINITY}) {
          Col c = uniform(nl, false, S0);
          c.S[l] = bad;
          if (run(c).st != MODES_BAD_S) w.fail("S = " + std::to_string(bad) + " on interface " + std::to_string(l) + " accepted");
        }
      fails += report("S <= 0, NaN, inf on any one interface is MODES_BAD_S", nl, w);
    }
    // ---- data that cannot converge: the sweep cap ends the run
    {
      Worst w;
      const Col c = uniform(nl, false, S0);
      const Out o = run(c, true);
      if (o.st != MODES_NOCONV) w.fail("status " + std::to_string(o.st));
      if (o.neighbours_touched) w.fail("a neighbouring lane's slot was written");
      fails += report("dhc[0] = NaN is MODES_NOCONV", nl, w);
    }
    // ---- columns that must be refused
    if (nl == 3 || nl == 6 || nl == 9 || nl == 16) {
      Worst w;
      for (int thin = 0; thin < 2; thin++) {
        const Col c = weak_middle(nl, thin != 0, thin ? 1e-20 : 1e-17);
        const Tri T = tri_of(c);
        if (!(eig_ref(T, 1) <= 8 * nl * (ld)EPS * eig_ref(T, nl - 1) / 16)) w.fail("the column is no fair case: reference lambda_1 > threshold / 16");
        const Out o = run(c);
        if (o.st != MODES_WEAK) w.fail("status " + std::to_string(o.st) + (thin ? " (thin)" : " (equal)"));
      }
      fails += report("S_mid = 1e-17 S0 (equal layers), 1e-20 S0 (thin layers) is MODES_WEAK", nl, w);
    }
  }
  return fails ? 1 : 0;
}
