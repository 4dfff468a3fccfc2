// node_floats_host_check.cpp -- stand-alone check of the index and weight arithmetic of the vertex model's Lagrangian floats (the
// vertex part of msom_amd/csrc/floats_inl.h), no GPU.  For N in {1, 2, 3, 32} every position of a list of awkward inputs is located
// and the four corners of its cell are read from a heap array of exactly (N + 1)^2 doubles -- the vertex layer the kernels read, no
// ghost, no pad -- so that AddressSanitizer sees any index outside [0, N] and UBSan any conversion of an out-of-range double.  The
// inputs: the walls 0 and L0 and their nextafter neighbours, every vertex line, +-1e300, +-DBL_MAX, +-0, NaN, +-inf.  Asserted:
// indices stay in [0, N - 1], weights stay in [0, 1], x = L0 reads column N with weight exactly 1, NaN and inf are routed to "lost",
// a cell of equal corners gives velocity exactly 0, the normal velocity on a constant wall is exactly 0, one stage from any of them
// ends in the box or lost.  Build with -fsanitize=address,undefined (tests/test_node_floats_host.py does); exit status 0 = all holds.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../msom_amd/csrc/floats_inl.h"

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (fails < 40) { printf("FAIL " __VA_ARGS__); printf("  [%s]\n", #cond); } \
      fails++;                                             \
    }                                                      \
  } while (0)

static std::vector<double> inputs(int n, double L) {
  const double D = L / n;
  std::vector<double> v;
  for (double c : {0., L}) {
    v.push_back(c);
    v.push_back(nextafter(c, -HUGE_VAL));
    v.push_back(nextafter(c, HUGE_VAL));
  }
  for (int i = 0; i <= n; i++) v.push_back(i * D);   // vertex lines: a = 0 up to the rounding of idx
  v.push_back(0.37 * L);
  for (double c : {1e300, -1e300, 0., -0., (double)NAN, (double)INFINITY, -(double)INFINITY, DBL_MAX, -DBL_MAX}) v.push_back(c);
  return v;
}

static void check_grid(int N, double L0) {
  const FloatsGeom g{N, N, 0, N / L0, L0, L0};
  const size_t n1 = (size_t)N + 1;
  std::vector<double> F(n1 * n1), C(n1 * n1, 0.75);   // a field, and a constant one (land)
  for (size_t k = 0; k < F.size(); k++) F[k] = sin(0.37 * k);
  for (size_t j = 0; j < n1; j++) F[j * n1] = F[j * n1 + N] = 0.25;   // constant on the walls x = 0 and x = L0
  const std::vector<double> xs = inputs(N, L0);
  long located = 0, lost = 0;
  const int before = fails;
  for (double x : xs)
    for (double y : xs) {
      const FloatsCell c = nfloats_locate(x, y, g);
      const bool fin = std::isfinite(x) && std::isfinite(y);
      if (!fin) CHECK(!c.ok, "%d: (%g, %g) not lost\n", N, x, y);
      CHECK(c.i0 >= 0 && c.i0 <= N - 1 && c.j0 >= 0 && c.j0 <= N - 1, "%d: (%g, %g) -> cell %d %d\n", N, x, y, c.i0, c.j0);
      if (!c.ok) { lost++; continue; }
      located++;
      CHECK(c.a >= 0 && c.a <= 1 && c.b >= 0 && c.b <= 1, "%d: (%g, %g) -> weights %g %g\n", N, x, y, c.a, c.b);
      // the reads of the kernel, in the vertex layer: rows j0, j0 + 1, columns i0, i0 + 1
      const size_t o = (size_t)c.j0 * n1 + c.i0;
      double u, v, xo, yo;
      floats_uv(F[o], F[o + 1], F[o + n1], F[o + n1 + 1], c.a, c.b, g.idx, &u, &v);
      const double s = floats_bilinear(F[o], F[o + 1], F[o + n1], F[o + n1 + 1], c.a, c.b);
      CHECK(std::isfinite(u) && std::isfinite(v) && std::fabs(s) <= 1 + 16 * DBL_EPSILON, "%d: (%g, %g) -> u %g v %g s %g\n", N, x, y, u, v, s);
      if (x == 0. || x == L0) CHECK(u == 0., "%d: normal velocity %g on the wall x = %g\n", N, u, x);
      const int flag = floats_move(x, y, u, v, 0.75, g, &xo, &yo);
      if (flag & 2) CHECK(std::isnan(xo) && std::isnan(yo), "%d: lost float at (%g, %g)\n", N, xo, yo);
      else CHECK(xo >= 0 && xo <= L0 && yo >= 0 && yo <= L0, "%d: (%g, %g) moved out of the box to (%g, %g)\n", N, x, y, xo, yo);
      // a cell of four equal corners: velocity exactly zero, the value the constant
      floats_uv(C[o], C[o + 1], C[o + n1], C[o + n1 + 1], c.a, c.b, g.idx, &u, &v);
      CHECK(u == 0. && v == 0., "%d: land velocity %g %g\n", N, u, v);
      // in the box the weight is that of the formula
      if (x >= 0 && x < L0 && x * g.idx < N) CHECK(c.a == x * g.idx - floor(x * g.idx), "%d: a of %g\n", N, x);
    }
  // the wall x = L0 reads column N with weight exactly 1, the wall x = 0 column 0 with weight 0
  const FloatsCell w = nfloats_locate(L0, 0., g);
  CHECK(w.ok && w.i0 == N - 1 && w.a == 1. && w.j0 == 0 && w.b == 0., "%d: wall cell %d %d weights %g %g\n", N, w.i0, w.j0, w.a, w.b);
  CHECK(floats_bilinear(1., 2., 3., 4., w.a, w.b) == 2., "%d: value on the wall\n", N);
  printf("N = %d, L0 = %g: %ld located, %ld lost: %s\n", N, L0, located, lost, fails > before ? "FAILED" : "ok");
}

int main() {
  int grids = 0;
  for (double L0 : {100., 80., 1. / 3.})
    for (int N : {1, 2, 3, 32}) {
      check_grid(N, L0);
      grids++;
    }
  printf("%d grids checked, %d failures\n", grids, fails);
  return fails != 0;
}
