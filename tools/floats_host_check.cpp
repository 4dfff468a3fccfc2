// floats_host_check.cpp -- stand-alone check of the index and weight arithmetic of the Lagrangian floats (msom_amd/csrc/floats_inl.h),
// no GPU.  For nx, ny in {1, 2, 3, 32, 48}, walls and periodic, every position of a list of awkward inputs is located and the four
// corners of its dual cell are read from a heap array of exactly (ny + 2) x (nx + 2) doubles -- the ghosted layer the kernels read --
// so that AddressSanitizer sees any index outside [-1, n] and UBSan any conversion of an out-of-range double.  The inputs: 0, L,
// Delta / 2 and the nextafter neighbours of each, every cell-centre line, +-1e300, +-0, NaN, +-inf, and on periodic domains
// -3.7 L and 1e9 L.  Asserted: indices stay in [-1, n] (periodic: [0, n]), weights of finite inputs stay in [0, 1 + 4 eps n], NaN is
// routed to "lost", one stage from any of them ends in the box or lost.  Build with -fsanitize=address,undefined
// (tests/test_floats_host.py does); exit status 0 = everything holds.
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

static std::vector<double> inputs(int n, double L, bool periodic) {
  const double D = L / n;
  std::vector<double> v;
  for (double c : {0., L, D / 2}) {
    v.push_back(c);
    v.push_back(nextafter(c, -HUGE_VAL));
    v.push_back(nextafter(c, HUGE_VAL));
  }
  for (int i = 0; i < n; i++) v.push_back((i + 0.5) * D);   // cell-centre lines: a = 0 up to the rounding of idx
  for (double c : {1e300, -1e300, 0., -0., (double)NAN, (double)INFINITY, -(double)INFINITY, DBL_MAX, -DBL_MAX}) v.push_back(c);
  if (periodic) {
    v.push_back(-3.7 * L);
    v.push_back(1e9 * L);
  }
  return v;
}

static void check_grid(int nx, int ny, bool periodic) {
  const double L0 = 80.;
  const FloatsGeom g{nx, ny, periodic, nx / L0, L0, L0 * ny / nx};
  std::vector<double> F((size_t)(ny + 2) * (nx + 2));
  for (size_t k = 0; k < F.size(); k++) F[k] = sin(0.37 * k);
  const std::vector<double> xs = inputs(nx, g.Lx, periodic), ys = inputs(ny, g.Ly, periodic);
  const int lo = periodic ? 0 : -1;
  long located = 0, lost = 0;
  for (double x : xs)
    for (double y : ys) {
      const FloatsCell c = floats_locate(x, y, g);
      const bool fin = std::isfinite(x) && std::isfinite(y);
      if (!fin) CHECK(!c.ok, "%d x %d per %d: (%g, %g) not lost\n", nx, ny, (int)periodic, x, y);
      CHECK(c.i0 >= lo && c.i0 <= nx - 1 && c.j0 >= lo && c.j0 <= ny - 1, "%d x %d per %d: (%g, %g) -> cell %d %d\n", nx, ny, (int)periodic, x, y,
            c.i0, c.j0);
      if (!c.ok) { lost++; continue; }
      located++;
      CHECK(c.a >= 0 && c.a <= 1 + 4 * DBL_EPSILON * nx && c.b >= 0 && c.b <= 1 + 4 * DBL_EPSILON * ny, "%d x %d per %d: (%g, %g) -> weights %g %g\n",
            nx, ny, (int)periodic, x, y, c.a, c.b);
      // the reads of the kernel, in the ghosted layer: rows j0 + 1, j0 + 2, columns i0 + 1, i0 + 2
      const double *p = &F[(size_t)(c.j0 + 1) * (nx + 2) + (c.i0 + 1)];
      double u, v, xo, yo;
      floats_uv(p[0], p[1], p[nx + 2], p[nx + 3], c.a, c.b, g.idx, &u, &v);
      const double s = floats_bilinear(p[0], p[1], p[nx + 2], p[nx + 3], c.a, c.b);
      CHECK(std::isfinite(u) && std::isfinite(v) && std::fabs(s) <= 1 + 16 * DBL_EPSILON, "%d x %d: (%g, %g) -> u %g v %g s %g\n", nx, ny, x, y, u, v, s);
      const int flag = floats_move(x, y, u, v, 0.75, g, &xo, &yo);
      if (flag & 2) CHECK(std::isnan(xo) && std::isnan(yo), "%d x %d: lost float at (%g, %g)\n", nx, ny, xo, yo);
      else if (!periodic) CHECK(xo >= 0 && xo <= g.Lx && yo >= 0 && yo <= g.Ly, "%d x %d: (%g, %g) moved out of the box to (%g, %g)\n", nx, ny, x, y, xo, yo);
      // in the box the weights are those of the formula
      if (!periodic && x >= 0 && x <= g.Lx) CHECK(c.a == (x * g.idx - 0.5) - floor(x * g.idx - 0.5), "%d: a of %g\n", nx, x);
    }
  // on the walls of a walled box the lower index is the ghost column / the last cell
  if (!periodic) {
    const FloatsCell w = floats_locate(0., g.Ly, g);
    CHECK(w.i0 == -1 && w.a == 0.5 && w.j0 == ny - 1 && std::fabs(w.b - 0.5) <= 4 * DBL_EPSILON * ny, "%d x %d: wall cell %d %d weights %g %g\n", nx, ny, w.i0,
          w.j0, w.a, w.b);
  }
  printf("%d x %d %s: %ld located, %ld lost: %s\n", nx, ny, periodic ? "periodic" : "walls", located, lost, fails ? "FAILED" : "ok");
}

int main() {
  int grids = 0;
  for (int periodic = 0; periodic < 2; periodic++)
    for (int nx : {1, 2, 3, 32, 48})
      for (int ny : {1, 2, 3, 32, 48}) {
        check_grid(nx, ny, periodic != 0);
        grids++;
      }
  printf("%d grids checked, %d failures\n", grids, fails);
  return fails != 0;
}
