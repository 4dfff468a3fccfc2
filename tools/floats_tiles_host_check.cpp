// floats_tiles_host_check.cpp -- stand-alone check of the owner rule of the Lagrangian floats on tiles (floats_owner_axis, floats_owner,
// floats_hop of msom_amd/csrc/floats_inl.h), no GPU.  For tile sizes {1, 2, 16} x tiles per side {1, 2, 4}, walls and periodic, every
// position of a list of awkward inputs is located on the global geometry and given to its owner, and the four corners of its dual
// cell are read from a heap array of exactly the owner tile's ghosted layer, (tn + 2) x (tn + 2) doubles, so that AddressSanitizer
// sees any local corner index outside [-1, tn] and UBSan any conversion of an out-of-range double.  The inputs: every seam and its
// nextafter neighbours, the cell-centre lines on either side of a seam (where i0, and with it the owner, changes) and theirs, 0 and
// L, +-1e300, +-0, NaN, +-inf, and on periodic domains -3.7 L and 1e9 L.  Asserted: the owner is a tile of the tiling, the local
// corner indices lie in [-1, tn], the owner agrees with brute force (the tile whose cells, or whose wall ghost, hold the lower corner),
// the value read through the owner's ghosted layer is the value the single tile reads, and floats_hop names a neighbour's direction
// exactly for the neighbours.  Build with -fsanitize=address,undefined (tests/test_floats_tiles_host.py does); exit status 0 =
// everything holds.
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

static std::vector<double> inputs(int tn, int p, double L, bool periodic) {
  const int n = tn * p;
  const double D = L / n;
  std::vector<double> v;
  auto with_neighbours = [&](double c) {
    v.push_back(c);
    v.push_back(nextafter(c, -HUGE_VAL));
    v.push_back(nextafter(c, HUGE_VAL));
  };
  for (int k = 0; k <= p; k++) {   // seams, the walls (or the wrap seam) among them, and the centre lines on either side
    with_neighbours(k * tn * D);
    with_neighbours((k * tn - 0.5) * D);
    with_neighbours((k * tn + 0.5) * D);
  }
  for (double c : {1e300, -1e300, 0., -0., (double)NAN, (double)INFINITY, -(double)INFINITY, DBL_MAX, -DBL_MAX}) v.push_back(c);
  if (periodic) {
    v.push_back(-3.7 * L);
    v.push_back(1e9 * L);
  }
  return v;
}

// the value the single tile holds at (i, j) of its ghosted layer, i in [-1, n]: anything that tells the cells apart
static double cell_value(int i, int j) { return sin(0.37 * i + 1.3) + cos(0.91 * j - 0.2); }

static void check_tiling(int tn, int p, bool periodic) {
  const double L0 = 80.;
  const int n = tn * p;
  const FloatsGeom g{n, n, periodic, n / L0, L0, L0};
  const std::vector<double> xs = inputs(tn, p, L0, periodic);
  const int before = fails;
  long located = 0, lost = 0;
  for (double x : xs)
    for (double y : xs) {
      const FloatsCell c = floats_locate(x, y, g);
      if (!c.ok) { lost++; continue; }   // stays where it is, nothing is read
      located++;
      FloatsTiling t{p, p, 0, 0, tn, tn};
      int col, row;
      floats_owner(c, t, &col, &row);
      CHECK(col >= 0 && col < p && row >= 0 && row < p, "tile %d x %d per %d: (%g, %g) -> owner %d %d\n", tn, p, (int)periodic, x, y, col, row);
      if (!(col >= 0 && col < p && row >= 0 && row < p)) continue;
      // brute force: the tile whose columns [ox, ox + tn) hold i0; the wall ghost -1 goes with the first tile
      int bcol = -1, brow = -1;
      for (int k = 0; k < p; k++) {
        if ((c.i0 >= k * tn && c.i0 < (k + 1) * tn) || (k == 0 && c.i0 == -1)) bcol = k;
        if ((c.j0 >= k * tn && c.j0 < (k + 1) * tn) || (k == 0 && c.j0 == -1)) brow = k;
      }
      CHECK(col == bcol && row == brow, "tile %d x %d per %d: (%g, %g) cell %d %d -> owner %d %d, brute force %d %d\n", tn, p, (int)periodic, x, y, c.i0,
            c.j0, col, row, bcol, brow);
      // the owner's ghosted layer, filled with what the exchange leaves there: the global cell of every local index in [-1, tn]
      const int ox = col * tn, oy = row * tn;
      std::vector<double> F((size_t)(tn + 2) * (tn + 2));
      for (int j = -1; j <= tn; j++)
        for (int i = -1; i <= tn; i++) F[(size_t)(j + 1) * (tn + 2) + (i + 1)] = cell_value(ox + i, oy + j);
      const int li = c.i0 - ox, lj = c.j0 - oy;
      CHECK(li >= -1 && li + 1 <= tn && lj >= -1 && lj + 1 <= tn, "tile %d x %d per %d: (%g, %g) -> local corner %d %d\n", tn, p, (int)periodic, x, y, li, lj);
      if (!(li >= -1 && li + 1 <= tn && lj >= -1 && lj + 1 <= tn)) continue;
      const double *q = &F[(size_t)(lj + 1) * (tn + 2) + (li + 1)];
      CHECK(q[0] == cell_value(c.i0, c.j0) && q[1] == cell_value(c.i0 + 1, c.j0) && q[tn + 2] == cell_value(c.i0, c.j0 + 1) &&
                q[tn + 3] == cell_value(c.i0 + 1, c.j0 + 1),
            "tile %d x %d: (%g, %g) reads other cells than the single tile\n", tn, p, x, y);
      // seen from every tile of the row: stay, a neighbour's direction, or farther
      for (int at = 0; at < p; at++) {
        const int h = floats_hop(col, at, p, periodic);
        const int up = periodic ? (at + 1) % p : at + 1, dn = periodic ? (at - 1 + p) % p : at - 1;
        const int want = col == at ? 0 : col == up ? 1 : col == dn ? -1 : 2;
        CHECK(h == want, "hop(%d, %d, %d, %d) = %d, not %d\n", col, at, p, (int)periodic, h, want);
      }
    }
  printf("tiles of %d, %d per side, %s: %ld located, %ld lost: %s\n", tn, p, periodic ? "periodic" : "walls", located, lost, fails == before ? "ok" : "FAILED");
}

int main() {
  int tilings = 0;
  for (int periodic = 0; periodic < 2; periodic++)
    for (int tn : {1, 2, 16})
      for (int p : {1, 2, 4}) {
        check_tiling(tn, p, periodic != 0);
        tilings++;
      }
  printf("%d tilings checked, %d failures\n", tilings, fails);
  return fails != 0;
}
