// node_floats_tiles_host_check.cpp -- stand-alone check of the owner rule of the vertex model's Lagrangian floats on tiles
// (nfloats_owner_axis, nfloats_owner, nfloats_local of msom_amd/csrc/floats_inl.h, the header the kernels and msomn_floats_begin
// compile), no GPU.  For N in {2, 4, 32, 64} and every px x py of {1, 2, 4}^2 that the vertex model runs on (node_tile_inl.h's
// ntile_check; non-square tilings included), every position of a list of awkward inputs is located on the global geometry and given to
// its owner, and the four corners of its cell are read from a heap array of exactly the (tx + 1) x (ty + 1) vertices the owner holds,
// so that AddressSanitizer sees any local corner outside [0, tx] x [0, ty] and UBSan any conversion of an out-of-range double.  The
// inputs: every seam and its nextafter neighbours, 0 and L0, +-1e300, +-DBL_MAX, +-0, NaN, +-inf.  Asserted: the owner is a tile of the
// tiling and agrees with brute force (the tile whose cells hold the located cell; a position exactly on a seam belongs to the upper
// tile, x = L0 to the last), the local corners lie in [0, tx] x [0, ty], the value read through the owner's vertices is the value the
// single tile reads, x = L0 reads column tx with weight exactly 1, and floats_hop without the periodic case names a neighbour's
// direction exactly for the neighbours.  Build with -fsanitize=address,undefined (tests/test_node_floats_tiles_host.py does); exit
// status 0 = everything holds.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../msom_amd/csrc/floats_inl.h"
#include "../msom_amd/csrc/node_tile_inl.h"

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (fails < 40) { printf("FAIL " __VA_ARGS__); printf("  [%s]\n", #cond); } \
      fails++;                                             \
    }                                                      \
  } while (0)

// the seams of a p-tile axis of n cells (the walls among them) with their nextafter neighbours, and the inputs no grid explains
static std::vector<double> inputs(int n, double L) {
  const double D = L / n;
  std::vector<double> v;
  for (int p : {1, 2, 4}) {
    if (n % p) continue;
    for (int k = 0; k <= p; k++) {
      const double c = k == p ? L : k * (n / p) * D;
      v.push_back(c);
      v.push_back(nextafter(c, -HUGE_VAL));
      v.push_back(nextafter(c, HUGE_VAL));
    }
  }
  for (double c : {1e300, -1e300, 0., -0., (double)NAN, (double)INFINITY, -(double)INFINITY, DBL_MAX, -DBL_MAX, 0.37 * L, L - 0.25 * D}) v.push_back(c);
  return v;
}

// the value the single tile holds at global vertex (i, j): anything that tells the vertices apart
static double vertex_value(int i, int j) { return sin(0.37 * i + 1.3) + cos(0.91 * j - 0.2); }

static void check_tiling(int N, int px, int py) {
  const double L0 = 100.;
  const FloatsGeom g{N, N, 0, N / L0, L0, L0};
  const int tx = N / px, ty = N / py;
  const std::vector<double> xs = inputs(N, L0);
  const int before = fails;
  long located = 0, lost = 0;
  for (double x : xs)
    for (double y : xs) {
      const FloatsCell c = nfloats_locate(x, y, g);
      if (!c.ok) { lost++; continue; }   // stays where it is, nothing is read
      located++;
      CHECK(c.i0 >= 0 && c.i0 <= N - 1 && c.j0 >= 0 && c.j0 <= N - 1, "N %d: (%g, %g) -> cell %d %d\n", N, x, y, c.i0, c.j0);
      const FloatsTiling t{px, py, 0, 0, tx, ty};
      int col, row;
      nfloats_owner(c, t, &col, &row);
      CHECK(col >= 0 && col < px && row >= 0 && row < py, "N %d, %d x %d: (%g, %g) -> owner %d %d\n", N, px, py, x, y, col, row);
      if (!(col >= 0 && col < px && row >= 0 && row < py)) continue;
      // brute force: the tile whose cells [ox, ox + tx) x [oy, oy + ty) hold the cell
      int bcol = -1, brow = -1;
      for (int k = 0; k < px; k++)
        if (c.i0 >= k * tx && c.i0 < (k + 1) * tx) bcol = k;
      for (int k = 0; k < py; k++)
        if (c.j0 >= k * ty && c.j0 < (k + 1) * ty) brow = k;
      CHECK(col == bcol && row == brow, "N %d, %d x %d: (%g, %g) cell %d %d -> owner %d %d, brute force %d %d\n", N, px, py, x, y, c.i0, c.j0, col, row, bcol,
            brow);
      // the owner as the library cuts the grid (node_tile_inl.h): its origin and its size
      const NodeTile nt = ntile_level(N, px, py, row * px + col, 0);
      CHECK(nt.tx == tx && nt.ty == ty && nt.ox == col * tx && nt.oy == row * ty, "N %d, %d x %d: tile %d %d of ntile_level\n", N, px, py, col, row);
      // a position exactly on a seam belongs to the upper tile, the far wall to the last one
      if (x == L0) CHECK(col == px - 1 && c.i0 == N - 1 && c.a == 1., "N %d, %d x %d: x = L0 -> column %d, cell %d, weight %g\n", N, px, py, col, c.i0, c.a);
      if (y == L0) CHECK(row == py - 1 && c.j0 == N - 1 && c.b == 1., "N %d, %d x %d: y = L0 -> row %d, cell %d, weight %g\n", N, px, py, row, c.j0, c.b);
      for (int k = 1; k < px; k++)
        if (x == k * tx * (L0 / N)) CHECK(col == k && c.a == 0., "N %d, %d x %d: x on seam %d -> column %d, weight %g\n", N, px, py, k, col, c.a);
      for (int k = 1; k < py; k++)
        if (y == k * ty * (L0 / N)) CHECK(row == k && c.b == 0., "N %d, %d x %d: y on seam %d -> row %d, weight %g\n", N, px, py, k, row, c.b);
      // the vertices the owner holds, and nothing else: exactly (tx + 1) x (ty + 1) doubles on the heap
      std::vector<double> F((size_t)(tx + 1) * (ty + 1));
      for (int j = 0; j <= ty; j++)
        for (int i = 0; i <= tx; i++) F[(size_t)j * (tx + 1) + i] = vertex_value(nt.ox + i, nt.oy + j);
      FloatsCell lc = c;
      const bool home = nfloats_local(&lc, nt.ox, nt.oy, tx, ty);
      CHECK(home && lc.i0 == c.i0 - nt.ox && lc.j0 == c.j0 - nt.oy && lc.i0 >= 0 && lc.i0 + 1 <= tx && lc.j0 >= 0 && lc.j0 + 1 <= ty,
            "N %d, %d x %d: (%g, %g) -> local corner %d %d\n", N, px, py, x, y, lc.i0, lc.j0);
      if (!home) continue;
      const double *q = &F[(size_t)lc.j0 * (tx + 1) + lc.i0];
      CHECK(q[0] == vertex_value(c.i0, c.j0) && q[1] == vertex_value(c.i0 + 1, c.j0) && q[tx + 1] == vertex_value(c.i0, c.j0 + 1) &&
                q[tx + 2] == vertex_value(c.i0 + 1, c.j0 + 1),
            "N %d, %d x %d: (%g, %g) reads other vertices than the single tile\n", N, px, py, x, y);
      // on any other tile the float is not at home: nothing would be read for it
      for (int r = 0; r < px * py; r++) {
        if (r == row * px + col) continue;
        const NodeTile o = ntile_level(N, px, py, r, 0);
        FloatsCell oc = c;
        CHECK(!nfloats_local(&oc, o.ox, o.oy, tx, ty), "N %d, %d x %d: (%g, %g) is also at home on rank %d\n", N, px, py, x, y, r);
      }
      // seen from every tile of the row: stay, a neighbour's direction, or farther; no wrap
      for (int at = 0; at < px; at++) {
        const int h = floats_hop(col, at, px, 0);
        const int want = col == at ? 0 : col == at + 1 ? 1 : col == at - 1 ? -1 : 2;
        CHECK(h == want, "hop(%d, %d, %d, 0) = %d, not %d\n", col, at, px, h, want);
      }
    }
  printf("N %d, %d x %d tiles: %ld located, %ld lost: %s\n", N, px, py, located, lost, fails == before ? "ok" : "FAILED");
}

int main() {
  int tilings = 0;
  for (int N : {2, 4, 32, 64})
    for (int px : {1, 2, 4})
      for (int py : {1, 2, 4}) {
        if (ntile_check(N, px, py, 0)) continue;   // a decomposition the vertex model does not run on
        check_tiling(N, px, py);
        tilings++;
      }
  printf("%d tilings checked, %d failures\n", tilings, fails);
  return fails != 0;
}
