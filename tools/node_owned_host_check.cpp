// node_owned_host_check.cpp -- stand-alone check of the owned windows of the vertex model on tiles (ntile_owned_range of
// msom_amd/csrc/node_tile_inl.h: what a tile contributes to a state file's records and digests and to the gathers of the NetCDF
// output, option io_tiles), no GPU.
//
// For N in {8, 32, 64} and every px, py in {1, 2, 4, 8} with tile sides of at least 2 cells, against brute force over every global
// vertex: the owned windows of all ranks cover the (N + 1)^2 vertices exactly once, each lies inside the window its tile holds and
// starts at the tile's origin, a shared vertex belongs to the holder with the higher tile coordinate, the window is the one
// ntile_sum_range states with the wall bits, and the record digest of a global array (the sum of state_io.c's per-element terms
// with the GLOBAL index) is the sum of the digests the ranks form over what they own.  Build with -fsanitize=address,undefined
// (tests/test_node_owned_host.py does); exit status 0 = everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../msom_amd/csrc/node_tile_inl.h"

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (fails < 40) { printf("FAIL " __VA_ARGS__); printf("  [%s]\n", #cond); } \
      fails++;                                             \
    }                                                      \
  } while (0)

static uint64_t mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ULL;
  z ^= z >> 27; z *= 0x94d049bb133111ebULL;
  z ^= z >> 31;
  return z;
}
static uint64_t term(double v, uint64_t k) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return mix64(b + 0x9E3779B97F4A7C15ULL * (k + 1));
}

static void check(int N, int px, int py) {
  const int n1 = N + 1, P = px * py, nl = 2;
  std::vector<int> owner((size_t)n1 * n1, -1);
  std::vector<double> a((size_t)nl * n1 * n1);
  uint64_t s = 88172645463325252ULL;
  for (double &v : a) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = (double)(int64_t)(s >> 11) * 1e-9; }
  uint64_t whole = 0, parts = 0;
  for (size_t k = 0; k < a.size(); k++) whole += term(a[k], k);
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, 0);
    const NodeRange w = ntile_owned_range(N, px, py, r, 0), sum = ntile_sum_range(t);
    CHECK(w.i0 == 0 && w.j0 == 0 && w.i1 <= t.tx && w.j1 <= t.ty && w.i1 >= t.tx - 1 && w.j1 >= t.ty - 1,
          "N %d %dx%d rank %d: owned window %d..%d x %d..%d outside the held one (%d x %d cells)\n", N, px, py, r, w.i0, w.i1, w.j0, w.j1, t.tx, t.ty);
    CHECK((w.i1 == t.tx) == (t.ix == px - 1) && (w.j1 == t.ty) == (t.iy == py - 1), "N %d %dx%d rank %d: the last column / row goes to the last tile only\n", N, px, py, r);
    CHECK(w.i0 == sum.i0 && w.i1 == sum.i1 && w.j0 == sum.j0 && w.j1 == sum.j1, "N %d %dx%d rank %d: not the window of ntile_sum_range\n", N, px, py, r);
    for (int j = w.j0; j <= w.j1; j++)
      for (int i = w.i0; i <= w.i1; i++) {
        const int I = t.ox + i, J = t.oy + j;
        CHECK(I >= 0 && I < n1 && J >= 0 && J < n1, "N %d %dx%d rank %d: vertex %d %d outside the grid\n", N, px, py, r, i, j);
        if (I < 0 || I >= n1 || J < 0 || J >= n1) continue;
        CHECK(owner[(size_t)J * n1 + I] == -1, "N %d %dx%d: vertex %d %d owned by ranks %d and %d\n", N, px, py, I, J, owner[(size_t)J * n1 + I], r);
        owner[(size_t)J * n1 + I] = r;
        for (int l = 0; l < nl; l++) {   // the rank's digest word: its owned vertices with their global indices
          const size_t k = ((size_t)l * n1 + J) * n1 + I;
          parts += term(a[k], k);
        }
      }
  }
  for (int J = 0; J < n1; J++)
    for (int I = 0; I < n1; I++) {
      const int o = owner[(size_t)J * n1 + I];
      CHECK(o >= 0, "N %d %dx%d: vertex %d %d owned by nobody\n", N, px, py, I, J);
      // the holder with the higher tile coordinate: the tile whose origin the vertex is, unless it lies on the east / north wall
      const int tx = N / px, ty = N / py;
      int ix = I / tx, iy = J / ty;
      if (ix > px - 1) ix = px - 1;
      if (iy > py - 1) iy = py - 1;
      CHECK(o == iy * px + ix, "N %d %dx%d: vertex %d %d owned by rank %d, expected %d\n", N, px, py, I, J, o, iy * px + ix);
    }
  CHECK(whole == parts, "N %d %dx%d: digest %016llx, sum of the owned digests %016llx\n", N, px, py, (unsigned long long)whole, (unsigned long long)parts);
}

int main() {
  int checked = 0, refused = 0;
  for (int N : {8, 32, 64})
    for (int px : {1, 2, 4, 8})
      for (int py : {1, 2, 4, 8}) {
        if (ntile_check(N, px, py, 0)) { refused++; continue; }
        const int before = fails;
        check(N, px, py);
        checked++;
        if (fails == before) printf("N %d %d x %d: ok\n", N, px, py);
      }
  printf("%d decompositions checked, %d refused, %d failures\n", checked, refused, fails);
  return fails ? 1 : 0;
}
