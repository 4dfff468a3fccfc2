// node_tile_host_check.cpp -- stand-alone check of the vertex model's tile index arithmetic (msom_amd/csrc/node_tile_inl.h), no GPU.
//
// For N in {8 .. 256}, every power-of-two px, py <= 8 and mg_coarse in {0, 4, 8, 32} the windows, wall bits, update / sum / halo
// ranges, the gather level and the piece offsets of the gather are compared with brute force over the global vertices of every
// level: every global vertex has a holder (1 inside a tile, 2 on a seam, 4 at a cross point), every vertex is in exactly one tile's
// sum set, origins of tiled levels are even, a held vertex is updated if and only if it is not on the domain boundary, a halo
// vertex is the neighbour's first inner column or row, and the gathered buffer assembles to the global level.  Decompositions that
// msomn_create_tiled must refuse are checked to be refused.  Build with -fsanitize=address,undefined (tests/test_node_tile_host.py
// does); exit status 0 = everything agrees.
#include <cstdio>
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

// windows, walls and ranges of level k of one decomposition against the global vertices
static void check_level(int N, int px, int py, int k, bool tiled) {
  const int n = N >> k, n1 = n + 1, P = px * py;
  std::vector<int> holders((size_t)n1 * n1, 0), summed((size_t)n1 * n1, 0);
  std::vector<std::vector<int>> held(P);   // global vertex id of every local vertex, per rank (what a neighbour's halo reads)
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, k);
    CHECK(t.ix == r % px && t.iy == r / px, "N %d %dx%d level %d rank %d: tile coordinates\n", N, px, py, k, r);
    CHECK(t.tx * px == n && t.ty * py == n && t.tx >= 1 && t.ty >= 1, "N %d %dx%d level %d: tile size %d x %d\n", N, px, py, k, t.tx, t.ty);
    if (tiled) {
      CHECK(t.tx >= 2 && t.ty >= 2, "N %d %dx%d tiled level %d: tile side below 2 cells\n", N, px, py, k);
      CHECK(!(t.ox & 1) && !(t.oy & 1), "N %d %dx%d tiled level %d rank %d: odd origin %d %d\n", N, px, py, k, r, t.ox, t.oy);
    }
    // the wall bits say which tile edges lie on the domain boundary
    CHECK(!!(t.walls & NT_WALL_W) == (t.ox == 0) && !!(t.walls & NT_WALL_E) == (t.ox + t.tx == n) && !!(t.walls & NT_WALL_S) == (t.oy == 0) &&
              !!(t.walls & NT_WALL_N) == (t.oy + t.ty == n),
          "N %d %dx%d level %d rank %d: walls %d\n", N, px, py, k, r, t.walls);
    CHECK(t.walls == ntile_walls(px, py, r), "walls differ from ntile_walls\n");
    if (P == 1) CHECK(t.walls == NT_WALL_ALL, "a single tile is not WALL_ALL\n");
    const NodeRange up = ntile_update_range(t), su = ntile_sum_range(t), ha = ntile_halo_range(t);
    held[r].assign((size_t)(t.tx + 1) * (t.ty + 1), -1);
    for (int j = -1; j <= t.ty + 1; j++)
      for (int i = -1; i <= t.tx + 1; i++) {
        const int I = t.ox + i, J = t.oy + j;
        const bool in_tile = i >= 0 && i <= t.tx && j >= 0 && j <= t.ty, in_domain = I >= 0 && I <= n && J >= 0 && J <= n;
        // the halo ring exists where the domain goes on, and nowhere else
        CHECK(ntile_in(ha, i, j) == in_domain, "N %d %dx%d level %d rank %d: halo range at %d %d\n", N, px, py, k, r, i, j);
        if (!in_tile) { CHECK(!ntile_in(up, i, j) && !ntile_in(su, i, j), "a range leaves the tile\n"); continue; }
        CHECK(in_domain, "N %d %dx%d level %d rank %d: held vertex %d %d outside the domain\n", N, px, py, k, r, I, J);
        if (!in_domain) continue;
        holders[(size_t)J * n1 + I]++;
        held[r][(size_t)j * (t.tx + 1) + i] = J * n1 + I;
        if (ntile_in(su, i, j)) summed[(size_t)J * n1 + I]++;
        const bool boundary = I == 0 || I == n || J == 0 || J == n;
        CHECK(ntile_in(up, i, j) == !boundary, "N %d %dx%d level %d rank %d: update range at %d %d (global %d %d)\n", N, px, py, k, r, i, j, I, J);
      }
  }
  for (int J = 0; J <= n; J++)
    for (int I = 0; I <= n; I++) {
      const int tx = n / px, ty = n / py;
      const int want = ((I % tx == 0 && I > 0 && I < n) ? 2 : 1) * ((J % ty == 0 && J > 0 && J < n) ? 2 : 1);
      CHECK(holders[(size_t)J * n1 + I] == want, "N %d %dx%d level %d: vertex %d %d has %d holders, not %d\n", N, px, py, k, I, J, holders[(size_t)J * n1 + I], want);
      CHECK(summed[(size_t)J * n1 + I] == 1, "N %d %dx%d level %d: vertex %d %d is summed %d times\n", N, px, py, k, I, J, summed[(size_t)J * n1 + I]);
    }
  // the halo of an interior edge is the neighbour's first inner column / row, corners included: local -1 <-> its t - 1, local t + 1 <-> its 1
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, k);
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        if (!dx && !dy) continue;
        const int nb = ntile_neighbour(px, py, r, dx, dy);
        const bool wall = (dx < 0 && (t.walls & NT_WALL_W)) || (dx > 0 && (t.walls & NT_WALL_E)) || (dy < 0 && (t.walls & NT_WALL_S)) || (dy > 0 && (t.walls & NT_WALL_N));
        CHECK((nb < 0) == wall, "N %d %dx%d rank %d: neighbour %d %d is %d\n", N, px, py, r, dx, dy, nb);
        if (nb < 0) continue;
        const NodeTile u = ntile_level(N, px, py, nb, k);
        const int i0 = dx < 0 ? -1 : dx > 0 ? t.tx + 1 : 0, i1 = dx ? i0 : t.tx, j0 = dy < 0 ? -1 : dy > 0 ? t.ty + 1 : 0, j1 = dy ? j0 : t.ty;
        for (int j = j0; j <= j1; j++)
          for (int i = i0; i <= i1; i++) {
            const int ui = dx < 0 ? u.tx - 1 : dx > 0 ? 1 : i, uj = dy < 0 ? u.ty - 1 : dy > 0 ? 1 : j;   // the strip the neighbour packs
            const int I = t.ox + i, J = t.oy + j;
            CHECK(ui >= 0 && ui <= u.tx && uj >= 0 && uj <= u.ty && held[nb][(size_t)uj * (u.tx + 1) + ui] == J * n1 + I,
                  "N %d %dx%d level %d rank %d: halo %d %d is not vertex %d %d of rank %d\n", N, px, py, k, r, i, j, ui, uj, nb);
          }
      }
  }
}

// the gathered buffer of level k: every rank writes the global vertex id of what it holds, the assembly reads the global level back
static void check_gather(int N, int px, int py, int k) {
  const int n = N >> k, n1 = n + 1, P = px * py, nl = 2;
  const long piece = ntile_piece_count(N, px, py, k, nl);
  std::vector<long> buf((size_t)(piece * P), -1);
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, k);
    CHECK(piece == (long)nl * (t.tx + 1) * (t.ty + 1), "N %d %dx%d level %d: piece count\n", N, px, py, k);
    long o = (long)r * piece;
    for (int l = 0; l < nl; l++)
      for (int j = 0; j <= t.ty; j++)
        for (int i = 0; i <= t.tx; i++) buf[(size_t)o++] = ((long)l * n1 + t.oy + j) * n1 + t.ox + i;
  }
  for (int l = 0; l < nl; l++)
    for (int J = 0; J <= n; J++)
      for (int I = 0; I <= n; I++) {
        int rank = -1;
        const long o = ntile_gather_src(N, px, py, k, nl, l, I, J, &rank);
        CHECK(rank >= 0 && rank < P && o >= (long)rank * piece && o < (long)(rank + 1) * piece, "N %d %dx%d level %d: source of %d %d outside its piece\n", N, px, py, k, I, J);
        if (o < 0 || o >= piece * P) continue;
        CHECK(buf[(size_t)o] == ((long)l * n1 + J) * n1 + I, "N %d %dx%d level %d: gathered vertex %d %d layer %d reads %ld\n", N, px, py, k, I, J, l, buf[(size_t)o]);
      }
}

int main() {
  const int sizes[] = {8, 16, 32, 64, 128, 256}, parts[] = {1, 2, 4, 8}, coarse[] = {0, 4, 8, 32};
  int cases = 0, refused = 0;
  for (int N : sizes)
    for (int px : parts)
      for (int py : parts) {
        const int before = fails, nlev = ntile_nlev(N);
        CHECK((N >> (nlev - 1)) == 2, "N %d: %d levels\n", N, nlev);
        if (px * py > 1 && (N / px < 2 || N / py < 2)) {   // a tile side below 2 cells
          CHECK(ntile_check(N, px, py, 0) != nullptr, "N %d %dx%d is not refused\n", N, px, py);
          refused++;
          continue;
        }
        for (int r = 0; r < px * py; r++) CHECK(ntile_check(N, px, py, r) == nullptr, "N %d %dx%d rank %d is refused\n", N, px, py, r);
        CHECK(ntile_check(N, px, py, px * py) != nullptr && ntile_check(N, px, py, -1) != nullptr, "N %d %dx%d: a bad rank is accepted\n", N, px, py);
        for (int mgc : coarse) {
          const int kg = ntile_kg(N, px, py, mgc), lim = mgc > px ? (mgc > py ? mgc : py) : (px > py ? px : py);
          CHECK(kg >= 0 && kg <= nlev, "N %d %dx%d mg_coarse %d: kg %d\n", N, px, py, mgc, kg);
          for (int k = 0; k < nlev; k++)   // kg is the FIRST level at or below the limit; level 0 stays on the tiles
            CHECK((k < kg) == ((N >> k) > lim || (k == 0 && px * py > 1)), "N %d %dx%d mg_coarse %d: kg %d but n_%d = %d, limit %d\n", N, px, py, mgc, kg, k, N >> k, lim);
          if (px * py > 1) CHECK(kg < nlev, "N %d %dx%d mg_coarse %d: no gathered level\n", N, px, py, mgc);
          if (px * py == 1 && mgc == 32 && N > 32) CHECK((N >> kg) == 32, "one tile, mg_coarse 32: kg %d\n", kg);
          for (int k = 0; k < kg; k++) check_level(N, px, py, k, true);
          if (kg < nlev) {   // the pieces of the gather: at least one cell a side
            check_level(N, px, py, kg, false);
            check_gather(N, px, py, kg);
          }
        }
        check_level(N, px, py, 0, false);   // the model fields live on the tiles whatever kg is
        cases++;
        printf("N %d tiles %d x %d: %s\n", N, px, py, fails == before ? "ok" : "FAIL");
      }
  for (int bad : {0, 3, 5, 6, 12, -2}) {
    CHECK(ntile_check(64, bad, 2, 0) != nullptr && ntile_check(64, 2, bad, 0) != nullptr, "tile grid with %d is accepted\n", bad);
  }
  CHECK(ntile_check(48, 2, 2, 0) != nullptr, "N 48 is accepted\n");
  CHECK(ntile_check(64, 64, 1, 0) != nullptr, "N 64 on 64 x 1 tiles is accepted\n");
  printf("%d decompositions checked, %d refused, %d failures\n", cases, refused, fails);
  return fails ? 1 : 0;
}
