// node_cell_tile_host_check.cpp -- stand-alone check of the cell tile layer of the vertex model (the ctile_* functions of
// msom_amd/csrc/node_tile_inl.h: the wavelet pyramids of the noise and of the scale filter on tiles), no GPU.
//
// For N in {8 .. 256}, every power-of-two px, py <= 8 and mg_coarse in {0, 4, 8, 32}, against brute force over every global cell of
// every level down to the gather level: every cell belongs to exactly one tile, tiled levels have >= 2 cells a tile side and an even
// origin (the local child parity is the global one), a ring cell comes from the rank and local index that hold the global cell it
// is -- beyond a seam the neighbour's edge cell, the diagonal neighbour's at a corner; beyond a wall the mirror cell inside --, the
// gathered buffer of level kg assembles to the global level, and the noise counter of every window and ring cell is the one the
// single tile uses for the cell it is or mirrors.  Decompositions with one-cell tiles are refused.  Build with
// -fsanitize=address,undefined (tests/test_node_cell_tile_host.py does); exit status 0 = everything agrees.
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

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// windows and ring of cell level k
static void check_cells(int N, int px, int py, int k, bool tiled) {
  const int n = N >> k, P = px * py;
  std::vector<int> owner((size_t)n * n, -1), local((size_t)n * n, -1);   // brute force: who holds global cell (I, J), and where
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, k);
    CHECK(t.tx * px == n && t.ty * py == n && t.tx >= 1 && t.ty >= 1, "N %d %dx%d level %d: tile of %d x %d cells\n", N, px, py, k, t.tx, t.ty);
    if (tiled) {
      CHECK(t.tx >= 2 && t.ty >= 2, "N %d %dx%d tiled level %d: tile side below 2 cells\n", N, px, py, k);
      CHECK(ctile_origin_even(t) && t.ox % 2 == 0 && t.oy % 2 == 0, "N %d %dx%d tiled level %d rank %d: odd origin %d %d\n", N, px, py, k, r, t.ox, t.oy);
      // the window of the next coarser level is the window of this one, halved: a cell's children are cells of the same tile
      const NodeTile c = ntile_level(N, px, py, r, k + 1);
      CHECK(c.ox * 2 == t.ox && c.oy * 2 == t.oy && c.tx * 2 == t.tx && c.ty * 2 == t.ty, "N %d %dx%d level %d rank %d: the coarser window is not half\n", N, px, py, k, r);
    }
    for (int j = 0; j < t.ty; j++)
      for (int i = 0; i < t.tx; i++) {
        const int I = t.ox + i, J = t.oy + j;
        CHECK(I >= 0 && I < n && J >= 0 && J < n, "N %d %dx%d level %d rank %d: cell %d %d outside the grid\n", N, px, py, k, r, i, j);
        if (I < 0 || I >= n || J < 0 || J >= n) continue;
        CHECK(owner[(size_t)J * n + I] == -1, "N %d %dx%d level %d: cell %d %d belongs to ranks %d and %d\n", N, px, py, k, I, J, owner[(size_t)J * n + I], r);
        owner[(size_t)J * n + I] = r;
        local[(size_t)J * n + I] = j * t.tx + i;
      }
  }
  for (size_t c = 0; c < owner.size(); c++) CHECK(owner[c] >= 0, "N %d %dx%d level %d: cell %zu belongs to nobody\n", N, px, py, k, c);
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, k);
    for (int j = -1; j <= t.ty; j++)
      for (int i = -1; i <= t.tx; i++) {
        // the global cell a window or ring cell is; beyond a wall the ghost cell mirrors the cell inside (x first, then y: a corner
        // ghost mirrors in both)
        const int I = clampi(t.ox + i, 0, n - 1), J = clampi(t.oy + j, 0, n - 1);
        int si = -9, sj = -9;
        const int src = ctile_halo_src(N, px, py, r, k, i, j, &si, &sj);
        CHECK(src >= 0 && src < P, "N %d %dx%d level %d rank %d: source rank %d of %d %d\n", N, px, py, k, r, src, i, j);
        if (src < 0 || src >= P) continue;
        const NodeTile u = ntile_level(N, px, py, src, k);
        CHECK(src == owner[(size_t)J * n + I] && si >= 0 && si < u.tx && sj >= 0 && sj < u.ty && sj * u.tx + si == local[(size_t)J * n + I],
              "N %d %dx%d level %d rank %d: ring %d %d reads %d %d of rank %d\n", N, px, py, k, r, i, j, si, sj, src);
        const bool inside = i >= 0 && i < t.tx && j >= 0 && j < t.ty;
        if (inside) { CHECK(src == r && si == i && sj == j, "a window cell is not its own source\n"); continue; }
        // beyond a seam: the neighbour behind that side (the diagonal one at a corner), its edge cell -- local 0 or t - 1, not 1 / t - 2
        const int dx = i < 0 ? -1 : i >= t.tx ? 1 : 0, dy = j < 0 ? -1 : j >= t.ty ? 1 : 0;
        const bool wx = (dx < 0 && (t.walls & NT_WALL_W)) || (dx > 0 && (t.walls & NT_WALL_E)), wy = (dy < 0 && (t.walls & NT_WALL_S)) || (dy > 0 && (t.walls & NT_WALL_N));
        const int nb = ntile_neighbour(px, py, r, wx ? 0 : dx, wy ? 0 : dy);
        CHECK(nb == src, "N %d %dx%d level %d rank %d: ring %d %d comes from rank %d, not the neighbour %d\n", N, px, py, k, r, i, j, src, nb);
        const int wi = dx == 0 ? i : wx ? (dx < 0 ? 0 : t.tx - 1) : (dx < 0 ? u.tx - 1 : 0);
        const int wj = dy == 0 ? j : wy ? (dy < 0 ? 0 : t.ty - 1) : (dy < 0 ? u.ty - 1 : 0);
        CHECK(si == wi && sj == wj, "N %d %dx%d level %d rank %d: ring %d %d reads %d %d, expected %d %d\n", N, px, py, k, r, i, j, si, sj, wi, wj);
      }
  }
}

// the gathered buffer of cell level k: every rank writes the global cell id of what it holds, the assembly reads the global level back
static void check_cell_gather(int N, int px, int py, int k) {
  const int n = N >> k, P = px * py, nl = 3;
  const long piece = ctile_piece_count(N, px, py, k, nl);
  std::vector<long> buf((size_t)(piece * P), -1);
  for (int r = 0; r < P; r++) {
    const NodeTile t = ntile_level(N, px, py, r, k);
    CHECK(piece == (long)nl * t.tx * t.ty, "N %d %dx%d level %d: piece count\n", N, px, py, k);
    long o = (long)r * piece;
    for (int l = 0; l < nl; l++)
      for (int j = 0; j < t.ty; j++)
        for (int i = 0; i < t.tx; i++) buf[(size_t)o++] = ((long)l * n + t.oy + j) * n + t.ox + i;
  }
  std::vector<int> read((size_t)(piece * P), 0);
  for (int l = 0; l < nl; l++)
    for (int J = 0; J < n; J++)
      for (int I = 0; I < n; I++) {
        int rank = -1;
        const long o = ctile_gather_src(N, px, py, k, nl, l, I, J, &rank);
        CHECK(rank >= 0 && rank < P && o >= (long)rank * piece && o < (long)(rank + 1) * piece, "N %d %dx%d level %d: source of cell %d %d outside its piece\n", N, px, py, k, I, J);
        if (o < 0 || o >= piece * P) continue;
        CHECK(buf[(size_t)o] == ((long)l * n + J) * n + I, "N %d %dx%d level %d: gathered cell %d %d layer %d reads %ld\n", N, px, py, k, I, J, l, buf[(size_t)o]);
        read[(size_t)o]++;
      }
  for (size_t o = 0; o < read.size(); o++) CHECK(read[o] == 1, "N %d %dx%d level %d: element %zu of the gathered buffer is read %d times\n", N, px, py, k, o, read[o]);
}

// the counter of the device noise of every window and ring cell against the single tile's (k_n_noise: sj * N + si with the clamped
// indices of the whole grid)
static void check_noise_index(int N, int px, int py) {
  for (int r = 0; r < px * py; r++) {
    const NodeTile t = ntile_level(N, px, py, r, 0);
    for (int j = -1; j <= t.ty; j++)
      for (int i = -1; i <= t.tx; i++) {
        const int I = t.ox + i, J = t.oy + j;   // the cell of the single tile's launch, -1 .. N
        const int si = I < 0 ? 0 : I >= N ? N - 1 : I, sj = J < 0 ? 0 : J >= N ? N - 1 : J;
        const unsigned want = (unsigned)sj * (unsigned)N + (unsigned)si;
        CHECK(ctile_noise_index(N, t.ox, t.oy, i, j) == want, "N %d %dx%d rank %d: noise index of %d %d\n", N, px, py, r, i, j);
        // ... and it is the counter of the cell that the halo exchange or the Neumann fill would copy from
        int ci = 0, cj = 0;
        const int src = ctile_halo_src(N, px, py, r, 0, i, j, &ci, &cj);
        const NodeTile u = ntile_level(N, px, py, src, 0);
        CHECK(ctile_noise_index(N, u.ox, u.oy, ci, cj) == want, "N %d %dx%d rank %d: the source of ring %d %d draws another number\n", N, px, py, r, i, j);
      }
  }
}

int main() {
  const int sizes[] = {8, 16, 32, 64, 128, 256}, parts[] = {1, 2, 4, 8}, coarse[] = {0, 4, 8, 32};
  int cases = 0, refused = 0;
  for (int N : sizes)
    for (int px : parts)
      for (int py : parts) {
        const int before = fails;
        if (px * py > 1 && (N / px < 2 || N / py < 2)) {   // one-cell tiles
          CHECK(ntile_check(N, px, py, 0) != nullptr, "N %d %dx%d is not refused\n", N, px, py);
          refused++;
          continue;
        }
        int K = 1;   // levels of a cell pyramid: down to the 1-cell root
        while ((N >> K) >= 1) K++;
        for (int mgc : coarse) {
          const int kg = ntile_kg(N, px, py, mgc);
          if (px * py == 1) continue;   // one tile: nothing is tiled, the pyramid is the single tile's
          CHECK(kg >= 1 && kg <= K - 1, "N %d %dx%d mg_coarse %d: gather level %d outside the cell pyramid of %d levels\n", N, px, py, mgc, kg, K);
          for (int k = 0; k < kg; k++) check_cells(N, px, py, k, true);
          check_cells(N, px, py, kg, false);   // the piece: at least one cell a tile side
          check_cell_gather(N, px, py, kg);
        }
        check_cells(N, px, py, 0, false);
        check_noise_index(N, px, py);
        cases++;
        printf("N %d tiles %d x %d: %s\n", N, px, py, fails == before ? "ok" : "FAIL");
      }
  printf("%d decompositions checked, %d refused, %d failures\n", cases, refused, fails);
  return fails ? 1 : 0;
}
