// node_tile_inl.h -- index arithmetic of the vertex model on tiles ("Vertex model on tiles").  Plain C++, no HIP:
// tools/node_tile_host_check.cpp checks every function here against brute force under AddressSanitizer and UBSan.
//
// The global grid has N x N cells and (N + 1)^2 vertices; level k has n_k = N >> k cells a side.  A px x py grid of tiles covers it,
// rank r = tile (r % px, r / px) as msom_create_tiled.  A tile of level k has tx = n_k / px by ty = n_k / py cells and HOLDS
// (tx + 1) x (ty + 1) vertices, the ones on its interior edges included: a vertex on a shared edge exists on both tiles (on all four
// at a cross point), every holder computes it; only the I/O asks who OWNS it (ntile_owned_range).  Local vertex (i, j) is global vertex (ox + i, oy + j).  The halo
// is the first pad column / row beyond an interior edge (i = -1, i = tx + 1, j = -1, j = ty + 1): the neighbour's local tx - 1 / 1 /
// ty - 1 / 1.  Beyond a wall the pad stays 0.
//
// Levels k < kg live on the tiles, levels k >= kg are solved on the gathered global grid by every rank.
#ifndef MSOM_NODE_TILE_INL_H
#define MSOM_NODE_TILE_INL_H

// the device kernels of the gather read the same functions
#ifdef __HIPCC__
#define NT_HD __host__ __device__
#else
#define NT_HD
#endif

// the values of WALL_W / E / S / N / ALL of msom_internal.h (which needs the HIP headers; this file must not)
enum { NT_WALL_W = 1, NT_WALL_E = 2, NT_WALL_S = 4, NT_WALL_N = 8, NT_WALL_ALL = 15 };

struct NodeTile {
  int ix, iy;   // tile coordinates
  int walls;    // NT_WALL_* bits: the sides of the tile that are sides of the domain
  int tx, ty;   // cells of the tile on this level: (tx + 1) x (ty + 1) vertices held
  int ox, oy;   // global index of local vertex (0, 0)
};
// inclusive ranges of local vertex indices
struct NodeRange {
  int i0, i1, j0, j1;
};

NT_HD static inline bool ntile_pow2(int v) { return v >= 1 && !(v & (v - 1)); }
// levels of the multigrid: the coarsest has 2 x 2 cells
NT_HD static inline int ntile_nlev(int N) {
  int n = 0;
  while ((N >> n) >= 2) n++;
  return n;
}
// null if (N, px, py, rank) is a decomposition the vertex model runs on, else what is wrong with it
NT_HD static inline const char *ntile_check(int N, int px, int py, int rank) {
  if (!ntile_pow2(px) || !ntile_pow2(py)) return "px and py must be powers of two";
  if (N < 2 || !ntile_pow2(N)) return "N must be a power of two >= 2";
  if (N % px || N % py) return "N is not divisible by the tile grid";
  if (px * py > 1 && (N / px < 2 || N / py < 2)) return "a tile side has fewer than 2 cells";
  if (rank < 0 || rank >= px * py) return "rank outside 0 .. px * py - 1";
  return nullptr;
}
NT_HD static inline int ntile_walls(int px, int py, int rank) {
  const int ix = rank % px, iy = rank / px;
  return (ix == 0 ? NT_WALL_W : 0) | (ix == px - 1 ? NT_WALL_E : 0) | (iy == 0 ? NT_WALL_S : 0) | (iy == py - 1 ? NT_WALL_N : 0);
}
// gather level: the first level whose global n_k <= max(mg_coarse, px, py); nlev if there is none (one tile with mg_coarse = 0).
// On more than one tile level 0, which holds the model fields, always stays on the tiles: kg >= 1.
// Every tiled level k < kg then has n_k >= 2 max(px, py): at least 2 cells a tile side, so tile origins are even and the local
// red-black colour (i + j) & 1 is the global one; level kg has at least 1 cell a tile side.
NT_HD static inline int ntile_kg(int N, int px, int py, int mg_coarse) {
  int lim = mg_coarse > px ? mg_coarse : px;
  if (py > lim) lim = py;
  const int nlev = ntile_nlev(N);
  int k = 0;
  while (k < nlev && (N >> k) > lim) k++;
  return px * py > 1 && k == 0 ? 1 : k;
}
// the tile of `rank` on level k (k <= kg: the window of level kg is the piece the rank contributes to the gather)
NT_HD static inline NodeTile ntile_level(int N, int px, int py, int rank, int k) {
  NodeTile t;
  t.ix = rank % px; t.iy = rank / px;
  t.walls = ntile_walls(px, py, rank);
  t.tx = (N >> k) / px; t.ty = (N >> k) / py;
  t.ox = t.ix * t.tx; t.oy = t.iy * t.ty;
  return t;
}
// the vertices a stencil kernel updates (the smoother, the residual, the restriction, the correction): all held vertices but the
// ones on a wall.  A wall side spans the whole tile edge, the shared vertices at its ends included.
NT_HD static inline NodeRange ntile_update_range(const NodeTile &t) {
  NodeRange r;
  r.i0 = (t.walls & NT_WALL_W) ? 1 : 0; r.i1 = (t.walls & NT_WALL_E) ? t.tx - 1 : t.tx;
  r.j0 = (t.walls & NT_WALL_S) ? 1 : 0; r.j1 = (t.walls & NT_WALL_N) ? t.ty - 1 : t.ty;
  return r;
}
// the vertices a tile adds to a global sum (msomn_ke, msomn_diag1d): a tile leaves out its east and north edge unless that edge is
// a wall, so every vertex is counted once
NT_HD static inline NodeRange ntile_sum_range(const NodeTile &t) {
  NodeRange r;
  r.i0 = 0; r.i1 = (t.walls & NT_WALL_E) ? t.tx : t.tx - 1;
  r.j0 = 0; r.j1 = (t.walls & NT_WALL_N) ? t.ty : t.ty - 1;
  return r;
}
// the vertices a tile OWNS where each global vertex must be counted exactly once (the records and digests of a state file, the
// gathers of msomn_write_nc; option io_tiles): local columns 0 .. tx - 1, and column tx too iff the tile is the last of its row of
// tiles; rows likewise.  Over all ranks the owned windows cover the (N + 1)^2 vertices once; a shared vertex belongs to the holder
// with the higher tile coordinate.  The same window as ntile_sum_range, stated with the tile grid instead of the wall bits
NT_HD static inline NodeRange ntile_owned_range(int N, int px, int py, int rank, int k) {
  const NodeTile t = ntile_level(N, px, py, rank, k);
  NodeRange r;
  r.i0 = 0; r.i1 = t.ix == px - 1 ? t.tx : t.tx - 1;
  r.j0 = 0; r.j1 = t.iy == py - 1 ? t.ty : t.ty - 1;
  return r;
}
// the held vertices and one halo column / row beyond every interior edge: what a halo exchange leaves valid
NT_HD static inline NodeRange ntile_halo_range(const NodeTile &t) {
  NodeRange r;
  r.i0 = (t.walls & NT_WALL_W) ? 0 : -1; r.i1 = (t.walls & NT_WALL_E) ? t.tx : t.tx + 1;
  r.j0 = (t.walls & NT_WALL_S) ? 0 : -1; r.j1 = (t.walls & NT_WALL_N) ? t.ty : t.ty + 1;
  return r;
}
NT_HD static inline bool ntile_in(const NodeRange &r, int i, int j) { return i >= r.i0 && i <= r.i1 && j >= r.j0 && j <= r.j1; }
// rank behind side (dx, dy) of the tile, -1 behind a wall
NT_HD static inline int ntile_neighbour(int px, int py, int rank, int dx, int dy) {
  const int jx = rank % px + dx, jy = rank / px + dy;
  return jx >= 0 && jx < px && jy >= 0 && jy < py ? jy * px + jx : -1;
}

// ---- the gather of level k: every rank contributes its window, [nl][ty + 1][tx + 1] contiguous, comm_allgather lines the pieces up
// by rank
NT_HD static inline long ntile_piece_count(int N, int px, int py, int k, int nl) {
  return (long)nl * ((N >> k) / px + 1) * ((N >> k) / py + 1);
}
// position of global vertex (I, J) of layer l in the gathered buffer.  A shared vertex has identical copies; the holder with the
// lower tile coordinate is read.
NT_HD static inline long ntile_gather_src(int N, int px, int py, int k, int nl, int l, int I, int J, int *rank_out = nullptr) {
  const int tx = (N >> k) / px, ty = (N >> k) / py;
  int ix = I / tx, iy = J / ty;
  if (ix > px - 1) ix = px - 1;
  if (iy > py - 1) iy = py - 1;
  if (ix > 0 && I == ix * tx) ix--;
  if (iy > 0 && J == iy * ty) iy--;
  const int rank = iy * px + ix, i = I - ix * tx, j = J - iy * ty;
  if (rank_out) *rank_out = rank;
  return rank * ntile_piece_count(N, px, py, k, nl) + ((long)l * (ty + 1) + j) * (tx + 1) + i;
}

// ---- cell fields on tiles (the wavelet pyramids of the noise and of the scale filter; tools/node_cell_tile_host_check.cpp).
// Level k of a cell pyramid has n_k = N >> k cells a side, down to the 1-cell root.  A cell belongs to exactly one tile: the tile of
// ntile_level(.., k) holds the tx x ty cells [ox, ox + tx) x [oy, oy + ty), local cell (i, j) is global cell (ox + i, oy + j), nothing
// is shared.  The halo is the ring i = -1, i = tx, j = -1, j = ty: beyond a seam the neighbour's edge cell (its local tx - 1 / 0 /
// ty - 1 / 0, corners from the diagonal neighbour), beyond a wall the ghost cell of the boundary condition, which mirrors the edge
// cell.  Levels k < kg (ntile_kg) live on the tiles, with >= 2 cells a side and an even origin; levels k >= kg on every rank.
NT_HD static inline bool ctile_origin_even(const NodeTile &t) { return !(t.ox & 1) && !(t.oy & 1); }
// where ring or interior cell (i, j), -1 <= i <= tx, -1 <= j <= ty, of the tile `rank` on level k gets its value from: the rank that
// holds the cell and its local index there.  A cell beyond a wall is the mirror image of the cell inside (the boundary condition
// gives it that cell's value or minus it), found by clamping against the GLOBAL grid
NT_HD static inline int ctile_halo_src(int N, int px, int py, int rank, int k, int i, int j, int *si, int *sj) {
  const NodeTile t = ntile_level(N, px, py, rank, k);
  const int n = N >> k;
  int I = t.ox + i, J = t.oy + j;
  I = I < 0 ? 0 : I > n - 1 ? n - 1 : I;
  J = J < 0 ? 0 : J > n - 1 ? n - 1 : J;
  const int ix = I / t.tx, iy = J / t.ty;
  *si = I - ix * t.tx; *sj = J - iy * t.ty;
  return iy * px + ix;
}
// the gather of cell level k: every rank contributes its window, [nl][ty][tx] contiguous, lined up by rank
NT_HD static inline long ctile_piece_count(int N, int px, int py, int k, int nl) { return (long)nl * ((N >> k) / px) * ((N >> k) / py); }
// position of global cell (I, J) of layer l in the gathered buffer
NT_HD static inline long ctile_gather_src(int N, int px, int py, int k, int nl, int l, int I, int J, int *rank_out = nullptr) {
  const int tx = (N >> k) / px, ty = (N >> k) / py;
  const int ix = I / tx, iy = J / ty, rank = iy * px + ix;
  if (rank_out) *rank_out = rank;
  return rank * ctile_piece_count(N, px, py, k, nl) + ((long)l * ty + (J - iy * ty)) * tx + (I - ix * tx);
}
// counter of the device noise generator for local cell (i, j) of a tile with origin (ox, oy), ring included: the index of the global
// cell, clamped against the global N (k_n_noise on one tile: sj * N + si).  A ring cell beyond a seam is the neighbour's own draw, one
// beyond a wall the Neumann copy
NT_HD static inline unsigned ctile_noise_index(int N, int ox, int oy, int i, int j) {
  int I = ox + i, J = oy + j;
  I = I < 0 ? 0 : I > N - 1 ? N - 1 : I;
  J = J < 0 ? 0 : J > N - 1 ? N - 1 : J;
  return (unsigned)J * (unsigned)N + (unsigned)I;
}

#endif
