// floats_inl.h -- arithmetic of the Lagrangian floats (msom_floats_*).  Plain C++, no HIP header: the device
// kernels (kernels_floats.hip), the host calls (msom_floats.hip) and tools/floats_host_check.cpp (AddressSanitizer + UBSan) read
// the same functions; tests/floats_ref.py restates them in numpy.
//
// Cells are square, Delta = L0 / gnx, idx = gnx / L0 rounded once on the host; cell centre i sits at (i + 1/2) Delta.  A float at
// (x, y) in layer l lies in the dual cell whose corners are the centres (i0, j0) .. (i0 + 1, j0 + 1):
//     xi = x * idx - 0.5;  i0 = floor(xi);  a = xi - i0          (eta, j0, b likewise from y)
//   walls:    i0 clamped to [-1, nx - 1], j0 to [-1, ny - 1]: the one-cell ghost ring is read (psi = 0 on the wall face)
//   periodic: i0, j0 taken modulo nx, ny into [0, n - 1]; i0 + 1 may be the wrapped ghost column nx
//     P00 = F[l][j0][i0], P10 = F[l][j0][i0 + 1], P01 = F[l][j0 + 1][i0], P11 = F[l][j0 + 1][i0 + 1]
//     u = -((1 - a) * (P01 - P00) + a * (P11 - P10)) * idx
//     v =  ((1 - b) * (P10 - P00) + b * (P11 - P01)) * idx
// the exactly non-divergent velocity of the bilinear psi.  a is formed from the unclamped floor, so it lies in [0, 1] whatever x is;
// the index is clamped as a double, before the conversion to int, so no input bits can take it out of [-1, n].
#ifndef MSOM_FLOATS_INL_H
#define MSOM_FLOATS_INL_H

#include <math.h>

#ifdef __HIPCC__
#define FL_HD __host__ __device__
#else
#define FL_HD
#endif

struct FloatsGeom {
  int nx, ny;      // cells of the domain
  int periodic;    // sbc = -1: positions are kept unwrapped, indices wrap
  double idx;      // gnx / L0
  double Lx, Ly;   // L0, L0 * gny / gnx
};
// dual cell and weights of one position; ok = 0: the position is not finite (the float is lost, nothing may be read for it)
struct FloatsCell {
  int i0, j0;
  double a, b;
  int ok;
};

FL_HD static inline bool floats_finite(double x) { return x - x == 0.; }

// one axis: index of the lower corner and the weight of the upper one
FL_HD static inline bool floats_axis(double x, double idx, int n, int periodic, int *i0, double *a) {
  *i0 = 0;
  *a = 0.;
  const double xi = x * idx - 0.5;
  if (!floats_finite(xi)) return false;
  double f = floor(xi);
  *a = xi - f;
  if (periodic) {
    f = fmod(f, (double)n);   // exact; takes the sign of f
    if (f < 0.) f += (double)n;
    if (!(f >= 0.)) f = 0.;
    if (f > (double)(n - 1)) f = (double)(n - 1);
  } else {
    if (!(f >= -1.)) f = -1.;
    if (f > (double)(n - 1)) f = (double)(n - 1);
  }
  *i0 = (int)f;
  return true;
}

FL_HD static inline FloatsCell floats_locate(double x, double y, const FloatsGeom &g) {
  FloatsCell c;
  const bool okx = floats_axis(x, g.idx, g.nx, g.periodic, &c.i0, &c.a);
  const bool oky = floats_axis(y, g.idx, g.ny, g.periodic, &c.j0, &c.b);
  c.ok = okx && oky;
  return c;
}

// ---- on tiles ("On tiles").  The domain of g.nx x g.ny cells is cut into px x py tiles of tnx x tny cells; tile
// (ix, iy) has the origin (ix * tnx, iy * tny).  A float belongs to the tile that holds the lower corner of its dual cell, the ghost
// column -1 of a wall counted to the first tile: with i0 of floats_axis on the GLOBAL geometry (walls: [-1, gnx - 1], periodic:
// [0, gnx - 1]) the owner column is max(i0, 0) / tnx, rows likewise.  The owner then reads the local corners i0 - ox, i0 + 1 - ox in
// [-1, tnx]: its own cells, the wall ghost or the exchanged ghost column -- the numbers the single tile reads.
struct FloatsTiling {
  int px, py;      // tiles per side
  int ix, iy;      // this tile
  int tnx, tny;    // cells of a tile
};
FL_HD static inline int floats_owner_axis(int i0, int tn) { return (i0 > 0 ? i0 : 0) / tn; }
// the tile of a located position: column and row
FL_HD static inline void floats_owner(const FloatsCell &c, const FloatsTiling &t, int *col, int *row) {
  *col = floats_owner_axis(c.i0, t.tnx);
  *row = floats_owner_axis(c.j0, t.tny);
}
// One axis of a migration phase: the tile at `at` of `p` per side holds a float owned by `own`.  0: it stays; -1 / +1: it goes to
// the lower / upper neighbour (periodic: the wrapped one; where both are the same tile, the upper); 2: farther than a neighbour.
FL_HD static inline int floats_hop(int own, int at, int p, int periodic) {
  if (own == at) return 0;
  if (own == at + 1 || (periodic && own == (at + 1) % p)) return 1;
  if (own == at - 1 || (periodic && own == (at - 1 + p) % p)) return -1;
  return 2;
}

FL_HD static inline void floats_uv(double P00, double P10, double P01, double P11, double a, double b, double idx, double *u, double *v) {
  *u = -((1. - a) * (P01 - P00) + a * (P11 - P10)) * idx;
  *v = ((1. - b) * (P10 - P00) + b * (P11 - P01)) * idx;
}

// the bilinear value itself (msom_floats_sample)
FL_HD static inline double floats_bilinear(double P00, double P10, double P01, double P11, double a, double b) {
  return (1. - b) * ((1. - a) * P00 + a * P10) + b * ((1. - a) * P01 + a * P11);
}

// One RK2 stage of one float: (bx, by) the position the step starts from, (u, v) the velocity at the position the stage evaluates,
// h = dt / 2 (stage 1) or dt (stage 2).  On walls the result is clamped to the box.  Returns bit 0: clamped, bit 1: the result is not
// finite (both coordinates become NaN).
FL_HD static inline int floats_move(double bx, double by, double u, double v, double h, const FloatsGeom &g, double *ox, double *oy) {
  double x = bx + h * u, y = by + h * v;
  if (!floats_finite(x) || !floats_finite(y)) {
    *ox = *oy = NAN;
    return 2;
  }
  int flag = 0;
  if (!g.periodic) {
    if (x < 0.) { x = 0.; flag = 1; }
    if (x > g.Lx) { x = g.Lx; flag = 1; }
    if (y < 0.) { y = 0.; flag = 1; }
    if (y > g.Ly) { y = g.Ly; flag = 1; }
  }
  *ox = x;
  *oy = y;
  return flag;
}

// ---- on the vertex grid (msomn_floats_*, include/msomn_floats.h).  The domain [0, L0]^2 has N x N cells, vertex i
// sits at i Delta and psi lives on the vertices: the bilinear psi of a grid cell is the interpolant, no ghost ring is read and no
// - 0.5 appears.  With idx = N / L0 rounded once on the host, one axis is
//     xi = x * idx;  f = floor(xi) clamped as a double to [0, N - 1];  i0 = (int)f;  a = xi - f clamped to [0, 1]
// and the corners are Pcd = P[layer][j0 + d][i0 + c], vertices in [0, N].  a is clamped, so a float at x = L0 reads column N with weight
// exactly 1 even if L0 * idx rounds above N, and no pad column is ever read; f is clamped as a double, before the conversion to int,
// for the reason floats_axis gives.  Velocity, value and stage move are floats_uv, floats_bilinear and floats_move with
// FloatsGeom{N, N, 0, idx, L0, L0}.  What follows:
//   - a cell whose four corners hold the same P (land: psi is masked to 0 there and no psipg is set) has velocity exactly +-0: every
//     difference in floats_uv is an exact zero;
//   - along an edge on which P is constant (a domain wall, a coast edge between two land vertices) the normal velocity is exactly +-0:
//     on the edge the weight is exactly 0 (or 1), the other edge's difference is multiplied by it and the edge's own difference is 0;
//   - x * idx is one rounding, formed without contraction in both builds: the product and the strict build locate the same cell for
//     the same position.
// (contraction is switched off here because the product is also the operand of floats_finite's xi - xi: fused, that difference would be
// fma(x, idx, -xi), the rounding error of the product instead of zero, and every float with an inexact product would count as lost)
FL_HD static inline bool nfloats_axis(double x, double idx, int n, int *i0, double *a) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  *i0 = 0;
  *a = 0.;
  const double xi = x * idx;
  if (!floats_finite(xi)) return false;
  double f = floor(xi);
  if (!(f >= 0.)) f = 0.;
  if (f > (double)(n - 1)) f = (double)(n - 1);
  double w = xi - f;
  if (!(w >= 0.)) w = 0.;
  if (w > 1.) w = 1.;
  *i0 = (int)f;
  *a = w;
  return true;
}
FL_HD static inline FloatsCell nfloats_locate(double x, double y, const FloatsGeom &g) {
  FloatsCell c;
  const bool okx = nfloats_axis(x, g.idx, g.nx, &c.i0, &c.a);
  const bool oky = nfloats_axis(y, g.idx, g.ny, &c.j0, &c.b);
  c.ok = okx && oky;
  return c;
}

// ---- the vertex grid on tiles ("On tiles").  The N x N cells are cut into px x py tiles of tnx x tny cells; a
// tile HOLDS the (tnx + 1) x (tny + 1) vertices of its cells, the ones on its shared edges included (node_tile_inl.h).  A float
// belongs to the tile that holds its grid cell: with i0 of nfloats_axis on the GLOBAL geometry, in [0, N - 1], the owner column is
// i0 / tnx, rows likewise.  The owner's local corners i0 - ox, i0 + 1 - ox then lie in [0, tnx]: vertices the tile holds, so the
// gathers read no halo, and every holder of a shared vertex carries the same bits, so they read the single tile's numbers.  The
// owner line is the seam itself: xi exactly on a seam gives i0 = the seam's vertex, the first cell of the upper tile; x = L0 gives
// i0 = N - 1, the last tile, column tnx with weight exactly 1.  The domain has walls on all four sides: floats_hop with periodic = 0.
FL_HD static inline int nfloats_owner_axis(int i0, int tn, int p) {
  int o = (i0 > 0 ? i0 : 0) / tn;
  return o < p ? o : p - 1;   // i0 <= N - 1 by nfloats_axis: never taken, but the owner is a tile whatever i0 is
}
FL_HD static inline void nfloats_owner(const FloatsCell &c, const FloatsTiling &t, int *col, int *row) {
  *col = nfloats_owner_axis(c.i0, t.tnx, t.px);
  *row = nfloats_owner_axis(c.j0, t.tny, t.py);
}
// the located cell in the indices of the tile whose vertex (0, 0) is global vertex (ox, oy) and which holds (tx + 1) x (ty + 1)
// vertices; false: a corner is not a vertex the tile holds (the float is not at home: nothing may be read for it)
FL_HD static inline bool nfloats_local(FloatsCell *c, int ox, int oy, int tx, int ty) {
  c->i0 -= ox;
  c->j0 -= oy;
  return c->i0 >= 0 && c->i0 <= tx - 1 && c->j0 >= 0 && c->j0 <= ty - 1;
}

#endif
