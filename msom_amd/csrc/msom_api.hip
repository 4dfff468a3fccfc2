// msom_api.hip -- core of libmsomhip's host side: tile halo exchange, lifecycle, fields, set_const, the elliptic solver driver, the RHS
// evaluation, pystep_bfn with its loop and the predictor-corrector time loop.  These sections call each other in both directions and
// share the speculative-pass state of struct msom (msom_host.h), so they stay in one unit; the features they reach through a few
// entry functions live in msom_helm.hip, msom_diag.hip, msom_newqg.hip, msom_wavelet.hip, msom_io.hip and msom_hooks.hip.
// Kernels live in kernels_*.hip; params.in parsing and .bas IO in params.c / bas_io.c (host C).
//
// Reference call stacks restated here (file:line in the reference tree):
//   set_vars msqg/qg.h:837-925, set_const :931-1116, invertq :114-163,
//   poisson_layer msqg/poisson_layer.h:263-306, mg_solve/mg_cycle mspg/elliptic.h:43-99,145-229,
//   update_qg msqg/qg.h:609-650, advance_qg :594-606, run() of Basilisk predictor-corrector.h
//   (SURVEY App. B), pystep_bfn msqg/qg_bfn.h:21-103, its time loop msqg/qg_bfn.py:47-73 (msom_bfn_steps).
#include "msom_host.h"
#include "step_dt_inl.h"

// option rhs_resid = -1 (default): on from 2^RHS_RESID_MIN cell-layers.  RK2 step on one MI355X, off -> on: 4096^2 x 6 5.65 -> 5.28 ms,
// 2048^2 x 3 (2^23.6) 1.23 -> 1.10 ms, 512^2 x 3 (2^19.6) 0.350 -> 0.348 ms (inside the noise), 128^2 x 1 0.197 -> 0.21 ms
#define RHS_RESID_MIN 23
// option rhs_close = -1 (default): RHS_CLOSE_DEFAULT (both RK stages; first stage only with a 3-D forcing) from 2^RHS_CLOSE_MIN cell-layers,
// off below.  RK2 step on one MI355X, 0 -> 1 -> 2: 4096^2 x 6 5.50 -> 5.38 -> 5.26 ms, 2048^2 x 3 1.098 -> 1.097 -> 1.074 ms, 512^2 x 3 0.353
// all three: the finest level is not marched there and the option resolves to 0 ("The tendency pass closes the solve
// in front of it")
#define RHS_CLOSE_MIN 23
#define RHS_CLOSE_DEFAULT 2
// option march_visit_levels = -1 (default): MARCH_VISIT_LEVELS_DEFAULT on levels below the finest of at least 2^MARCH_VISIT_LEVELS_MIN
// cell-layers ("Fused visit below the finest level").  RK2 step on one MI355X, 0 -> 1: 4096^2 x 6 5.29 -> 5.10 ms (the
// 2048^2 x 6 level: 0.318 -> 0.229 ms per visit), 4096^2 x 3 2.65 -> 2.61, 4096^2 x 2 (a level of 2^23 cell-layers) 1.948 -> 1.917
#define MARCH_VISIT_LEVELS_DEFAULT 1
#define MARCH_VISIT_LEVELS_MIN 23
#define MARCH_HALO 4   // rows (= cells in x) of neighbour data a pass of up to 4 chained half-sweeps reads

static void free_agglomeration(msom *m);

extern "C" const char *msom_version(void) {
#ifdef MSOM_STRICT
  return "msomhip 0.1 (strict: -ffp-contract=off, reference expression order, bit-exact vs oracle)";
#else
  return "msomhip 0.1 (fast: FMA contraction, reciprocal multiplies)";
#endif
}

// ------------------------------------------------------------------ helpers

NatGeom make_nat(int nx, int ny) {
  NatGeom g;
  g.nx = nx; g.ny = ny;
  g.pitch = ((nx + 15) / 16) * 16 + 2 * MSOM_XP;
  g.rows = ny + 2 * MSOM_YP;
  g.ls = (size_t)g.pitch * g.rows;
  return g;
}
static SplitGeom make_split(int nx, int ny) {
  SplitGeom s;
  s.nx = nx; s.ny = ny;
  s.hk = nx / 2;
  s.hp = ((s.hk + 15) / 16) * 16 + 2 * MSOM_SP;
  s.rp = 2 * s.hp;
  s.rows = ny + 2;
  s.ls = (size_t)s.rp * s.rows;
  return s;
}

int sync_stream(msom *m) {
  HIPCHK(hipStreamSynchronize(m->st));
  return m->sticky;
}

// profile = 1: every slot; 2: only the chained smoother passes (the dominant kernel of the bench line) -- an event pair costs
// ~10 us of stream time, 1.4 % of a 4096^2 x 6 step and 20 % of a 512^2 x 3 step with every slot on
static bool prof_on(const msom *m, const ProfSlot &ps) {
  if (m->profile == 2) return &ps == &m->prof_march_corr || &ps == &m->prof_march_visit || (&ps >= &m->prof_march[0] && &ps <= &m->prof_march[4]);
  return m->profile != 0;
}
void prof_begin(msom *m, ProfSlot &ps, hipStream_t st) { prof_slot_begin(ps, st ? st : m->st, prof_on(m, ps)); }
void prof_end(msom *m, ProfSlot &ps, hipStream_t st) { prof_slot_end(ps, st ? st : m->st, prof_on(m, ps)); }
void prof_collect(msom *m, ProfSlot &ps) { prof_slot_collect(ps, m->st); }

static double wall_seconds() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
static int is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }


// ------------------------------------------------------------------ tile halo exchange / reductions

static const int OPP[8] = {DIR_E, DIR_W, DIR_N, DIR_S, DIR_NE, DIR_NW, DIR_SE, DIR_SW};
// both ends of a neighbour pair label their message with the same axis id
// a message is labelled with the direction it travels in (the sender's); the receiving end of direction d pairs with the peer's
// message of direction OPP[d] (comm.hip).  On a periodic tiling with 1 or 2 tiles per side both neighbours of an axis are the
// same rank (or the tile itself): the direction tells the two messages apart.
#define AXIS(dir) (dir)

// communication stream <-> compute stream ordering (tiled runs)
// comm_hold: the caller has opened the window itself (comm_begin), queues independent kernels on the compute stream while
// the exchanges it calls run on the communication stream, and closes it (comm_end) before the kernels that need the halos
void comm_begin(msom *m) {  // st2 continues after everything queued on st so far
  if (m->comm_hold) return;
  hipEventRecord(m->ev_c2x, m->st);
  hipStreamWaitEvent(m->st2, m->ev_c2x, 0);
}
void comm_end(msom *m) {    // st continues after everything queued on st2 so far
  if (m->comm_hold) return;
  hipEventRecord(m->ev_x2c, m->st2);
  hipStreamWaitEvent(m->st, m->ev_x2c, 0);
}

// all-reduce n device scalars starting at `slot` over the tiles; result in h_scal (and d_scal)
int reduce_scal(msom *m, int slot, int n, int op) {
  if (m->nranks > 1) {
    comm_begin(m);
    const int r = comm_allreduce(m->comm, m->d_scal + slot, m->h_scal + slot, n, op);
    comm_end(m);
    return r;
  }
  if (m->dbg_nosync) return MSOM_OK;   // timing experiment: the host keeps the numbers of the last real read (results meaningless)
  HIPCHK(hipMemcpyAsync(m->h_scal + slot, m->d_scal + slot, n * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

// every message of an exchange must fit the per-direction staging buffers of the communicator
static bool fits_comm(msom *m, size_t count) {
  if (count <= comm_bufcount(m->comm)) return true;
  msom_set_error("halo message of %zu doubles exceeds the communication buffers (%zu)", count, comm_bufcount(m->comm));
  return false;
}

// halo exchange of a natural field, `depth` ghost columns/rows, corners included: two phases
// (x, then y over the x-ghost columns) with the wall BCs applied in between, exactly the
// order of Basilisk's boundary() (x direction first).
static int exch_nat(msom *m, double *f, int nl, int bc, int depth) { return exch_nat_g(m, f, m->g, nl, bc, depth); }
// the same on any level of a natural-layout pyramid of the tile (wavelet filter)
int exch_nat_g(msom *m, double *f, const NatGeom &g, int nl, int bc, int depth) {
  const int d = depth;
  if (m->nranks > 1 && !fits_comm(m, (size_t)d * ((g.nx > g.ny ? g.nx : g.ny) + 2 * d) * nl)) return MSOM_ERR_ARG;
  hipStream_t cs = m->nranks > 1 ? m->st2 : m->st;  // packs, wall BCs and unpacks ride on the communication stream
  if (m->nranks > 1) comm_begin(m);
  if (m->nranks > 1) {
    Xfer x[2];
    int n = 0;
    for (int dir : {DIR_W, DIR_E}) {
      if (m->nb[dir] < 0) continue;
      launch_nat_pack_strip(cs, f, g, nl, dir == DIR_W ? 0 : g.nx - d, 0, d, g.ny, comm_sendbuf(m->comm, dir));
      x[n++] = {m->nb[dir], AXIS(dir), comm_sendbuf(m->comm, dir), comm_recvbuf(m->comm, dir), (size_t)d * g.ny * nl};
    }
    int r = comm_exchange(m->comm, x, n);
    if (r) { comm_end(m); return r; }
    for (int dir : {DIR_W, DIR_E}) {
      if (m->nb[dir] < 0) continue;
      launch_nat_unpack_strip(cs, f, g, nl, dir == DIR_W ? -d : g.nx, 0, d, g.ny, comm_recvbuf(m->comm, dir));
    }
  }
  launch_fill_ghost(cs, f, g, nl, bc, m->walls, d);
  if (m->nranks > 1) {
    Xfer x[2];
    int n = 0;
    const int w = g.nx + 2 * d;
    for (int dir : {DIR_S, DIR_N}) {
      if (m->nb[dir] < 0) continue;
      launch_nat_pack_strip(cs, f, g, nl, -d, dir == DIR_S ? 0 : g.ny - d, w, d, comm_sendbuf(m->comm, dir));
      x[n++] = {m->nb[dir], AXIS(dir), comm_sendbuf(m->comm, dir), comm_recvbuf(m->comm, dir), (size_t)d * w * nl};
    }
    int r = comm_exchange(m->comm, x, n);
    if (r) { comm_end(m); return r; }
    for (int dir : {DIR_S, DIR_N}) {
      if (m->nb[dir] < 0) continue;
      launch_nat_unpack_strip(cs, f, g, nl, -d, dir == DIR_S ? -d : g.ny, w, d, comm_recvbuf(m->comm, dir));
    }
  }
  if (m->nranks > 1) comm_end(m);
  return MSOM_OK;
}

// halo exchange (depth 1) of a multigrid field in split layout.  corners = 0: the 4 face
// neighbours in one phase (enough for the 5-point smoother); corners = 1: two phases so that
// the corner ghosts needed by the bilinear prolongation are valid.
// everything on the communication stream; the caller orders it against the compute stream
static int exch_split_raw(msom *m, double *f, const SplitGeom &sg, int nl, int corners) {
  hipStream_t cs = m->st2;
  if (!fits_comm(m, (size_t)nl * ((sg.nx > sg.ny ? sg.nx : sg.ny) + 2))) return MSOM_ERR_ARG;
  Xfer x[4];
  int n = 0;
  if (!corners) {  // one pack launch, one message per neighbour, one unpack launch
    double *sb[4], *rb[4];
    for (int dir : {DIR_W, DIR_E, DIR_S, DIR_N}) {
      const bool on = m->nb[dir] >= 0;
      sb[dir] = on ? comm_sendbuf(m->comm, dir) : nullptr;
      rb[dir] = on ? comm_recvbuf(m->comm, dir) : nullptr;
      if (on) x[n++] = {m->nb[dir], AXIS(dir), sb[dir], rb[dir], (size_t)nl * (dir == DIR_W || dir == DIR_E ? sg.ny : sg.nx)};
    }
    launch_split_pack_faces(cs, f, sg, nl, sb);
    int r = comm_exchange(m->comm, x, n);
    if (r) return r;
    launch_split_unpack_faces(cs, f, sg, nl, rb);
    return MSOM_OK;
  }
  auto pack = [&](int dir, int i0, int j0, int w, int h) {
    launch_split_pack_strip(cs, f, sg, nl, i0, j0, w, h, comm_sendbuf(m->comm, dir));
    x[n++] = {m->nb[dir], AXIS(dir), comm_sendbuf(m->comm, dir), comm_recvbuf(m->comm, dir), (size_t)w * h * nl};
  };
  const int x0 = -1, xw = sg.nx + 2;
  if (m->nb[DIR_W] >= 0) pack(DIR_W, 0, 0, 1, sg.ny);
  if (m->nb[DIR_E] >= 0) pack(DIR_E, sg.nx - 1, 0, 1, sg.ny);
  int r = comm_exchange(m->comm, x, n);
  if (r) return r;
  if (m->nb[DIR_W] >= 0) launch_split_unpack_strip(cs, f, sg, nl, -1, 0, 1, sg.ny, comm_recvbuf(m->comm, DIR_W));
  if (m->nb[DIR_E] >= 0) launch_split_unpack_strip(cs, f, sg, nl, sg.nx, 0, 1, sg.ny, comm_recvbuf(m->comm, DIR_E));
  launch_split_wall_corners(cs, f, sg, nl, m->walls);
  n = 0;
  if (m->nb[DIR_S] >= 0) pack(DIR_S, x0, 0, xw, 1);
  if (m->nb[DIR_N] >= 0) pack(DIR_N, x0, sg.ny - 1, xw, 1);
  if ((r = comm_exchange(m->comm, x, n))) return r;
  if (m->nb[DIR_S] >= 0) launch_split_unpack_strip(cs, f, sg, nl, x0, -1, xw, 1, comm_recvbuf(m->comm, DIR_S));
  if (m->nb[DIR_N] >= 0) launch_split_unpack_strip(cs, f, sg, nl, x0, sg.ny, xw, 1, comm_recvbuf(m->comm, DIR_N));
  launch_split_wall_corners(cs, f, sg, nl, m->walls);
  return MSOM_OK;
}
int exch_split(msom *m, double *f, const SplitGeom &sg, int nl, int corners) {
  if (m->nranks == 1) return MSOM_OK;
  comm_begin(m);
  const int r = exch_split_raw(m, f, sg, nl, corners);
  comm_end(m);
  return r;
}

// Deep halo of a split field for the chained smoother (kernels_march.hip): MARCH_HALO cells beyond the W / E tile edges
// go into the row pads of the field itself, MARCH_HALO rows beyond the S / N edges into the halo arrays fs / fn
// (geometry hg: MARCH_HALO rows of the level).  Two phases, the second one carries the freshly received pad columns,
// so the corner regions arrive too.  Edges without a neighbour (walls) are left alone.
static int exch_split_deep(msom *m, double *f, const SplitGeom &sg, double *fs, double *fn, const SplitGeom &hg, int nl) {
  hipStream_t cs = m->st2;
  const int H = MARCH_HALO;
  Xfer x[2];
  int n = 0;
  if (!fits_comm(m, (size_t)H * ((sg.nx > sg.ny ? sg.nx : sg.ny) + 2 * H) * nl)) return MSOM_ERR_ARG;
  comm_begin(m);
  auto pack = [&](int dir, int i0, int j0, int w, int h) {
    launch_split_pack_strip(cs, f, sg, nl, i0, j0, w, h, comm_sendbuf(m->comm, dir));
    x[n++] = {m->nb[dir], AXIS(dir), comm_sendbuf(m->comm, dir), comm_recvbuf(m->comm, dir), (size_t)w * h * nl};
  };
  // rows -1 and ny ride along: next to a y wall they are the neighbour's wall ghosts, which the cells of the halo
  // columns read like any other row
  if (m->nb[DIR_W] >= 0) pack(DIR_W, 0, -1, H, sg.ny + 2);
  if (m->nb[DIR_E] >= 0) pack(DIR_E, sg.nx - H, -1, H, sg.ny + 2);
  int r = comm_exchange(m->comm, x, n);
  if (r) { comm_end(m); return r; }   // the compute stream is re-ordered after the communication stream on every exit
  if (m->nb[DIR_W] >= 0) launch_split_unpack_strip(cs, f, sg, nl, -H, -1, H, sg.ny + 2, comm_recvbuf(m->comm, DIR_W));
  if (m->nb[DIR_E] >= 0) launch_split_unpack_strip(cs, f, sg, nl, sg.nx, -1, H, sg.ny + 2, comm_recvbuf(m->comm, DIR_E));
  n = 0;
  const int x0 = -H, xw = sg.nx + 2 * H;
  if (m->nb[DIR_S] >= 0) pack(DIR_S, x0, 0, xw, H);
  if (m->nb[DIR_N] >= 0) pack(DIR_N, x0, sg.ny - H, xw, H);
  if ((r = comm_exchange(m->comm, x, n))) { comm_end(m); return r; }
  if (m->nb[DIR_S] >= 0) launch_split_unpack_strip(cs, fs, hg, nl, x0, 0, xw, H, comm_recvbuf(m->comm, DIR_S));
  if (m->nb[DIR_N] >= 0) launch_split_unpack_strip(cs, fn, hg, nl, x0, 0, xw, H, comm_recvbuf(m->comm, DIR_N));
  comm_end(m);
  return MSOM_OK;
}

// ------------------------------------------------------------------ lifecycle

static int alloc_all(msom *m) {
  HIPCHK(hipStreamCreate(&m->st));
  HIPCHK(hipHostMalloc(&m->h_pub, (SC_COUNT + 1) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
  memset(m->h_pub, 0, (SC_COUNT + 1) * sizeof(double));
  HIPCHK(hipHostGetDevicePointer((void **)&m->d_pub, m->h_pub, 0));
  if (m->nranks > 1) {
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&m->st2, hipStreamNonBlocking, hi));
    HIPCHK(hipEventCreateWithFlags(&m->ev_c2x, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_x2c, hipEventDisableTiming));
  }
  m->g = make_nat(m->nx, m->ny);
  for (int k = 0; k < MSOM_NFIELDS; k++) {
    m->f[k] = nullptr;
    m->flayers[k] = m->nl;
    m->fbc[k] = m->bc;
  }
  m->flayers[MSOM_FR] = m->flayers[MSOM_S] = m->nlm;
  m->flayers[MSOM_RO] = m->flayers[MSOM_TOPO] = 1;
  m->fbc[MSOM_FR] = m->fbc[MSOM_S] = m->fbc[MSOM_RO] = m->fbc[MSOM_TOPO] = m->bc == BC_PERIODIC ? BC_PERIODIC : BC_NEUMANN;
  if (m->bc == BC_PERIODIC) m->fbc[MSOM_PSIPG] = BC_DIRICHLET_LIN;  // msqg/qg.h:1105-1114
  for (int k = MSOM_PTR; k <= MSOM_PTR_PRED; k++) {  // passive tracers: Neumann / periodic (msqg/qg.h:867-870)
    m->flayers[k] = m->nl * (m->p.nptr > 0 ? m->p.nptr : 1);
    m->fbc[k] = m->bc == BC_PERIODIC ? BC_PERIODIC : BC_NEUMANN;
  }
  m->flayers[MSOM_RD] = 1;
  m->fbc[MSOM_RD] = m->bc == BC_PERIODIC ? BC_PERIODIC : BC_NEUMANN;
  for (int k = 0; k < MSOM_NFIELDS; k++) {
    if (k == MSOM_NOISE || k == MSOM_SIGMA || k == MSOM_QOF || k >= MSOM_DE_BF) continue;  // allocated when "stochastic" is switched on / on the first filter call
    if (k >= MSOM_PTR && k <= MSOM_PTR_PRED && m->p.nptr <= 0) continue;
    if (m->model && !nq_has_field(k)) continue;   // newqg dialect: its six fields, every other id stays unallocated (MSOM_ERR_ARG)
    size_t bytes = m->g.ls * m->flayers[k] * sizeof(double);
    HIPCHK(hipMalloc(&m->f[k], bytes));
    HIPCHK(hipMemsetAsync(m->f[k], 0, bytes, m->st));
  }
  // multigrid levels: minlevel = 1 (msqg/poisson_layer.h:296-297) -> coarsest tile has 2 cells
  // on its short side
  int n = 0;
  while ((m->nx >> n) >= 2 && (m->ny >> n) >= 2 && ((m->nx >> n) << n) == m->nx && ((m->ny >> n) << n) == m->ny) n++;
  if (m->p.mglevels > 0 && m->p.mglevels < n) n = m->p.mglevels;
  m->nlev = n;
  m->sg.resize(n); m->da.resize(n); m->da_alt.resize(n); m->res.resize(n); m->S.resize(n); m->rc.resize(n);
  for (int k = 0; k < n; k++) {
    m->sg[k] = make_split(m->nx >> k, m->ny >> k);
    size_t bytes = m->sg[k].ls * m->nl * sizeof(double);
    HIPCHK(hipMalloc(&m->da[k], bytes));
    HIPCHK(hipMalloc(&m->res[k], bytes));
    HIPCHK(hipMemsetAsync(m->da[k], 0, bytes, m->st));
    HIPCHK(hipMemsetAsync(m->res[k], 0, bytes, m->st));
    if (m->model) continue;   // the Helmholtz cycle works in place and has no stretching: no second correction, no S
    HIPCHK(hipMalloc(&m->da_alt[k], bytes));
    HIPCHK(hipMemsetAsync(m->da_alt[k], 0, bytes, m->st));
    HIPCHK(hipMalloc(&m->S[k], m->sg[k].ls * m->nlm * sizeof(double)));
    HIPCHK(hipMemsetAsync(m->S[k], 0, m->sg[k].ls * m->nlm * sizeof(double), m->st));
  }
  if (!m->model) {
    HIPCHK(hipMalloc(&m->psi_alt, m->g.ls * m->nl * sizeof(double)));
    HIPCHK(hipMemsetAsync(m->psi_alt, 0, m->g.ls * m->nl * sizeof(double), m->st));
  }
  HIPCHK(hipMalloc(&m->staging, (size_t)m->nl * (m->p.nptr > 1 ? m->p.nptr : 1) * m->nx * m->ny * sizeof(double)));
  HIPCHK(hipMalloc(&m->partial, ((size_t)partial_count(m->g) * m->nl + 64) * sizeof(double)));  // + chunk sums of launch_sum_final
  {  // one partial sum per workgroup of the pass: the LDS-tile kernel's grid or k_rhs_lpw's with the lowest chunks (8 rows) and one strip each
    const size_t lpw = (size_t)((m->g.nx + 57) / 58) * ((m->g.ny + 7) / 8), pipe = (size_t)rhs_pipe_blocks(m->g);
    HIPCHK(hipMalloc(&m->partial_rr, ((lpw > pipe ? lpw : pipe) + 64) * sizeof(double)));
  }
  {
    size_t nb = (size_t)rhs_fused_blocks(m->g);
    if (nb < 2048) nb = 2048;
    HIPCHK(hipMalloc(&m->partial_umax, nb * MSOM_MAXNL * sizeof(double)));
  }
  HIPCHK(hipMalloc(&m->d_scal, SC_COUNT * sizeof(double)));
  HIPCHK(hipMemsetAsync(m->d_scal, 0, SC_COUNT * sizeof(double), m->st));
  HIPCHK(hipHostMalloc(&m->h_scal, SC_COUNT * sizeof(double)));
  HIPCHK(hipMalloc(&m->d_wind, (size_t)m->ny * sizeof(double)));
  return MSOM_OK;
}

// set_vars, msqg/qg.h:837-925: defaults of the large-scale fields
static int set_vars(msom *m) {
  const Params &p = m->p;
  for (int l = 0; l < m->nl; l++) m->dhf[l] = p.dhu[l];
  std::vector<double> h((size_t)m->nl * m->nx * m->ny);
  const double D = p.L0 / m->gnx;
  // Fr[] = Frm[l]  (:898-902)
  for (int l = 0; l < m->nlm; l++)
    for (size_t k = 0; k < (size_t)m->nx * m->ny; k++) h[(size_t)l * m->nx * m->ny + k] = l < m->nl - 1 ? p.Frm[l] : 0.;
  int r = msom_set_field(m, MSOM_FR, h.data());
  if (r) return r;
  m->fr_uniform = 1;
  // pp[] = vpg*x - upg*y  (:904-909)
  m->have_pg = 0;
  for (int l = 0; l < m->nl; l++) {
    if (p.upg[l] != 0 || p.vpg[l] != 0) m->have_pg = 1;
    for (int j = 0; j < m->ny; j++)
      for (int i = 0; i < m->nx; i++) {
        const double x = (m->ix * m->nx + i + 0.5) * D, y = (m->iy * m->ny + j + 0.5) * D;
        h[((size_t)l * m->ny + j) * m->nx + i] = p.vpg[l] * x - p.upg[l] * y;
      }
  }
  int hp = m->have_pg;
  r = msom_set_field(m, MSOM_PSIPG, h.data());
  if (r) return r;
  m->have_pg = hp;
  // Ro[] = Rom, topo = 0  (:911-915)
  for (size_t k = 0; k < (size_t)m->nx * m->ny; k++) h[k] = p.Rom;
  r = msom_set_field(m, MSOM_RO, h.data());
  if (r) return r;
  for (size_t k = 0; k < (size_t)m->nx * m->ny; k++) h[k] = 1.;  // Rd[] = 1. (:913)
  r = msom_set_field(m, MSOM_RD, h.data());
  m->fr_uniform = 1;
  return r;
}

msom *create_common(const Params &p0, int px, int py, int rank, const void *id128, const NewqgParams *nq) {
  Params p = p0;
  if (p.Ny <= 0) p.Ny = p.N;
  msom_params_derive(&p);
  if (p.nl < 1 || p.nl > MSOM_MAXNL) {
    msom_set_error("nl = %d outside the supported range 1..%d", p.nl, MSOM_MAXNL);
    return nullptr;
  }
  if (p.N % px || p.Ny % py || !is_pow2(p.N / px) || !is_pow2(p.Ny / py) || p.N / px < 2 || p.Ny / py < 2) {
    msom_set_error("grid %d x %d on %d x %d tiles: every tile edge must be a power of two >= 2", p.N, p.Ny, px, py);
    return nullptr;
  }
  if (p.nptr < 0 || p.nptr > MSOM_MAXNL) {
    msom_set_error("nptr = %d outside 0..%d", p.nptr, MSOM_MAXNL);
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    msom_set_error("no HIP device available: libmsomhip has no CPU fallback");
    return nullptr;
  }
  msom *m = new msom();
  m->p = p;
  if (nq) { m->model = 1; m->nq = *nq; }
  m->px = px; m->py = py; m->rank = rank; m->nranks = px * py;
  m->ix = rank % px; m->iy = rank / px;
  m->gnx = p.N; m->gny = p.Ny;
  m->nx = p.N / px; m->ny = p.Ny / py;
  m->nl = p.nl; m->nlm = p.nl > 1 ? p.nl - 1 : 1;
  m->walls = 0;
  if (p.sbc == -1) {  // periodic(right); periodic(top), msqg/qg.h:842-846
    m->bc = BC_PERIODIC;
    // one tile: ghost cells are wrapped copies kept by the owning thread (WALL_PER); tiles: no walls at all, every edge is
    // an exchange with the (wrapped) neighbour
    m->walls = px * py > 1 ? 0 : WALL_PER;
  } else {
    if (m->ix == 0) m->walls |= WALL_W;
    if (m->ix == px - 1) m->walls |= WALL_E;
    if (m->iy == 0) m->walls |= WALL_S;
    if (m->iy == py - 1) m->walls |= WALL_N;
  }
  // neighbour ranks
  for (int d = 0; d < 8; d++) m->nb[d] = -1;
  {
    const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
    for (int d = 0; d < 8; d++) {
      const int jx = m->ix + dx[d], jy = m->iy + dy[d];
      if (p.sbc == -1 && px * py > 1) m->nb[d] = ((jy + py) % py) * px + (jx + px) % px;
      else if (jx >= 0 && jx < px && jy >= 0 && jy < py) m->nb[d] = jy * px + jx;
    }
  }
  if (alloc_all(m) != MSOM_OK ||
      (m->nranks > 1 && comm_create(&m->comm, rank, m->nranks, id128, m->st2,
                                    // largest message: a MARCH_HALO-deep strip of the widest exchanged field
                                    // (tracer fields carry nl * nptr layers, fill_bc exchanges them whole)
                                    (size_t)MARCH_HALO * ((m->nx > m->ny ? m->nx : m->ny) + 16) * m->nl * (p.nptr > 1 ? p.nptr : 1)) != MSOM_OK) ||
      (nq ? nq_alloc(m) : set_vars(m)) != MSOM_OK) {
    msom_destroy(m);
    return nullptr;
  }
  return m;
}

extern "C" msom_t *msom_create_str(const char *text) {
  if (!text) { msom_set_error("null params text"); return nullptr; }
  Params p;
  msom_params_defaults(&p);
  msom_params_parse_text(&p, text);
  msom *m = create_common(p, 1, 1, 0, nullptr);
  if (m) m->params_text = text;
  return m;
}
extern "C" msom_t *msom_create(const char *path) {
  const char *pp = path ? path : "params.in";
  FILE *fp = fopen(pp, "rt");
  if (!fp) {
    msom_set_error("file %s not found", pp);  // reference: message + exit(0), msqg/qg.h:735-738
    return nullptr;
  }
  std::string text;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, n);
  fclose(fp);
  return msom_create_str(text.c_str());
}

static void clear_graphs(msom *m);
extern "C" int msom_destroy(msom_t *m) {
  if (!m) return MSOM_ERR_ARG;
  if (m->st) hipStreamSynchronize(m->st);
  clear_graphs(m);
  for (int k = 0; k < MSOM_NFIELDS; k++)
    if (m->f[k]) hipFree(m->f[k]);
  for (int k = 0; k < m->nlev; k++) {
    if (m->da[k]) hipFree(m->da[k]);
    if (m->da_alt[k]) hipFree(m->da_alt[k]);
    for (auto *v : {&m->mh_da_s, &m->mh_da_n, &m->mh_res_s, &m->mh_res_n})
      if (k < v->size() && (*v)[k]) hipFree((*v)[k]);
    if (m->res[k]) hipFree(m->res[k]);
    if (m->S[k]) hipFree(m->S[k]);
  }
  free_agglomeration(m);
  for (size_t k = 0; k < m->wv_sig.size(); k++) {
    if (k == 0) { if (m->wv_gsend) hipFree(m->wv_gsend); if (m->wv_grecv) hipFree(m->wv_grecv); }
    if (k > 0 && m->wv_s[k]) hipFree(m->wv_s[k]);
    if (k > 0 && m->wv_r[k]) hipFree(m->wv_r[k]);
    if (m->wv_sig[k]) hipFree(m->wv_sig[k]);
  }
  if (m->psi_alt) hipFree(m->psi_alt);
  if (m->q_alt) hipFree(m->q_alt);
  if (m->h_pub) hipHostFree(m->h_pub);
  if (m->staging) hipFree(m->staging);
  if (m->partial) hipFree(m->partial);
  if (m->partial_rr) hipFree(m->partial_rr);
  if (m->bfn_partial) hipFree(m->bfn_partial);
  stats_drop(m);
  floats_drop(m);
  modes_drop(m);
  spec_drop(m);
  if (m->modes_dev) hipFree(m->modes_dev);
  if (m->modes_flag) hipFree(m->modes_flag);
  if (m->modes_partial) hipFree(m->modes_partial);
  for (double *p : {m->helm_pm, m->helm_qm, m->helm_scal, m->helm_partial})
    if (p) hipFree(p);
  if (m->d_cargs) hipFree(m->d_cargs);
  if (m->partial_umax) hipFree(m->partial_umax);
  if (m->d_scal) hipFree(m->d_scal);
  if (m->h_scal) hipHostFree(m->h_scal);
  if (m->d_wind) hipFree(m->d_wind);
  for (const auto &s : prof_slots(m))
    for (auto e : s.second->ev) hipEventDestroy(e);
  if (m->comm) comm_destroy(m->comm);
  if (m->ev_c2x) hipEventDestroy(m->ev_c2x);
  if (m->ev_x2c) hipEventDestroy(m->ev_x2c);
  if (m->st2) hipStreamDestroy(m->st2);
  if (m->st) hipStreamDestroy(m->st);
  delete m;
  return MSOM_OK;
}

static void free_agglomeration(msom *m);

static void clear_graphs(msom *m);
// the field of KernelOpts under an option key (its name; null: not one of them)
static int *kernel_opt(KernelOpts &o, const char *key) {
#define KOPT(f) {#f, &KernelOpts::f}
  static const struct { const char *key; int KernelOpts::*f; } keys[] = {
      KOPT(march_rows), KOPT(march_xcd), KOPT(march_flip), KOPT(march_dbg), KOPT(march_lean), KOPT(march_dma),
      KOPT(march_visit_rows), KOPT(march_visit_pairs), KOPT(march_visit_ring), KOPT(march_visit_split), KOPT(resmax_rows), KOPT(block_variant), KOPT(rhs_dbg), KOPT(lpw_dbg)};
#undef KOPT
  for (const auto &k : keys)
    if (!strcmp(key, k.key)) return &(o.*k.f);
  return nullptr;
}
extern "C" int msom_set_option(msom_t *m, const char *key, double v) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  if (!m || !key) return MSOM_ERR_ARG;
  if (m->model) return nq_set_option(m, key, v);
  clear_graphs(m);   // captured cycles hold kernel arguments by value: any option may change them
  if (!strcmp(key, "graph")) { m->use_graph = (int)v; return MSOM_OK; }
  if (!strcmp(key, "TOLERANCE")) m->p.tolerance = v;
  else if (!strcmp(key, "NITERMAX")) m->p.nitermax = (int)v;
  else if (!strcmp(key, "NITERMIN")) m->p.nitermin = (int)v;
  else if (!strcmp(key, "DT")) m->p.DT = v;
  else if (!strcmp(key, "flag_topo")) m->flag_topo = (int)v;
  else if (!strcmp(key, "quiet")) m->quiet = (int)v;
  else if (!strcmp(key, "uniform_S")) {
    m->uniform_opt = (int)v;
    if (m->const_set) return build_coefs(m);
  }
  else if (!strcmp(key, "profile")) m->profile = (int)v;
  else if (!strcmp(key, "fused")) m->fused = (int)v;
  else if (!strcmp(key, "mg_fused")) m->mg_fused = (int)v;
  else if (!strcmp(key, "march")) m->march = (int)v;
  else if (!strcmp(key, "march_min")) m->march_min = (int)v;
  else if (!strcmp(key, "march_min_tiled")) m->march_min_tiled = (int)v;
  else if (!strcmp(key, "march_partial")) m->march_partial = (int)v;
  else if (!strcmp(key, "march_prolong")) m->march_prolong = (int)v;
  else if (!strcmp(key, "march_correct")) m->march_correct = (int)v;
  else if (!strcmp(key, "march_visit")) m->march_visit = (int)v;
  else if (!strcmp(key, "march_visit_min")) m->march_visit_min = (int)v;
  else if (!strcmp(key, "march_visit_levels")) m->march_visit_levels = (int)v;
  else if (!strcmp(key, "dbg_nosync")) m->dbg_nosync = (int)v;
  else if (!strcmp(key, "async_solve")) m->async_solve = (int)v;
  else if (!strcmp(key, "step_sync")) m->step_sync = (int)v;
  else if (!strcmp(key, "march_k")) m->march_k = (int)v < 2 ? 2 : ((int)v > 4 ? 4 : (int)v);
  else if (!strcmp(key, "block_small")) m->block_small = (int)v;
  else if (!strcmp(key, "block8")) m->block8 = (int)v;
  else if (!strcmp(key, "restrict2")) m->restrict2 = (int)v;
  else if (!strcmp(key, "restrict_pyr")) m->restrict_pyr = (int)v;
  else if (!strcmp(key, "block8_max")) m->block8_max = (int)v;
  else if (!strcmp(key, "block_sweeps")) { m->block_sweeps = (int)v; if (m->const_set) return build_coefs(m); }
  else if (!strcmp(key, "mg_global_sum")) m->mg_global_sum = (int)v;
  else if (!strcmp(key, "agglomerate")) { m->agglomerate = (int)v; if (m->const_set) return build_coefs(m); }
  else if (!strcmp(key, "agg_size")) { m->agg_size = (int)v; if (m->const_set) return build_coefs(m); }
  else if (!strcmp(key, "prolong_fused")) { m->prolong_fused = (int)v; if (m->const_set) return build_coefs(m); }
  else if (!strcmp(key, "mg_coarse")) { m->mgc_opt = (int)v; if (m->const_set) return build_coefs(m); }
  else if (!strcmp(key, "mgc_pfused")) { m->mgc_pfused = (int)v; if (m->const_set) return build_coefs(m); }
  else if (!strcmp(key, "mg_coarse_dim")) { m->mgc_dim = (int)v; if (m->const_set) return build_coefs(m); }
  else if (int *o = kernel_opt(m->opt, key)) *o = (int)v;
  else if (!strcmp(key, "rhs_variant")) m->rhs_variant = (int)v;
  else if (!strcmp(key, "adv_fused")) m->adv_fused = (int)v;
  else if (!strcmp(key, "overlap")) m->overlap = (int)v;
  else if (!strcmp(key, "rhs_resid")) { m->rhs_resid = (int)v; m->res_ready = -1; }
  else if (!strcmp(key, "rhs_close")) {
    if ((int)v < -1 || (int)v > 2) { msom_set_error("option rhs_close = %g (-1, 0, 1 or 2)", v); return MSOM_ERR_ARG; }
    m->rhs_close = (int)v; m->res_ready = -1;
  }
  else if (!strcmp(key, "seed")) { m->seed = (unsigned)v; srand(m->seed); }
  else if (!strcmp(key, "noise_mode")) m->noise_mode = (int)v;
  else if (!strcmp(key, "stoch_fused")) m->stoch_fused = (int)v;
  else if (!strcmp(key, "stats")) {
    if ((int)v && !m->stats_mask) { msom_set_error("option stats = 1 before msom_stats_begin"); return MSOM_ERR_STATE; }
    m->stats_on = (int)v != 0;
  }
  else if (!strcmp(key, "stats_every")) {
    if (!(v >= 1)) { msom_set_error("option stats_every = %g", v); return MSOM_ERR_ARG; }
    m->stats_every = (int)v;
  }
  else if (!strncmp(key, "floats", 6)) return fh::set_option(m->floats, key, v);   // floats, floats_tiles, floats_msg_cap (msom_floats.h)
  else if (!strcmp(key, "ckpt_steps")) {   // msom_run: <workdir>/state.msom every that many steps (msom_state.h); 0: off
    if (!(v >= 0)) { msom_set_error("option ckpt_steps = %g", v); return MSOM_ERR_ARG; }
    m->ckpt_steps = (int)v;
  }
  else if (!strcmp(key, "resume")) m->resume = (int)v != 0;   // msom_run: continue from <workdir>/state.msom if it is there
  else if (!strcmp(key, "tau_f")) {
    if (!(v > 0) || !std::isfinite(v)) { msom_set_error("option tau_f = %g", v); return MSOM_ERR_ARG; }
    m->tau_f = v;
  }
  else if (!strcmp(key, "modes_compact")) {
    if ((int)v != -1 && (int)v != 0) { msom_set_error("option modes_compact = %g (-1 or 0)", v); return MSOM_ERR_ARG; }
    m->modes_compact_opt = (int)v;
  }
  else if (!strcmp(key, "mode_pv_invert")) {
    if ((int)v != 0 && (int)v != 1) { msom_set_error("option mode_pv_invert = %g (0 or 1)", v); return MSOM_ERR_ARG; }
    if ((int)v && m->nranks > 1) {
      msom_set_error("option mode_pv_invert: the modal inversion runs on a single tile, this handle is one of %d", m->nranks);
      return MSOM_ERR_CONFIG;
    }
    m->mode_pv_invert = (int)v;
    m->res_ready = -1;
  }
  else if (!strcmp(key, "stochastic")) {
    m->stochastic = (int)v;
    if (m->stochastic && !m->f[MSOM_NOISE]) {
      for (int k : {MSOM_NOISE, MSOM_SIGMA}) {
        size_t bytes = m->g.ls * m->nl * sizeof(double);
        HIPCHK(hipMalloc(&m->f[k], bytes));
        HIPCHK(hipMemsetAsync(m->f[k], 0, bytes, m->st));
      }
    }
  } else {
    msom_set_error("unknown option %s", key);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}

static int march_levels(const msom *m);
static int march_kmax(const msom *m);
static bool march_lean_fine(const msom *m);
static bool fine_visit_fused(const msom *m);
static bool level_visit_fused(const msom *m, int k);
static int level_path(const msom *m, int k);
static bool restrict2_ok(const msom *m);
static bool rhs_resid_emits(const msom *m, int want = -1);
static int rhs_close_mode(const msom *m);
extern "C" double msom_get_param(msom_t *m, const char *key) {
  if (!m || !key) return NAN;
  if (!strcmp(key, "model")) return m->model;
  if (m->model) return nq_get_param(m, key);
  const Params &p = m->p;
  if (!strcmp(key, "N") || !strcmp(key, "nx")) return m->gnx;
  if (!strcmp(key, "ny")) return m->gny;
  if (!strcmp(key, "nl")) return m->nl;
  if (!strcmp(key, "nptr")) return p.nptr;
  if (!strcmp(key, "L0")) return p.L0;
  if (!strcmp(key, "DT")) return p.DT;
  if (!strcmp(key, "iRe")) return p.iRe;
  if (!strcmp(key, "iRe4")) return p.iRe4;
  if (!strcmp(key, "CFL")) return p.CFL;
  if (!strcmp(key, "Rom")) return p.Rom;
  if (!strcmp(key, "tend")) return p.tend;
  if (!strcmp(key, "dtout")) return p.dtout;
  if (!strcmp(key, "beta")) return p.beta;
  if (!strcmp(key, "tau0")) return p.tau0;
  if (!strcmp(key, "Ekb")) return p.Ekb;
  if (!strcmp(key, "Eks")) return p.Eks;
  if (!strcmp(key, "sbc")) return p.sbc;
  if (!strcmp(key, "TOLERANCE")) return p.tolerance;
  if (!strcmp(key, "nlevels")) return m->nlev;
  if (!strcmp(key, "uniform_S")) return m->uniformS;
  if (!strcmp(key, "agg_level")) return m->agg_level;
  if (!strcmp(key, "overlap")) return m->overlap;
  if (!strcmp(key, "stats_mask")) return m->stats_mask;
  if (!strcmp(key, "stats_dev_samples")) return (double)m->stats_ndev;
  if (!strcmp(key, "stats_bytes")) {   // 8 nl ny nx per array held: the selected accumulators and qo_me
    int n = m->stats_qme ? 1 : 0;
    for (int k = 0; k < MSOM_ST_NACC; k++) n += m->stats.s[k] ? 1 : 0;
    return (double)n * m->nl * m->nx * m->ny * sizeof(double);
  }
  if (double fv; floats_param(m, key, &fv)) return fv;
  if (!strcmp(key, "mode_pv_invert")) return m->mode_pv_invert;
  if (!strcmp(key, "modes_ready")) return m->const_set && m->modes_ready;
  if (!strcmp(key, "modes_compact")) return m->const_set && m->modes_ready ? m->modes_compact : (m->modes_compact_opt != 0 && m->fr_uniform);
  if (!strcmp(key, "spec_bytes")) return (double)m->spc_bytes;   // the work arrays of msom_spec_*: 0 until the first spectrum call
  if (!strcmp(key, "spec_batch")) return m->spc_batch;
  if (!strcmp(key, "modes_bytes"))   // 8 ny nx per stored array: nl*nl + nl of them in the general form, none in the compact one
    return m->modes_md ? (double)(m->nl * m->nl + m->nl) * m->nx * m->ny * sizeof(double) : 0.;
  // which kernels the dispatch picks for this handle (bench.py names what ran from these, not from a table)
  if (!strcmp(key, "resmax_marching")) return m->uniformS && m->nl <= MSOM_FASTNL && m->g.nx >= 64 && m->g.ny >= 16 && m->opt.resmax_rows >= 0;
  // how the wall-ring chunks around the fused visit run (-1: no fused visit on this handle), as launch_relax_visit reads the option
  if (!strcmp(key, "march_visit_ring")) return !fine_visit_fused(m) ? -1 : (m->opt.march_visit_ring >= 2 ? 2 : (m->opt.march_visit_ring == 1 ? 1 : 0));
  // level k's 4 + 4 half-sweeps take k_relax_visit (level 0: march_visit); the chunk height the launch then takes there
  if (!strncmp(key, "march_visit_rows_", 17) && key[17] >= '0' && key[17] <= '9') {
    const int k = atoi(key + 17);
    return level_visit_fused(m, k) ? relax_visit_rows(m->opt, m->nl, m->sg[k], k == 0) : 0;
  }
  if (!strncmp(key, "march_visit_", 12) && key[12] >= '0' && key[12] <= '9') return level_visit_fused(m, atoi(key + 12));
  if (!strcmp(key, "march_visit_levels")) return m->march_visit_levels;
  if (const int *o = kernel_opt(m->opt, key)) return *o;   // the handle's kernel options (march_rows, march_lean, ... rhs_dbg)
  if (!strcmp(key, "rhs_resid")) return rhs_resid_emits(m);   // the tendency + advance pass emits the next solve's first residual
  if (!strcmp(key, "rhs_close")) return rhs_close_mode(m);    // ... and closes the solve in front of it: 0 no, 1 first RK stage, 2 both
  if (!strncmp(key, "split_ls_", 9)) { const int k = atoi(key + 9); return k >= 0 && k < m->nlev ? (double)m->sg[k].ls : NAN; }
  if (!strncmp(key, "split_rp_", 9)) { const int k = atoi(key + 9); return k >= 0 && k < m->nlev ? (double)m->sg[k].rp : NAN; }   // doubles per row
  if (!strcmp(key, "split_pad")) return MSOM_SP;   // pad doubles on each side of a half row of a split field
  if (!strcmp(key, "restrict2")) return restrict2_ok(m);   // the pre-cycle residual pass restricts two levels down
  if (!strcmp(key, "mg_coarse_lean")) return m->mgc_first >= 0 && m->mgc_lean;   // the coarse group runs in k_mg_coarse_lean
  if (!strcmp(key, "march_levels")) return march_levels(m);   // tile levels whose half-sweeps are chained (kernels_march.hip)
  if (!strcmp(key, "march_min")) return m->march_min;   // log2 of the cell-layers a single-tile level needs for the chained pass
  if (!strcmp(key, "march_kmax")) return march_kmax(m);   // half-sweeps per marching pass that relax_sweeps allows
  if (!strcmp(key, "march_lean_fine")) return march_lean_fine(m);   // the finest level's interior chunks take the lean body
  if (!strcmp(key, "march_visit")) return fine_visit_fused(m);   // the finest level's 4 + 4 half-sweeps with the correction take k_relax_visit
  if (!strncmp(key, "relax_path_", 11)) { const int k = atoi(key + 11); return k >= 0 && k < m->nlev ? level_path(m, k) : NAN; }   // RP_*
  if (!strcmp(key, "split_ls")) return m->nlev > 0 ? (double)m->sg[0].ls : NAN;   // doubles per layer of the finest split field
  auto idx = [](const char *s, int n) { const int k = atoi(s); return k >= 0 && k < n ? k : -1; };
  if (!strncmp(key, "idh0_", 5)) { const int k = idx(key + 5, MSOM_MAXNL); return k < 0 ? NAN : m->lc.idh0[k]; }
  if (!strncmp(key, "idh1_", 5)) { const int k = idx(key + 5, MSOM_MAXNL); return k < 0 ? NAN : m->lc.idh1[k]; }
  if (!strncmp(key, "Fr_", 3)) { const int k = idx(key + 3, MSOM_MAXARR); return k < 0 ? NAN : p.Frm[k]; }
  if (!strncmp(key, "dh_", 3)) { const int k = idx(key + 3, MSOM_MAXARR); return k < 0 ? NAN : m->dhf[k]; }
  return NAN;
}

// ------------------------------------------------------------------ fields

int check_field(msom *m, int field) {
  if (!m || field < 0 || field >= MSOM_NFIELDS || !m->f[field]) {
    msom_set_error("bad field id %d", field);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}

// boundary(): wall BCs + halo exchange with the neighbour tiles.  The ghosts of q, dq and the
// predictor are never read (b enters the solver at cell centres only), so those fields skip
// the exchange; so do the arrays of the nudging loop (tendency history, observations, gain: read at cell centres only).
int fill_bc(msom *m, int field) {
  if (m->nranks > 1 && field != MSOM_Q && field != MSOM_DQ && field != MSOM_QPRED && field != MSOM_NOISE && field != MSOM_SIGMA &&
      !(field >= MSOM_BFN_F1 && field <= MSOM_BFN_GAIN)) {
    int r = exch_nat(m, m->f[field], m->flayers[field], m->fbc[field], 1);
    if (!r && m->fbc[field] == BC_DIRICHLET_LIN) {  // the wrapped ghosts on the domain edges give way to dirichlet(vpg x - upg y)
      const int sides = (m->ix == 0 ? WALL_W : 0) | (m->ix == m->px - 1 ? WALL_E : 0) | (m->iy == 0 ? WALL_S : 0) | (m->iy == m->py - 1 ? WALL_N : 0);
      launch_fill_lin_dirichlet(m->st, m->f[field], m->g, m->flayers[field], m->p.upg, m->p.vpg, m->p.L0 / m->gnx, m->p.L0,
                                m->p.L0 * m->gny / m->gnx, m->ix * m->nx, m->iy * m->ny, sides);
    }
    return r;
  }
  if (m->fbc[field] == BC_PERIODIC) launch_fill_periodic(m->st, m->f[field], m->g, m->flayers[field], 1);
  else if (m->fbc[field] == BC_DIRICHLET_LIN)
    launch_fill_lin_dirichlet(m->st, m->f[field], m->g, m->flayers[field], m->p.upg, m->p.vpg, m->p.L0 / m->gnx, m->p.L0,
                              m->p.L0 * m->gny / m->gnx);
  else launch_fill_ghost(m->st, m->f[field], m->g, m->flayers[field], m->fbc[field], m->walls);
  return MSOM_OK;
}

// host or device pointer -> natural field (+ boundary())
int upload(msom *m, int field, const double *a) {
  m->res_ready = -1;
  const size_t n = (size_t)m->flayers[field] * m->nx * m->ny;
  HIPCHK(hipMemcpyAsync(m->staging, a, n * sizeof(double), hipMemcpyDefault, m->st));
  launch_pack(m->st, m->staging, m->f[field], m->g, m->flayers[field]);
  fill_bc(m, field);
  return MSOM_OK;
}
int download(msom *m, int field, double *a) {
  const size_t n = (size_t)m->flayers[field] * m->nx * m->ny;
  launch_unpack(m->st, m->f[field], m->staging, m->g, m->flayers[field]);
  HIPCHK(hipMemcpyAsync(a, m->staging, n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

extern "C" int msom_field_layers(msom_t *m, int field) {
  if (m && m->model && !(field >= 0 && field < MSOM_NFIELDS && m->f[field])) return 0;
  if (check_field(m, field)) return MSOM_ERR_ARG;
  return m->flayers[field];
}

int ensure_field(msom *m, int field) {
  if (m->f[field]) return MSOM_OK;
  const size_t bytes = m->g.ls * m->flayers[field] * sizeof(double);
  HIPCHK(hipMalloc(&m->f[field], bytes));
  HIPCHK(hipMemsetAsync(m->f[field], 0, bytes, m->st));
  return MSOM_OK;
}
extern "C" int msom_set_field(msom_t *m, int field, const double *a) {
  if (m && !m->model && (field == MSOM_QOF || (field >= MSOM_DE_BF && field < MSOM_NFIELDS)) && ensure_field(m, field)) return MSOM_ERR_HIP;
  if (check_field(m, field) || !a) return MSOM_ERR_ARG;
  int r = upload(m, field, a);
  if (r) return r;
  if (m->model && (r = nq_after_upload(m, field))) return r;
  if (field == MSOM_RD) m->wv_ready = 0;
  if (field == MSOM_FR || field == MSOM_RO || field == MSOM_S) { m->fr_uniform = 0; m->const_set = 0; }
  // the background flow feeds values cached by msom_set_const (max |u_pg| of the dt limiter, zeta_pg when flsrv = 1;
  // the reference recomputes them on every step, msqg/qg.h:383-391): a new psi_pg needs a new set_const
  if (field == MSOM_PSIPG) { m->have_pg = 1; m->const_set = 0; }
  if (field == MSOM_ZETAPG) m->have_zpg = 1;
  if (field == MSOM_QFORC) m->have_qforc = 1;
  if (field == MSOM_TOPO) m->flag_topo = 1;
  if (field == MSOM_BFN_OBS) m->bfn_obs_set = 1;
  if (field == MSOM_BFN_GAIN) m->bfn_gain_set = 1;
  return sync_stream(m);
}
extern "C" int msom_get_field(msom_t *m, int field, double *a) {
  if (m && !m->model && (field == MSOM_QOF || (field >= MSOM_DE_BF && field < MSOM_NFIELDS)) && ensure_field(m, field)) return MSOM_ERR_HIP;
  if (check_field(m, field) || !a) return MSOM_ERR_ARG;
  return download(m, field, a);
}

// msqg/qg.c:65-70: po[] -= s.sum/s.volume per layer
extern "C" int msom_remove_mean(msom_t *m, int field) {
  MSQG_ONLY(m);
  if (check_field(m, field)) return MSOM_ERR_ARG;
  const int nl = m->flayers[field];
  m->res_ready = -1;
#ifdef MSOM_STRICT
  // validation build, one tile: the mean as the oracle forms it -- the cells column by column (x outer, y inner), each times Delta^2,
  // over the volume summed the same way (the statsf of msqg/qg.c:65-70 run serially) -- so that the field keeps the oracle's bits
  // through the steps that follow; the parallel sum below differs from it in the last place.  An initialisation call: one download
  std::vector<double> mean(nl);
  if (m->nranks == 1) {
    std::vector<double> h((size_t)nl * m->nx * m->ny);
    int r = download(m, field, h.data());
    if (r) return r;
    const double D2 = (m->p.L0 / m->gnx) * (m->p.L0 / m->gnx);
    for (int l = 0; l < nl; l++) {
      double sum = 0, vol = 0;
      for (int i = 0; i < m->nx; i++)
        for (int j = 0; j < m->ny; j++) { sum += h[((size_t)l * m->ny + j) * m->nx + i] * D2; vol += D2; }
      mean[l] = sum / vol;
    }
    HIPCHK(hipMemcpyAsync(m->d_scal + SC_LSUM, mean.data(), nl * sizeof(double), hipMemcpyHostToDevice, m->st));
    launch_sub_layer_const(m->st, m->f[field], m->d_scal + SC_LSUM, m->g, nl, 1.);
    fill_bc(m, field);
    return sync_stream(m);
  }
#endif
  launch_sum_layers(m->st, m->f[field], m->partial, m->d_scal + SC_LSUM, m->g, nl);
  if (m->nranks > 1) {
    int r = reduce_scal(m, SC_LSUM, nl, RED_SUM);
    if (r) return r;
  }
  launch_sub_layer_const(m->st, m->f[field], m->d_scal + SC_LSUM, m->g, nl, 1. / ((double)m->gnx * m->gny));
  fill_bc(m, field);
  return sync_stream(m);
}

// ------------------------------------------------------------------ set_const

// uniform-S Thomas factorisation of one level (msqg/poisson_layer.h:84-140 with constant S)
static void make_relax_coef(msom *m, int k) {
  RelaxCoef &rc = m->rc[k];
  memset(&rc, 0, sizeof rc);
  const int nl = m->nl;
  rc.D = m->p.L0 / (double)(m->gnx >> k);
  rc.sqD = rc.D * rc.D;
  for (int l = 0; l < nl; l++) { rc.idh0[l] = m->lc.idh0[l]; rc.idh1[l] = m->lc.idh1[l]; }
  if (nl < 2) { rc.it1[0] = 0.25; return; }   // one layer: plain Poisson relaxation, x = rhs / 4 (exact either way)
  double t0[MSOM_MAXNL], t1[MSOM_MAXNL], t2[MSOM_MAXNL];
  for (int l = 0; l < nl - 1; l++) {
    const double r = m->s_zero ? 0. : m->p.Frm[l] / m->p.Rom;
    rc.S[l] = r * r;
  }
  for (int l = 0; l < nl; l++) {
    t0[l] = l > 0 ? -rc.sqD * rc.S[l - 1] * rc.idh0[l] : 0.;
    t2[l] = l < nl - 1 ? -rc.sqD * rc.S[l] * rc.idh1[l] : 0.;
    t1[l] = -t0[l] - t2[l] + 4.;
  }
  for (int l = 1; l < nl; l++) t1[l] -= t0[l] * t2[l - 1] / t1[l - 1];
  for (int l = 0; l < nl; l++) {
    rc.t2[l] = t2[l];
    rc.w[l] = l > 0 ? t0[l] / t1[l - 1] : 0.;
    rc.it1[l] = 1. / t1[l];
  }
}

static void free_agglomeration(msom *m) {
  for (auto *v : {&m->gda, &m->gda_alt, &m->gres}) {
    for (double *p : *v)
      if (p) hipFree(p);
    v->clear();
  }
  m->gsg.clear();
  if (m->agg_send) hipFree(m->agg_send);
  if (m->agg_recv) hipFree(m->agg_recv);
  m->agg_send = m->agg_recv = nullptr;
  m->agg_level = -1;
}
static int setup_agglomeration(msom *m) {
  hipStreamSynchronize(m->st);
  free_agglomeration(m);
  if (m->nranks == 1 || !m->agglomerate || (m->nl > 1 && !m->uniformS)) return MSOM_OK;
  int kc = -1;
  for (int k = 0; k < m->nlev; k++)
    if (m->sg[k].nx <= m->agg_size && m->sg[k].ny <= m->agg_size) { kc = k; break; }
  if (kc < 0) return MSOM_OK;
  const int n = m->nlev - kc;
  m->gsg.resize(n); m->gda.assign(n, nullptr); m->gda_alt.assign(n, nullptr); m->gres.assign(n, nullptr);
  for (int q = 0; q < n; q++) {
    m->gsg[q] = make_split(m->sg[kc + q].nx * m->px, m->sg[kc + q].ny * m->py);
    const size_t bytes = m->gsg[q].ls * m->nl * sizeof(double);
    HIPCHK(hipMalloc(&m->gda[q], bytes));
    HIPCHK(hipMalloc(&m->gda_alt[q], bytes));
    HIPCHK(hipMalloc(&m->gres[q], bytes));
    HIPCHK(hipMemsetAsync(m->gda[q], 0, bytes, m->st));
    HIPCHK(hipMemsetAsync(m->gda_alt[q], 0, bytes, m->st));
    HIPCHK(hipMemsetAsync(m->gres[q], 0, bytes, m->st));
  }
  const size_t cnt = (size_t)m->nl * m->sg[kc].nx * m->sg[kc].ny;
  HIPCHK(hipMalloc(&m->agg_send, cnt * sizeof(double)));
  HIPCHK(hipMalloc(&m->agg_recv, cnt * m->nranks * sizeof(double)));
  m->agg_level = kc;
  return MSOM_OK;
}

// group of coarsest levels handled by k_mg_coarse: the gathered global levels (tiles + agglomeration) or
// this tile's own levels (single tile); levels that need halo exchanges stay on the per-kernel path
static int setup_mg_coarse(msom *m) {
  m->mgc_first = -1;
  m->mgc_lean = 0;
  if (!m->mgc_opt || m->block_sweeps || m->nlev < 1 || m->nl > MSOM_FASTNL) return MSOM_OK;
  const bool glob = m->agg_level >= 0;
  if (!glob && m->nranks > 1) return MSOM_OK;
  const int klo = glob ? m->agg_level : 0;
  int k0 = -1;
  for (int k = m->nlev - 1; k >= klo; k--) {
    const SplitGeom &g = glob ? m->gsg[k - m->agg_level] : m->sg[k];
    if (g.nx > m->mgc_dim || g.ny > m->mgc_dim) break;
    k0 = k;
  }
  if (k0 < 0 || m->nlev - k0 > MGC_MAXLEV) return MSOM_OK;
  {
    // k_mg_coarse declares a static LDS pool sized for the 160 KB of gfx950 (MGC_POOL doubles + its bookkeeping): on a
    // device that cannot give a workgroup that much the kernel cannot launch at all, so the levels keep one launch each
    int dev = 0, lds_max = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || (size_t)lds_max < mg_coarse_static_lds()) return MSOM_OK;
  }
  CoarseArgs h;
  memset(&h, 0, sizeof h);
  h.n = m->nlev - k0;
  h.walls = glob ? (m->bc == BC_PERIODIC ? WALL_PER : WALL_ALL) : m->walls;
  h.prolong_fused = m->prolong_fused && m->mgc_pfused;  // the kernel itself compiles the fused phase out from nl = 5 on (registers)
  h.lds = m->mgc_opt == 3 ? 2 : (m->mgc_opt >= 2 ? 1 : 0);
  for (int k = k0; k < m->nlev; k++) {
    CoarseLev &L = h.lev[k - k0];
    if (glob) { const int q = k - m->agg_level; L.da = m->gda[q]; L.res = m->gres[q]; L.S = nullptr; L.g = m->gsg[q]; }
    else { L.da = m->da[k]; L.res = m->res[k]; L.S = m->S[k]; L.g = m->sg[k]; }
    L.rc = m->rc[k];
  }
  // mg_coarse = 4 (default): the lean LDS form of the kernel where it exists -- uniform S or one layer, walls on every side or the
  // doubly periodic single tile (also the gathered levels of a tiled run, which are a whole domain), all levels inside the pool
  m->mgc_lean = m->mgc_opt >= 4 && (m->uniformS || m->nl == 1) && (h.walls == WALL_ALL || h.walls == WALL_PER) &&
                mg_coarse_lean_doubles(h, m->nl) <= (size_t)MGC_POOL;
  if (!m->d_cargs) HIPCHK(hipMalloc(&m->d_cargs, sizeof(CoarseArgs)));
  HIPCHK(hipMemcpyAsync(m->d_cargs, &h, sizeof h, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  m->mgc_first = k0;
  return MSOM_OK;
}

// layer metrics, Ro, S on all levels, column-solver constants, forcing profile
int build_coefs(msom *m) {
  clear_graphs(m);
  const Params &p = m->p;
  const int nl = m->nl;
  // sanity checks :990-1012 (reference: exit(0))
  for (int l = 0; l < nl; l++)
    if (m->dhf[l] == 0) {
      msom_set_error("thickness = 0: check the definition of dh in params.in");
      return MSOM_ERR_CONFIG;
    }
  if (p.Rom <= 0) {
    msom_set_error("Rom <= 0");
    return MSOM_ERR_CONFIG;
  }
  // layer metrics :1017-1027
  memset(&m->lc, 0, sizeof m->lc);
  for (int l = 0; l < nl - 1; l++) m->dhc[l] = 0.5 * (m->dhf[l] + m->dhf[l + 1]);
  if (nl > 1) {
    m->lc.idh0[0] = 0.;
    m->lc.idh1[0] = 1. / (m->dhc[0] * m->dhf[0]);
    for (int l = 1; l < nl - 1; l++) {
      m->lc.idh0[l] = 1. / (m->dhc[l - 1] * m->dhf[l]);
      m->lc.idh1[l] = 1. / (m->dhc[l] * m->dhf[l]);
    }
    m->lc.idh0[nl - 1] = 1. / (m->dhc[nl - 2] * m->dhf[nl - 1]);
    m->lc.idh1[nl - 1] = 0.;
  }
  const double D = p.L0 / m->gnx;
  // variable Rossby number :1032-1037
  if (p.varRo > 0) {
    std::vector<double> h((size_t)m->nx * m->ny);
    for (int j = 0; j < m->ny; j++) {
      const double y = (m->iy * m->ny + j + 0.5) * D;
      for (int i = 0; i < m->nx; i++) h[(size_t)j * m->nx + i] = p.Rom / (1 + p.Rom * p.beta * (y - 0.5 * p.L0));
    }
    int r = upload(m, MSOM_RO, h.data());
    if (r) return r;
    m->fr_uniform = 0;
  }
  // S = (Fr/Ro)^2 :1043-1048, then restricted to every level (hoisted out of the solve:
  // the reference redoes it on every poisson_layer call, msqg/poisson_layer.h:284)
  launch_make_S(m->st, m->f[MSOM_FR], m->f[MSOM_RO], m->f[MSOM_S], m->g, m->nlm);
  if (m->s_zero) HIPCHK(hipMemsetAsync(m->f[MSOM_S], 0, m->g.ls * m->nlm * sizeof(double), m->st));
  fill_bc(m, MSOM_S);
  launch_nat_to_split(m->st, m->f[MSOM_S], m->g, m->S[0], m->sg[0], m->nlm);
  for (int k = 1; k < m->nlev; k++) launch_restrict(m->st, m->S[k - 1], m->sg[k - 1], m->S[k], m->sg[k], m->nlm);
#ifdef MSOM_STRICT
  const int auto_uniform = 0;
#else
  const int auto_uniform = 1;
#endif
  m->uniformS = (m->uniform_opt < 0 ? auto_uniform : m->uniform_opt) && m->fr_uniform && nl > 1;
  for (int k = 0; k < m->nlev; k++) make_relax_coef(m, k);
  // coarse-level agglomeration (tiles): from the first level whose tile is <= agg_size cells
  // wide, every rank holds the whole coarse grid
  {
    int r = setup_agglomeration(m);
    if (r) return r;
    if ((r = setup_mg_coarse(m))) return r;
  }
  // surface forcing profile :451 (host libm so that it matches the CPU formulation bit for bit)
  {
    std::vector<double> w(m->ny);
    for (int j = 0; j < m->ny; j++) {
      const double y = (m->iy * m->ny + j + 0.5) * D;
      w[j] = p.tau0 / (p.Rom * m->dhf[0]) * sin(2 * M_PI * y / p.L0) * sin(M_PI * y / p.L0);
    }
    HIPCHK(hipMemcpyAsync(m->d_wind, w.data(), m->ny * sizeof(double), hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
  }
  return MSOM_OK;
}

extern "C" int msom_set_const(msom_t *m) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  if (!m) return MSOM_ERR_ARG;
  if (m->model) return nq_set_const(m);
  m->s_zero = 0;
  int rr = build_coefs(m);
  if (rr) return rr;
  m->wv_ready = 0;  // sig_filt / sig_lev are rebuilt from Rd on the next filter call (msqg/qg.h:1059-1090)
  const Params &p = m->p;
  const int nl = m->nl;
  const double D = p.L0 / m->gnx;
  // q = comp_q(psi) :1092
  launch_del2(m->st, m->f[MSOM_PSI], m->f[MSOM_Q], m->g, nl, 0., 1., D);
  launch_stretch(m->st, m->f[MSOM_PSI], m->f[MSOM_Q], m->f[MSOM_S], m->g, nl, 1., 1., m->lc);
  fill_bc(m, MSOM_Q);
  // large-scale relative vorticity :1094-1097
  if (p.flsrv == 1) {
    launch_del2(m->st, m->f[MSOM_PSIPG], m->f[MSOM_ZETAPG], m->g, nl, 0., 1., D);
    fill_bc(m, MSOM_ZETAPG);
    m->have_zpg = 1;
  }
  // max |u| of the large-scale flow is constant in time: cache it for the dt limiter
  for (int l = 0; l < MSOM_MAXNL; l++) m->umax_pg[l] = 0.;
  if (m->have_pg) {
    launch_umax(m->st, m->f[MSOM_PSIPG], m->partial_umax, m->d_scal + SC_UMAX, m->g, nl, D);
    int r = reduce_scal(m, SC_UMAX, nl, RED_MAX);
    if (r) return r;
    for (int l = 0; l < nl; l++) m->umax_pg[l] = m->h_scal[SC_UMAX + l];
  }
  m->const_set = 1;
  m->bfn_begun = 0;
  stats_drop(m);
  floats_drop(m);
  modes_drop(m);
  spec_drop(m);
  m->helm_solved = 0;
  if (m->helm_pm) HIPCHK(hipMemsetAsync(m->helm_pm, 0, m->g.ls * nl * sizeof(double), m->st));   // the reference's freshly created pom
  if (m->mode_pv_invert) {   // eigmod and sig_filt from mode 1, msqg/qg.h:1053-1057
    if ((rr = msom_modes_compute(m))) return rr;
    if (nl > 1 && (rr = msom_modes_set_rd(m, 1))) return rr;
  }
  return sync_stream(m);
}

// ------------------------------------------------------------------ elliptic solver

Lev tile_lev(const msom *m, int k) {   // (const handle: the functions that decide; the smoother swaps da / da_alt through the Lev)
  return Lev{const_cast<double **>(&m->da[k]), const_cast<double **>(&m->da_alt[k]), m->res[k], m->S[k], &m->sg[k], &m->rc[k], m->walls, m->nranks > 1, k == 0, k};
}
static Lev glob_lev(const msom *m, int k) {
  const int q = k - m->agg_level;
  return Lev{const_cast<double **>(&m->gda[q]), const_cast<double **>(&m->gda_alt[q]), m->gres[q], nullptr, &m->gsg[q], &m->rc[k], m->bc == BC_PERIODIC ? WALL_PER : WALL_ALL, false, false, -1};
}

// which smoother a level visit takes -- the one statement of that choice: relax_sweeps, fuse_prolong, mg_cycle, march_levels and
// msom_get_param("relax_path_<k>") all read it.  Precedence march > block8 > block2 > per-colour launches
enum { RP_COLOUR = 0, RP_BLOCK2 = 1, RP_BLOCK8 = 2, RP_MARCH = 3, RP_COARSE = 4, RP_GATHERED = 8 };
// Modal mode (option mode_pv_invert): the solve is helm_solve's, per-colour launches of k_helm_relax on every level, and what the
// layered solver fuses around its own passes does not apply.  One predicate says so.  rhs_terms asks it before it lets the tendency
// pass produce the first residual (rhs_resid) and spec_ok before the speculative tendency launch; sweep_path answers RP_COLOUR (the
// relax_path_<k> report, msom_dbg_relax); residual2 with its max|u| by-product and the marched / fused visits are never reached,
// because helm_solve does not enter mg_solve.
static bool layered_fusions(const msom *m) { return !m->mode_pv_invert; }
// option rhs_resid resolved: asked for, or (-1) the default tendency kernel on a grid big enough for the by-product to pay
static bool rhs_resid_on(const msom *m) {
  return m->rhs_resid > 0 || (m->rhs_resid < 0 && m->rhs_variant == 6 && (size_t)m->g.nx * m->g.ny * m->nl >= ((size_t)1 << RHS_RESID_MIN));
}
// the tendency kernels whose by-product has k_residual2's bits, so that the option never changes a result: k_rhs_lpw in both builds; the
// LDS-tile kernel in the validation build only (its product form carries -(lap + Gamma) psi as one reassociated number per cell, and a run
// with it does not keep the bits of the run with the option off -- tests/test_gpu_call_sequences.py, row opt_rhs_variant)
static bool rhs_resid_variant(const msom *m) {
#ifdef MSOM_STRICT
  return m->rhs_variant == 1 || m->rhs_variant == 6;
#else
  return m->rhs_variant == 6;
#endif
}
// ... and emitted by this handle's tendency + advance passes: the one statement of use_rr's terms, which rhs_terms and
// msom_get_param("rhs_resid") both read.  The fused pass with the advance riding along (never the stochastic one), k_rhs_lpw or the
// LDS-tile kernel, the layered solver's fused residual consumer on more than one level, one tile with walls and even sides
// (want: what one pass asks for, RhsPass::emit_resid -- -1 the option, 1 / 0 in its place)
static bool rhs_resid_emits(const msom *m, int want) {
  return (want < 0 ? rhs_resid_on(m) : want > 0) && m->fused && m->adv_fused && m->nl <= MSOM_FASTNL && !m->have_pg && !m->have_zpg && !m->flag_topo && !m->stochastic &&
         layered_fusions(m) && rhs_resid_variant(m) && m->mg_fused && m->nlev > 1 && m->bc != BC_PERIODIC && m->nranks == 1 &&
         !(m->g.nx & 1) && !(m->g.ny & 1);
}
static int sweep_path(const msom *m, const Lev &L) {
  const SplitGeom &g = *L.sg;
  if (!layered_fusions(m)) return RP_COLOUR;
  // chained half-sweeps in registers (k_relax_march).  One GPU (no halo exchange between half-sweeps) or tiles with deep halos,
  // walls or the doubly periodic single tile (deep halo = the field's own other side, launch_split_wrap), uniform S or one layer
  // (no vertical coupling: the column system is x = rhs / 4), and a level big enough to be HBM-bound: a marching wavefront pays one
  // memory latency per row, which only ~2000 concurrent chunks hide (measured at nl = 6: 4096^2 1.54 -> 1.05 ms per 7 half-sweeps,
  // 2048^2 385 -> 310 us, but 1024^2 105 -> 238 us).  march = 2 forces it on every level that is wide enough (tests).
  // Tiles: one level more (2^22 cell-layers: 1024^2 x 6) -- on one GPU marching that level is neutral with the round-3 body (6.69 vs
  // 6.66 ms per step at 4096^2 x 6, 1.57 vs 1.56 at 2048^2 x 3), on tiles it replaces 8 per-colour halo exchanges of a level visit
  // by 3 deep ones; unmeasured on more than one GPU (none available), so the threshold is a separate option.
  // The gathered coarse levels of a periodic tiled run keep their per-colour launches
  if (m->march && !m->block_sweeps && (m->uniformS || m->nl == 1) && m->nl <= MSOM_FASTNL && g.nx >= 512 && g.ny >= 64 &&
      (L.tiled || L.walls == WALL_ALL || (L.walls == WALL_PER && L.k >= 0)) &&
      (m->march >= 2 || (size_t)g.nx * g.ny * m->nl >= ((size_t)1 << (L.tiled ? m->march_min_tiled : m->march_min))))
    return RP_MARCH;
  // launch-bound levels (round 3): the prolongation and up to 8 colour half-sweeps of a level visit in ONE launch of the LDS-tiled
  // smoother with a halo of 8 (k_relax_block<.., 8>, option block8; levels of 64 .. block8_max cells a side that are not marched).
  // One GPU, walls or doubly periodic, nl <= 8 (the fast kernels' limit); uniform S, one layer, or a general S field (the kernel's
  // GENERAL instantiation, S of the owned cells in registers; the gathered levels of a tiled run have no S array).  Doubly periodic
  // single tile: the kernel wraps its loads; the region (<= 48 x 32 cells) must not meet its own image; the gathered coarse levels
  // of tiled runs keep their per-colour launches.  Measured at 4096^2 x 6 / 512^2 x 3: see DESIGN.md section 4
  if (m->block8 && !m->block_sweeps && (m->uniformS || m->nl == 1 || L.S) && m->nl <= MSOM_FASTNL && !L.tiled && g.nx >= 64 && g.ny >= 16 &&
      g.nx <= m->block8_max && (L.walls == WALL_ALL || (L.walls == WALL_PER && L.k >= 0 && g.ny >= 64)))
    return RP_BLOCK8;
  // the temporally blocked smoother (k_relax_block: 2 sweeps per pass; an odd last sweep takes the per-colour launches): every
  // level (option block_sweeps, which excludes the two paths above) or the levels of at most block_small cells a side
  if ((m->block_sweeps || (m->block_small && g.nx <= m->block_small)) && m->uniformS && m->nl <= MSOM_FASTNL && !L.tiled &&
      !(m->walls & WALL_PER) && g.nx >= 64 && g.ny >= 16)
    return RP_BLOCK2;
  return RP_COLOUR;
}
// the path of level k as mg_cycle_levels visits it: inside the one-launch coarse group (k_mg_coarse), on the gathered global grid
// of a tiled run (RP_GATHERED + the path there), or on this rank's tile
static int level_path(const msom *m, int k) {
  if (m->mgc_first >= 0 && k >= m->mgc_first) return RP_COARSE;
  if (m->agg_level >= 0 && k >= m->agg_level) return RP_GATHERED + sweep_path(m, glob_lev(m, k));
  return sweep_path(m, tile_lev(m, k));
}
// tile levels whose half-sweeps are chained
static int march_levels(const msom *m) {
  int n = 0;
  for (int k = 0; k < m->nlev; k++) n += level_path(m, k) == RP_MARCH;
  return n;
}
// is the finest level marched, with its interior chunks in the lean body (option march_lean, byte offsets within reach:
// march_lean_fits, as launch_relax_march decides it for the passes of the level)?
static bool march_lean_fine(const msom *m) {
  return m->nlev > 0 && m->opt.march_lean && level_path(m, 0) == RP_MARCH && march_lean_fits(m->nl, m->sg[0], &m->g);
}
// is the prolongation coarse -> L folded into the first smoothing pass of L?
static bool fuse_prolong(const msom *m, const Lev &L, int nrelax) {
  const int path = sweep_path(m, L);
  if (path == RP_BLOCK2 && nrelax >= 2) return true;
  if (path == RP_BLOCK8 && nrelax >= 1) return true;
  return m->prolong_fused && m->nl <= MSOM_FASTNL && nrelax >= 1 && L.sg->nx >= 4 && L.sg->ny >= 4;
}
// does the solve ask the last pass of the finest level for the correction (psi_alt = psi + da)?
static bool corr_wanted(const msom *m) { return m->mg_fused && m->nlev > 1 && m->march_correct; }

// half-sweeps per marching pass: march_k, but 4 register windows of 7 or 8 layers do not fit (launch_relax_march)
static int march_kmax(const msom *m) { return m->nl >= 7 && m->march_k > 3 ? 3 : m->march_k; }

// The schedule of a marched level visit, one action at a time: n half-sweeps are left, coarse != nullptr while L.da still has to
// be interpolated from it, corr_req: the solve wants the finest level's last pass to apply the correction.
//   MA_VISIT    the finest level's whole visit (prolongation + 4, 4 + correction) in k_relax_visit and the passes around it
//   MA_PL       a pass of K half-sweeps whose input is interpolated from the coarse level on the fly, so that 2 nrelax half-sweeps are
//               4 + 4 instead of (red + prolongation) + 4 + 3
//   MA_REDPROL  the red half-sweep with the prolongation (in place), where the pass cannot carry it
//   MA_PASS     a pass of K half-sweeps, out of place; corr: it applies the correction itself
//   MA_HALF     a single left-over half-sweep, in place;  MA_DONE  nothing left
// partial: more half-sweeps follow, the pass stores only the colour of its last one.  No pass leaves a single half-sweep behind
// where a shorter one avoids it (K = 4 -> 3; a plain pass also 3 -> 2)
enum { MA_DONE, MA_VISIT, MA_PL, MA_REDPROL, MA_PASS, MA_HALF };
struct MarchAct { int kind, K; bool corr, partial; };
// option march_visit_levels resolved for a level below the finest: asked for (1: wherever it applies), or (-1) the default on a level
// big enough for the fused launch to gain
static bool visit_levels_on(const msom *m, const Lev &L) {
  if (m->march_visit_levels >= 0) return m->march_visit_levels > 0;
  return MARCH_VISIT_LEVELS_DEFAULT && (size_t)L.sg->nx * L.sg->ny * m->nl >= ((size_t)1 << MARCH_VISIT_LEVELS_MIN);
}
static MarchAct march_next(const msom *m, const Lev &L, const Lev *coarse, int n, bool corr_req) {
  const int kmax = march_kmax(m), nl = m->nl;
  const bool deep = L.tiled || (L.walls & WALL_PER);   // the pass reads rows beyond the tile (relax_sweeps)
  auto pass = [&](int kind, int kmin, bool corr_ok) {
    int K = n < kmax ? n : kmax;
    if (n - K == 1 && K > kmin) K--;
    return MarchAct{kind, K, corr_ok && n == K, m->march_partial && n - K >= 1};
  };
  if (coarse && n > 0) {
    // tiles: the pass then needs MARCH_HALO cells / rows of the COARSE correction beyond the tile edges too (LDS-DMA kernel, nl <= 6)
    const bool pl_tiled = coarse->k >= 0 && nl <= 6 && m->march_prolong >= 1 && coarse->sg->nx >= 2 * MARCH_HALO && coarse->sg->ny >= 2 * MARCH_HALO;
    if (n < 3 || kmax < 3 || !m->march_prolong || (deep && !pl_tiled)) return MarchAct{MA_REDPROL, 1, false, false};
    // the fused visit: one tile with walls, uniform S, nl = 2..6, the lean body, a level wide enough for one of its chunks and
    // (march_visit = 1) big enough to gain
    if (n == 8 && kmax == 4 && L.fine && corr_req && m->march_visit && m->opt.march_dma && m->uniformS && nl >= 2 && m->march_partial &&
        (m->march_visit >= 2 || (size_t)L.sg->nx * L.sg->ny * nl >= ((size_t)1 << m->march_visit_min)) && !L.tiled && L.walls == WALL_ALL &&
        march_lean_fine(m) && relax_visit_fits(nl, *L.sg, m->opt.march_visit_rows, m->opt.march_visit_pairs))
      return MarchAct{MA_VISIT, 8, true, false};
    // ... and a marched level below the finest (option march_visit_levels): the same launch, its trailing wave storing the level's
    // correction.  The same conditions without the correction; the lean body admitted for this level's fields
    if (n == 8 && kmax == 4 && !L.fine && L.k > 0 && visit_levels_on(m, L) && m->opt.march_dma && m->uniformS && nl >= 2 && m->march_partial &&
        !L.tiled && L.walls == WALL_ALL && m->opt.march_lean && march_lean_fits(nl, *L.sg, nullptr) &&
        relax_visit_fits(nl, *L.sg, m->opt.march_visit_rows, m->opt.march_visit_pairs))
      return MarchAct{MA_VISIT, 8, false, false};
    return pass(MA_PL, 3, false);
  }
  if (n >= 2) return pass(MA_PASS, 2, corr_req && L.fine);   // the very last pass of the finest level can apply the correction (mg_solve swaps)
  return MarchAct{n == 1 ? MA_HALF : MA_DONE, n, false, false};
}
// the first action of the finest level's visit, asked the way mg_solve and level_solve ask it for nrelax = 4
// (msom_get_param("march_visit"), ("march_visit_ring"))
static bool fine_visit_fused(const msom *m) {
  if (m->nlev < 2 || level_path(m, 0) != RP_MARCH) return false;
  const Lev L = tile_lev(m, 0), C = tile_lev(m, 1);
  return march_next(m, L, fuse_prolong(m, L, 4) ? &C : nullptr, 8, corr_wanted(m)).kind == MA_VISIT;
}
// the same question for tile level k as mg_cycle_levels visits it with nrelax = 4 (msom_get_param("march_visit_<k>"))
static bool level_visit_fused(const msom *m, int k) {
  if (k == 0) return fine_visit_fused(m);
  if (k < 0 || k + 1 >= m->nlev || level_path(m, k) != RP_MARCH) return false;
  const Lev L = tile_lev(m, k), C = tile_lev(m, k + 1);
  return march_next(m, L, fuse_prolong(m, L, 4) ? &C : nullptr, 8, corr_wanted(m)).kind == MA_VISIT;
}

// does the finest level's visit of a first cycle (nrelax = 4) end in a pass that applies the correction (mg_solve then finds corr_done)?
// The same walk through march_next as relax_sweeps makes
static bool fine_corr_in_smoother(const msom *m) {
  if (m->nlev < 2 || level_path(m, 0) != RP_MARCH || !corr_wanted(m)) return false;
  const Lev L = tile_lev(m, 0), C = tile_lev(m, 1);
  const Lev *src = fuse_prolong(m, L, 4) ? &C : nullptr;
  for (int n = 8;;) {
    const MarchAct a = march_next(m, L, src, n, true);
    if (a.kind == MA_HALF || a.kind == MA_DONE) return false;
    if (a.kind == MA_VISIT || a.corr) return true;
    src = nullptr; n -= a.K;
  }
}
// option rhs_close resolved: what the speculative tendency passes of this handle do beside their own work (0: nothing, 1: the first
// stage's pass forms max|res| of the solve in front of it, 2: the second stage's too, with max|u|).  The one statement of the conditions,
// read by mg_solve and msom_get_param("rhs_close"): a speculative pass that emits the next residual (k_rhs_lpw RES), uniform S with the
// marching max-only pass (whose numbers the by-product repeats), the correction applied by the smoother's last pass
static bool spec_ok(const msom *m);
static int rhs_close_mode(const msom *m) {
  int v = m->rhs_close;
  // (default with a 3-D forcing: first stage only -- the CLS = 2 form that also reads qforc keeps 6 spilled VGPRs inside its marching loop)
  if (v < 0) v = (size_t)m->g.nx * m->g.ny * m->nl >= ((size_t)1 << RHS_CLOSE_MIN) ? (m->have_qforc ? 1 : RHS_CLOSE_DEFAULT) : 0;
  if (v <= 0) return 0;
  const bool resmax_marching = m->uniformS && m->nl <= MSOM_FASTNL && m->g.nx >= 64 && m->g.ny >= 16 && m->opt.resmax_rows >= 0;
  if (!spec_ok(m) || !rhs_resid_emits(m) || !resmax_marching || !fine_corr_in_smoother(m)) return 0;
  return v;
}

// level k's four deep-halo arrays of the chained smoother (MARCH_HALO rows each), allocated when a pass first needs them, as the
// kernels take them: those of the correction and, res, of the residual; wrap: the doubly periodic single tile is its own neighbour
static bool march_halo(msom *m, int k, bool wrap, bool res, MarchHalo *h) {
  const auto arrays = {&m->mh_da_s, &m->mh_da_n, &m->mh_res_s, &m->mh_res_n};
  if (m->mh_da_s.size() < (size_t)m->nlev)
    for (auto *v : arrays) v->assign(m->nlev, nullptr);
  const size_t ls = make_split(m->sg[k].nx, MARCH_HALO).ls, bytes = ls * m->nl * sizeof(double);
  if (!m->mh_da_s[k])
    for (auto *v : arrays) {
      if (hipMalloc(&(*v)[k], bytes) != hipSuccess) { m->sticky = MSOM_ERR_HIP; return false; }
      hipMemsetAsync((*v)[k], 0, bytes, m->st);
    }
  const bool s = wrap || m->nb[DIR_S] >= 0, n = wrap || m->nb[DIR_N] >= 0;
  *h = MarchHalo{s ? m->mh_da_s[k] : nullptr, n ? m->mh_da_n[k] : nullptr, s && res ? m->mh_res_s[k] : nullptr, n && res ? m->mh_res_n[k] : nullptr, ls, MARCH_HALO};
  return true;
}
// One marching pass.  launch(region) queues its chunks, halos() fills the deep halos it reads.  Tiles (option overlap): a pass is two
// launches -- the chunks that read nothing beyond the tile (region 1) are queued on the compute stream FIRST, the deep halo exchanges
// of the pass then run beside them on the communication stream, the chunks along the tile edges (region 2) follow once the halos
// have arrived.  Chunks are independent (out of place), so the order changes no bit
template <class Launch, class Halos>
static void march_pass(msom *m, bool overlap, ProfSlot *ps, Launch launch, Halos halos) {
  if (ps) prof_begin(m, *ps);
  if (overlap) {
    comm_begin(m); m->comm_hold = 1;
    launch(1);
    halos();
    m->comm_hold = 0; comm_end(m);
    launch(2);
  } else {
    halos();
    launch(0);
  }
  if (ps) prof_end(m, *ps);
}

// nrelax red-black relaxations of L.da against L.res (each followed by boundary_level).
// coarse != nullptr: L.da has not been prolongated yet -- the first pass interpolates it from
// the coarser level on the fly.  corners_last: the last exchange also carries corner ghosts.
// corr_req: the solve wants the finest level's last pass to apply the correction (march_next); returns whether one did -- psi + da
// then sits in psi_alt and L.da is not to be read
bool relax_sweeps(msom *m, Lev &L, const Lev *coarse, int nrelax, int corners_last, bool corr_req) {
  const bool prof = m->profile && L.fine;
  const int nl = m->nl;
  const int path = sweep_path(m, L);
  int it = 0;
  if (path == RP_MARCH) {
    // 2 nrelax half-sweeps in the actions of march_next; the passes ping-pong between the two correction buffers.
    // Tiles: a pass reads MARCH_HALO cells / rows of its neighbours (exchanged once per pass instead of once per
    // half-sweep; the cone of dependence is re-computed, bit-identically, on both sides of the edge).
    // Doubly periodic single tile: the pass sees a tile without walls whose four neighbours are the tile itself; the deep
    // halo (pads W / E, halo arrays S / N) is filled by local copies (launch_split_wrap) where tiles exchange
    const bool wrap = !L.tiled && (L.walls & WALL_PER), deep = L.tiled || wrap;
    const int kwalls = wrap ? 0 : L.walls;
    // deep halo of level k's correction (pads W / E, halo arrays S / N) and, res, of its residual
    auto fill_halo = [&](int k, bool res) {
      double *f = res ? m->res[k] : m->da[k], *fs = res ? m->mh_res_s[k] : m->mh_da_s[k], *fn = res ? m->mh_res_n[k] : m->mh_da_n[k];
      const SplitGeom hgeo = make_split(m->sg[k].nx, MARCH_HALO);
      if (L.tiled) STICKY(m, exch_split_deep(m, f, m->sg[k], fs, fn, hgeo, nl));
      else { launch_split_wrap(m->st, f, m->sg[k], fs, fn, hgeo, nl, MARCH_HALO, 0); launch_split_wrap(m->st, f, m->sg[k], fs, fn, hgeo, nl, MARCH_HALO, 1); }
    };
    MarchHalo mh{nullptr, nullptr, nullptr, nullptr, 0, MARCH_HALO}, ch = mh;
    if (deep && !march_halo(m, L.k, wrap, true, &mh)) return false;
    const bool ovl = L.tiled && m->overlap;
    bool res_halo = deep;   // the residual's deep halo is constant during the sweeps: it rides with the first pass
    const MarchCorrect mc{m->f[MSOM_PSI], m->psi_alt, m->g};
    const Lev *src = coarse;
    int n = 2 * nrelax, c = 0;
    for (;;) {
      const MarchAct a = march_next(m, L, src, n, corr_req);
      if (a.kind == MA_HALF || a.kind == MA_DONE) break;
      if (a.kind == MA_VISIT) {
        // the finest level: psi + da goes to psi_alt; a level below it: the visit leaves its correction in *L.da, ghost cells included
        // (the wall chunks around the fused ones keep the general body), where the finer level's prolongation reads it
        ProfSlot *ps = !m->profile ? nullptr : (a.corr ? &m->prof_march_visit : &m->prof_march_visit_coarse);
        if (ps) prof_begin(m, *ps);
        if (launch_relax_visit(m->st, m->opt, *L.da, *L.da_alt, L.res, *L.sg, nl, *L.rc, kwalls, *src->da, *src->sg, a.corr ? &mc : nullptr))
          m->sticky = MSOM_ERR_ARG;
        if (ps) prof_end(m, *ps);
        return a.corr;
      } else if (a.kind == MA_REDPROL) {
        if (prof) prof_begin(m, m->prof_redprol);
        launch_relax_red_prolong(m->st, m->opt, *L.da, *src->da, *src->sg, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, L.walls);
        if (prof) prof_end(m, m->prof_redprol);
      } else {
        const Lev *pl = a.kind == MA_PL ? src : nullptr;   // the pass reads the coarse level (and, deep, its halo) instead of L.da
        if (pl && deep && !march_halo(m, pl->k, wrap, false, &ch)) return false;
        march_pass(m, ovl, !prof ? nullptr : (pl ? &m->prof_march_pl : (a.corr ? &m->prof_march_corr : &m->prof_march[a.K])),
                   [&](int region) {
                     if (launch_relax_march(m->st, m->opt, pl ? nullptr : *L.da, *L.da_alt, L.res, *L.sg, nl, *L.rc, c, a.K, kwalls, m->opt.march_rows, deep ? &mh : nullptr,
                                            pl ? *pl->da : nullptr, pl ? pl->sg : nullptr, a.corr ? &mc : nullptr, a.partial, pl && deep ? &ch : nullptr, region))
                       m->sticky = MSOM_ERR_ARG;
                   },
                   [&]() {
                     if (res_halo) fill_halo(L.k, true);
                     res_halo = false;
                     if (deep) fill_halo(pl ? pl->k : L.k, false);
                   });
        if (a.corr) return true;  // da of this level was consumed in registers; nothing reads it any more
        std::swap(*L.da, *L.da_alt);
      }
      src = nullptr; n -= a.K; c = (c + a.K) & 1;
    }
    // periodic single tile: the passes wrote no ghost cell; boundary_level(da, l) = the wrapped copies, corners included
    if (wrap) launch_split_wrap(m->st, *L.da, *L.sg, nullptr, nullptr, make_split(L.sg->nx, MARCH_HALO), nl, MARCH_HALO, 2);
    if (n == 1) {
      if (L.tiled) STICKY(m, exch_split(m, *L.da, *L.sg, nl, 0));
      launch_relax_color(m->st, *L.da, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, c, L.walls, L.fine);
    }
    // boundary_level(da, l) after the last half-sweep; it also carries the corner ghosts the prolongation reads
    if (L.tiled) STICKY(m, exch_split(m, *L.da, *L.sg, nl, corners_last));
    return false;
  }
  if (path == RP_BLOCK8) {
    int n = 2 * nrelax, c = 0;
    const Lev *src = coarse;   // first pass: the correction is interpolated from the coarser level on the fly
    while (n > 0) {
      const int K = n < 8 ? n : 8;
      if (K == 1) { launch_relax_color(m->st, *L.da, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, c, L.walls, L.fine); break; }
      if (launch_relax_block8(m->st, m->opt, *L.da, src ? *src->da : nullptr, src ? *src->sg : *L.sg, L.res, *L.da_alt, *L.sg, nl, *L.rc, L.walls, K, c, m->uniformS ? nullptr : L.S)) m->sticky = MSOM_ERR_ARG;
      std::swap(*L.da, *L.da_alt);
      src = nullptr; n -= K; c = (c + K) & 1;
      // periodic: the pass stored no ghost cell; boundary_level(da, l) = the wrapped copies, corners included (a following colour
      // pass reads them, and so does the prolongation to the next finer level)
      if (L.walls & WALL_PER) launch_split_wrap(m->st, *L.da, *L.sg, nullptr, nullptr, make_split(L.sg->nx, MARCH_HALO), nl, MARCH_HALO, 2);
    }
    return false;
  }
  if (path == RP_BLOCK2) {
    for (; it + 2 <= nrelax; it += 2) {
      const bool pl = coarse && it == 0;
      if (prof && !pl) prof_begin(m, m->prof_block);
      launch_relax_block2(m->st, m->opt, *L.da, pl ? *coarse->da : nullptr, pl ? *coarse->sg : *L.sg, L.res, *L.da_alt, *L.sg, nl, *L.rc, L.walls, L.fine);
      if (prof && !pl) prof_end(m, m->prof_block);
      std::swap(*L.da, *L.da_alt);
    }
  }
  for (; it < nrelax; it++) {
    const bool pl = coarse && it == 0;  // prolongation rides in the first red half-sweep
    if (prof && !pl) prof_begin(m, m->prof_sweep);
    for (int c = 0; c < 2; c++) {
      const int corners = corners_last && it == nrelax - 1 && c == 1;
      if (L.tiled && m->overlap && !(pl && c == 0) && !corners && L.sg->nx >= 32 && L.sg->ny >= 8) {
        // the outermost ring of the tile first; its halo exchange (communication stream) then runs beside the
        // interior cells (compute stream); same per-cell arithmetic, so the result does not change
        launch_relax_ring(m->st, *L.da, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, c, L.walls);
        comm_begin(m);
        STICKY(m, exch_split_raw(m, *L.da, *L.sg, nl, 0));
        launch_relax_color(m->st, *L.da, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, c, L.walls, L.fine, 1);
        comm_end(m);
        continue;
      }
      if (pl && c == 0) {
        if (prof) prof_begin(m, m->prof_redprol);
        launch_relax_red_prolong(m->st, m->opt, *L.da, *coarse->da, *coarse->sg, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, L.walls);
        if (prof) prof_end(m, m->prof_redprol);
      } else
        launch_relax_color(m->st, *L.da, L.res, L.S, *L.sg, nl, *L.rc, m->uniformS, c, L.walls, L.fine);
      // boundary_level(da, l): the last exchange of the level also carries the corner ghosts
      // that the bilinear prolongation to the next finer level reads
      if (L.tiled) STICKY(m, exch_split(m, *L.da, *L.sg, nl, corners));
    }
    if (prof && !pl) prof_end(m, m->prof_sweep);
  }
  return false;
}

// one level of the coarse-to-fine half of mg_cycle: initial guess (zero / prolongation), then
// the relaxations (corr_req and the return value: see relax_sweeps)
static bool level_solve(msom *m, Lev &L, const Lev *coarse, int nrelax, int corners_last, bool corr_req) {
  const int nl = m->nl;
  bool fused = false;
  if (!coarse) hipMemsetAsync(*L.da, 0, L.sg->ls * nl * sizeof(double), m->st);
  else if (fuse_prolong(m, L, nrelax)) fused = true;
  else {
    launch_prolong(m->st, *coarse->da, *coarse->sg, *L.da, *L.sg, nl, L.walls);
    if (L.tiled) STICKY(m, exch_split(m, *L.da, *L.sg, nl, 0));
  }
  return relax_sweeps(m, L, fused ? coarse : nullptr, nrelax, corners_last, corr_req);
}

// coarse-to-fine part of mg_cycle, mspg/elliptic.h:53-89 (minlevel = 1): restriction of the
// residual to all levels (level 1 may already come out of the fused residual kernel), then
// prolongation + nrelax relaxations per level.  With tiles, the levels >= agg_level are solved
// on the gathered global coarse grid by every rank (identical arithmetic, no halo traffic).
// corr_req and the return value: see relax_sweeps (only the finest tile level can answer a request).
static bool mg_cycle_levels(msom *m, int nrelax, int first_restrict, bool corr_req) {
  const int nl = m->nl, kc = m->agg_level >= 0 ? m->agg_level : m->nlev;
  const int kg = m->mgc_first;  // levels >= kg (of the gathered grid if kc < nlev, else of this tile): one launch
  const bool glob = kc < m->nlev;
  // tile levels: restrict down to the gather level / to the finest level of the one-launch group
  const int rmax = glob ? kc : (kg >= 0 ? kg : m->nlev - 1);
  {
    // the chain in launches of up to 5 levels each (k_restrict_pyramid, round 3) where a tile of 2^n cells a side of the chain's finest
    // level exists on every level down; a single restriction keeps its own kernel
    int k = first_restrict;
    const int kend = rmax < m->nlev - 1 ? rmax : m->nlev - 1;
    while (k <= kend) {
      int n = kend - k + 1;
      if (n > 5) n = 5;
      const SplitGeom &fg = m->sg[k - 1];
      while (n > 1 && (fg.nx % (1 << n) || fg.ny % (1 << n))) n--;
      if (n >= 2 && m->restrict_pyr) {
        SplitGeom g[6];
        double *out[5];
        for (int q = 0; q <= n; q++) g[q] = m->sg[k - 1 + q];
        for (int q = 0; q < n; q++) out[q] = m->res[k + q];
        launch_restrict_pyramid(m->st, m->res[k - 1], out, g, n, nl);
      } else {
        n = 1;
        launch_restrict(m->st, m->res[k - 1], m->sg[k - 1], m->res[k], m->sg[k], nl);
      }
      k += n;
    }
  }
  if (glob) {
    // gather the level-kc residual of all tiles, restrict it further on the global grid
    const SplitGeom &tg = m->sg[kc];
    const size_t cnt = (size_t)nl * tg.nx * tg.ny;
    launch_split_unpack(m->st, m->res[kc], tg, m->agg_send, nl);
    comm_begin(m);
    STICKY(m, comm_allgather(m->comm, m->agg_send, m->agg_recv, cnt));
    comm_end(m);
    launch_assemble_global(m->st, m->agg_recv, m->gres[0], m->gsg[0], nl, tg.nx, tg.ny, m->px);
    const int gtop = kg >= 0 ? kg : m->nlev - 1;  // coarsest level restricted by its own launch
    for (int k = kc + 1; k <= gtop; k++) launch_restrict(m->st, m->gres[k - 1 - kc], m->gsg[k - 1 - kc], m->gres[k - kc], m->gsg[k - kc], nl);
    if (kg >= 0) {
      launch_mg_coarse(m->st, m->d_cargs, nrelax, nl, m->uniformS, m->mgc_lean);
      if (hipGetLastError() != hipSuccess && !m->sticky) m->sticky = MSOM_ERR_HIP;
    }
    for (int k = (kg >= 0 ? kg : m->nlev) - 1; k >= kc; k--) {
      Lev L = glob_lev(m, k);
      if (k == m->nlev - 1) level_solve(m, L, nullptr, nrelax, 0, false);
      else { Lev C = glob_lev(m, k + 1); level_solve(m, L, &C, nrelax, 0, false); }
    }
    // this rank's tile of the level-kc correction, with its ghost ring
    launch_extract_tile(m->st, m->gda[0], m->gsg[0], m->da[kc], tg, nl, m->ix * tg.nx, m->iy * tg.ny);
  } else if (kg >= 0) {
    launch_mg_coarse(m->st, m->d_cargs, nrelax, nl, m->uniformS, m->mgc_lean);
    if (hipGetLastError() != hipSuccess && !m->sticky) m->sticky = MSOM_ERR_HIP;
  }
  bool corr_done = false;
  for (int k = (glob ? kc : (kg >= 0 ? kg : m->nlev)) - 1; k >= 0; k--) {
    Lev L = tile_lev(m, k);
    if (k == m->nlev - 1) corr_done = level_solve(m, L, nullptr, nrelax, k > 0, corr_req);
    else { Lev C = tile_lev(m, k + 1); corr_done = level_solve(m, L, &C, nrelax, k > 0, corr_req); }
  }
  return corr_done;
}

static void clear_graphs(msom *m) {
  for (auto &kv : m->cyc_graph) (void)hipGraphExecDestroy(kv.second);
  m->cyc_graph.clear();
}
// the cycle through a captured graph where that is possible (see use_graph); same launches, same order, same arguments
// corr_req and the return value: see relax_sweeps.  A request acts inside a marching pass only and a captured cycle has none, so the
// capture is made, and replayed, without one
static bool mg_cycle(msom *m, int nrelax, int first_restrict, bool corr_req) {
  bool ok = m->use_graph && m->nranks == 1 && !m->profile;
  for (int k = 0; ok && k < m->nlev; k++) {
    Lev L = tile_lev(m, k);
    if (sweep_path(m, L) != RP_COLOUR) ok = false;   // those passes ping-pong between two buffers: pointers differ from cycle to cycle
  }
  if (!ok) return mg_cycle_levels(m, nrelax, first_restrict, corr_req);
  const long key = (long)nrelax * 8 + first_restrict;
  auto it = m->cyc_graph.find(key);
  if (it == m->cyc_graph.end()) {
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    if (hipStreamBeginCapture(m->st, hipStreamCaptureModeThreadLocal) != hipSuccess) { m->use_graph = 0; return mg_cycle_levels(m, nrelax, first_restrict, false); }
    mg_cycle_levels(m, nrelax, first_restrict, false);
    if (hipStreamEndCapture(m->st, &g) != hipSuccess || !g || hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
      if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError();
      m->use_graph = 0;                 // nothing was executed during the capture: run the cycle eagerly now
      return mg_cycle_levels(m, nrelax, first_restrict, false);
    }
    (void)hipGraphDestroy(g);
    it = m->cyc_graph.emplace(key, ex).first;
  }
  if (hipGraphLaunch(it->second, m->st) != hipSuccess && !m->sticky) m->sticky = MSOM_ERR_HIP;
  return false;
}

void residual(msom *m, const double *a, const double *b, int slot, int want_sum) {
  if (m->profile) prof_begin(m, m->prof_resid);
  launch_residual(m->st, a, b, m->f[MSOM_S], m->g, m->res[0], m->sg[0], m->nl, m->rc[0], m->uniformS, m->d_scal + slot, m->partial, want_sum);
  if (m->profile) prof_end(m, m->prof_resid);
}
// fused variants (kernels_mg.hip k_residual2); mode bits 1 = CORRECT, 2 = WRITE, 4 = RESTRICT
// the pre-cycle residual pass also restricts to level 2 (round 3: the launch of k_restrict that read the level-1 residual back, 53 us at
// 4096^2 x 6, becomes 1/16 w of extra stores): the block of 4 rows x 128 cells holds whole level-2 cells when ny % 4 == 0 and nx % 4 == 0
static bool restrict2_ok(const msom *m) { return m->restrict2 && m->mg_fused && m->nlev > 2 && m->g.ny % 4 == 0 && m->sg[0].hk % 2 == 0; }
void residual2(msom *m, int mode, const double *b, int slot, int want_sum) {
  ProfSlot &which = (mode & 8) ? m->prof_resmax : (mode & 1) ? m->prof_rescorr : m->prof_respre;
  if (m->profile) { prof_begin(m, m->prof_resid); prof_begin(m, which); }
  const bool r2 = (mode & 4) && restrict2_ok(m);
  launch_residual2(m->st, m->opt, mode, m->f[MSOM_PSI], m->da[0], m->psi_alt, b, m->f[MSOM_S], m->g, m->res[0], m->sg[0],
                   m->nlev > 1 ? m->res[1] : nullptr, m->sg[m->nlev > 1 ? 1 : 0], m->nl, m->rc[0], m->uniformS, m->walls, m->d_scal + slot,
                   m->partial, want_sum, m->partial_umax, m->d_scal + SC_UMAX, m->umax_clean, r2 ? m->res[2] : nullptr, r2 ? &m->sg[2] : nullptr);
  if (mode & (1 | 8)) m->umax_clean = 0;
  if (m->profile) { prof_end(m, m->prof_resid); prof_end(m, which); }
}

// max-residual slots (RES0, RES1) and the rhs sum (BSUM) -> host, reduced over the tiles
// (the reference's foreach(reduction(max:maxres)) / reduction(+:sum) are MPI all-reduces)
// published: k_step_dt copied the scalars to the host beside the speculative pass -- spin on its sequence word
static int read_residuals(msom *m, bool published = false) {
  if (m->nranks == 1) {
    // one copy of the whole scalar block (sums, residuals, max|u|, the device's dt) and one wait
    if (m->dbg_nosync) return MSOM_OK;
    if (published) {
      volatile long *seq = reinterpret_cast<volatile long *>(m->h_pub + SC_COUNT);
      const double t0 = wall_seconds();
      while (*seq != m->pub_seq) {
        if (wall_seconds() - t0 > 5.) {   // the device is stuck or faulted: let the runtime report it
          HIPCHK(hipStreamSynchronize(m->st));
          if (*seq != m->pub_seq) { msom_set_error("the device did not publish the solver's scalars"); return MSOM_ERR_HIP; }
        }
      }
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      memcpy(m->h_scal, m->h_pub, SC_COUNT * sizeof(double));
      return MSOM_OK;
    }
    HIPCHK(hipMemcpyAsync(m->h_scal, m->d_scal, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    return MSOM_OK;
  }
  int r = reduce_scal(m, SC_RES0, 2 + m->nl, RED_MAX);  // RES0, RES1, UMAX[nl]
  if (r) return r;
  // mgstats.sum is informational (the reference never prints it, msqg/qg.h:61): with tiles it
  // stays the local tile's sum unless "mg_global_sum" asks for the extra all-reduce
  if (m->nranks > 1 && !m->mg_global_sum) {
    HIPCHK(hipMemcpyAsync(m->h_scal + SC_BSUM, m->d_scal + SC_BSUM, sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    return MSOM_OK;
  }
  return reduce_scal(m, SC_BSUM, 1, RED_SUM);
}

// mg_solve, mspg/elliptic.h:145-229, called as poisson_layer does (msqg/poisson_layer.h:290-303)
// on a = psi (natural field with valid ghosts, warm start) and b (natural field).
// Fused path (default): the pre-cycle residual also produces the level-1 restriction, the
// correction a += da is folded into the post-cycle residual (written to a second psi buffer
// that then becomes psi), and the post-cycle pass only produces max|res|; the residual field
// is regenerated only if another cycle turns out to be needed.
// sp: the tendency pass to queue behind the first cycle, before the host knows the residual (struct SpecPass); null: none
static void spec_queue(msom *m, SpecPass *sp);
static int mg_solve(msom *m, const double *b, msom_mgstats *s, SpecPass *sp = nullptr) {
  const Params &p = m->p;
  const bool fused = m->mg_fused && m->nlev > 1;
  s->i = 0; s->nrelax = 4;
  // one fill for every accumulator of the solve: sums, max|res| before / after the first cycle, max|u| per layer
  HIPCHK(hipMemsetAsync(m->d_scal, 0, (SC_UMAX + MSOM_MAXNL) * sizeof(double), m->st));
  m->umax_clean = 1;
  m->umax_ready = 0;
  const bool have_res = fused && m->res_ready >= 0 && b == m->f[m->res_ready];
  m->res_ready = -1;
  if (have_res) {  // res[0], res[1], max|res| and the partial sums of b came out of the tendency pass
    HIPCHK(hipMemcpyAsync(m->d_scal + SC_RES0, m->d_scal + SC_RESF, sizeof(double), hipMemcpyDeviceToDevice, m->st));
    launch_sum_final(m->st, m->partial_rr, m->d_scal + SC_BSUM, m->rr_nparts);
  } else if (fused) {
    residual2(m, 2 | 4, b, SC_RES0, 1);
    launch_sum_final(m->st, m->partial, m->d_scal + SC_BSUM, residual2_blocks(m->g));
  } else {
    residual(m, m->f[MSOM_PSI], b, SC_RES0, 1);
    launch_sum_final(m->st, m->partial, m->d_scal + SC_BSUM, partial_count(m->g));
  }
  // The correction passes form the ghost values of a + da from those of a and of da, which is boundary(a + da) only while the ghosts
  // of a belong to its cells.  After pystep_de they do not (filter_de zeroes the cells of psi alone): the first residual reads them as
  // they are, as the reference's does, and the reference's boundary(a) after the correction is made here, ahead of the cycle
  // (tests/test_gpu_call_sequences.py, row pystep_de at TOLERANCE 1e-7: max|res| after the first cycle was 4.7e-5 for the oracle's 1.4e-4)
  if (m->psi_ghosts_stale) {
    m->psi_ghosts_stale = 0;
    fill_bc(m, MSOM_PSI);
  }
  bool have_first = false;
  double resb = 0;
  if (p.nitermin < 1) {  // need the initial residual before deciding on the first cycle
    int rr = read_residuals(m);
    if (rr) return rr;
    resb = s->resb = s->resa = m->h_scal[SC_RES0];
    s->sum = m->h_scal[SC_BSUM];
    have_first = true;
  }
  for (s->i = 0; s->i < p.nitermax && (s->i < p.nitermin || s->resa > p.tolerance); s->i++) {
    // restrictions still to do: from level 1 (plain path), 2 (the residual pass restricted once) or 3 (twice; not when the residual
    // came out of the tendency pass, option rhs_resid)
    const bool corr_done = mg_cycle(m, s->nrelax, fused ? ((restrict2_ok(m) && !(have_res && s->i == 0)) ? 3 : 2) : 1, corr_wanted(m));
    if (s->i > 0) HIPCHK(hipMemsetAsync(m->d_scal + SC_RES1, 0, sizeof(double), m->st));
    if (corr_done) {  // a_new = a + da already sits in psi_alt (last smoother pass): boundary(a), then max |res|, max |u|
      std::swap(m->f[MSOM_PSI], m->psi_alt);
      if (m->nranks > 1) STICKY(m, exch_nat(m, m->f[MSOM_PSI], m->nl, m->bc, 1));
      else if (m->bc == BC_PERIODIC) launch_fill_periodic(m->st, m->f[MSOM_PSI], m->g, m->nl, 1);
      else launch_fill_ghost(m->st, m->f[MSOM_PSI], m->g, m->nl, m->bc, m->walls);   // the LDS-DMA pass leaves the wall ghosts to this
      // option rhs_close: the speculative tendency pass queued below reads this psi anyway and forms max|res| (second stage: max|u|
      // too) on the side.  First stage: dt comes from max|u|, which therefore stays in front of the pass, from psi alone
      const int mode = (s->i == 0 && sp && m->nranks == 1) ? rhs_close_mode(m) : 0, cls = !mode ? 0 : (sp->stage == 1 ? 1 : (mode >= 2 ? 2 : 0));
      if (cls) { sp->pass.cls = cls; sp->pass.cls_b = b; }
      if (cls == 2) {   // the pass accumulates into the block zeroed with the solve's scalars
        if (!m->umax_clean) HIPCHK(hipMemsetAsync(m->d_scal + SC_UMAX, 0, m->nl * sizeof(double), m->st));
        m->umax_clean = 0;
      }
      else residual2(m, cls ? 8 | 16 : 8, b, SC_RES1, 0);
      m->umax_ready = 1;
    } else if (fused) {
      residual2(m, 1, b, SC_RES1, 0);            // a_new = a + da -> psi_alt, max |res(a_new)|, max |u(a_new)|
      std::swap(m->f[MSOM_PSI], m->psi_alt);
      m->umax_ready = 1;
      if (m->nranks > 1) STICKY(m, exch_nat(m, m->f[MSOM_PSI], m->nl, m->bc, 1));
    } else {
      launch_correct(m->st, m->f[MSOM_PSI], m->g, m->da[0], m->sg[0], m->nl, m->walls);
      if (m->nranks > 1) STICKY(m, exch_nat(m, m->f[MSOM_PSI], m->nl, m->bc, 1));  // boundary(a)
      residual(m, m->f[MSOM_PSI], b, SC_RES1, 0);
    }
    const bool queued = s->i == 0 && sp && m->umax_ready && m->nranks == 1;
    if (queued) spec_queue(m, sp);
    int rr = read_residuals(m, queued);
    if (rr) return rr;
    if (queued) {   // its output counts only if this solve ends here
      const double ra = m->h_scal[SC_RES1];
      sp->counts = !(s->i + 1 < p.nitermax && (s->i + 1 < p.nitermin || ra > p.tolerance));
    }
    if (!have_first) {
      resb = s->resb = m->h_scal[SC_RES0];
      s->sum = m->h_scal[SC_BSUM];
      have_first = true;
    }
    s->resa = m->h_scal[SC_RES1];
    if (s->resa > p.tolerance) {
      if (resb / s->resa < 1.2 && s->nrelax < 100) s->nrelax++;
      else if (resb / s->resa > 10 && s->nrelax > 2) s->nrelax--;
    }
    resb = s->resa;
    // another cycle follows: it needs the residual field of the corrected a on levels 0 and 1
    if (fused && s->i + 1 < p.nitermax && (s->i + 1 < p.nitermin || s->resa > p.tolerance)) residual2(m, 2 | 4, b, SC_SCRATCH, 0);
  }
  if (!have_first) {  // nitermax == 0
    int rr = read_residuals(m);
    if (rr) return rr;
    s->resb = s->resa = m->h_scal[SC_RES0];
    s->sum = m->h_scal[SC_BSUM];
  }
  if (s->resa > p.tolerance && !m->quiet)
    fprintf(stderr, "WARNING: convergence not reached after %d iterations\n  res: %g sum: %g nrelax: %d\n", s->i, s->resa, s->sum, s->nrelax);
  return MSOM_OK;
}

// invertq, msqg/qg.h:114-163 (the trailing boundary(pol) is already done by the correction)
int invertq(msom *m, const double *q, SpecPass *sp) {
  if (m->mode_pv_invert) return helm_solve(m, q);   // (spec_ok: never with a pass to queue)
  return mg_solve(m, q, &m->mg, sp);
}

// ------------------------------------------------------------------ RHS

double limiter(msom *m, double umax, double dtmax) { return step_limit(umax, dtmax, m->p.L0 / m->gnx, m->p.CFL, &m->previous); }

void comp_del2(msom *m, int in, int out, double add, double fac) {
  const double D = m->p.L0 / m->gnx;
  launch_del2(m->st, m->f[in], m->f[out], m->g, m->nl, add, fac, D);
  fill_bc(m, out);
  if (m->p.sbc > 0) launch_slip_bc(m->st, m->f[in], m->f[out], m->g, m->nl, m->p.sbc / ((0.5 * m->p.sbc + 1) * D * D), m->walls);
}
void comp_stretch(msom *m, int in, int out, double add, double fac) {
  launch_stretch(m->st, m->f[in], m->f[out], m->f[MSOM_S], m->g, m->nl, add, fac, m->lc);
  fill_bc(m, out);
}

// tendency terms after the inversion, as struct RhsPass (msom_host.h) asks for them; ps.advanced tells the caller whether the
// advance rode in the pass (fused path) or not.
static int stoch_prepare(msom *m, double dt, double *dts);
int rhs_terms(msom *m, RhsPass &ps) {
  ps.advanced = false;
  const Params &p = m->p;
  const int qfield = ps.qfield, dqfield = ps.dqfield, with_qforcing = ps.with_qforcing, adv_in = ps.adv_in;
  int adv_out = ps.adv_out;
  const double iRe = p.iRe, iRe4 = p.iRe4, Eks = p.Eks, Ekb = p.Ekb, adv_dt = ps.adv_dt;
  const double D = p.L0 / m->gnx;
  const int nl = m->nl;
  // stochastic runs (msqg/qg_stochastic.h) ride in the same kernel when the advance does: the relaxation -q/tau and the
  // noise are linear in fields that exist before the pass, so the finalisation of the pass reads them next to q_in.  The
  // validation build keeps the reference's operation order (separate kernels) instead.
#ifdef MSOM_STRICT
  const bool stoch_fused = false;
#else
  const bool stoch_fused = m->stochastic && m->stoch_fused && m->adv_fused && adv_out >= 0 && m->rhs_variant == 6;
#endif
  if (m->fused && m->nl <= MSOM_FASTNL && !m->have_pg && !m->have_zpg && !m->flag_topo && (!m->stochastic || stoch_fused) &&
      (m->nranks == 1 || (m->nx >= 4 && m->ny >= 4))) {
    // tiles: the fused kernel needs psi on a 3-cell halo (zeta on 2, lap(zeta) on 1).  With the one-layer-per-wavefront
    // kernel (option overlap) the wavefronts that read no halo cell are queued first and run beside the exchange, the
    // strips and chunks along the tile edges follow once it has arrived (each cell is written by exactly one wavefront)
    if (m->bc == BC_PERIODIC && m->nranks == 1) launch_fill_periodic(m->st, m->f[MSOM_PSI], m->g, nl, 3);
    if (!m->adv_fused) adv_out = -1;
    // the advance rides along: the pass can also emit the first residual of the inversion of q[adv_out]
    // (k_rhs_lpw's RES instantiation, or the LDS-tile kernel's): one tile with walls and even sides, one residual consumer per solve
    const int variant = m->rhs_variant;
    const bool use_rr = adv_out >= 0 && rhs_resid_emits(m, ps.emit_resid);
    RhsResid rr;
    if (use_rr) {
      rr.res = m->res[0]; rr.res_c = m->res[1]; rr.res_max = m->d_scal + SC_RESF; rr.bsum_partial = m->partial_rr;
      rr.sg = m->sg[0]; rr.cg = m->sg[1];
      if (ps.cls) {   // the speculative pass of mg_solve: max|res| of the solve that made psi, as k_resmax_march would leave it
        rr.cls = ps.cls; rr.cls_b = ps.cls_b; rr.cls_max = m->d_scal + SC_RES1; rr.cls_umax = m->d_scal + SC_UMAX;
      }
    }
    // the psi halo exchange of a tile around the launch(es) of the pass; splittable: the kernel takes a region argument
    auto with_psi_halo = [&](bool splittable, auto launch) {
      if (m->nranks > 1 && m->overlap && splittable) {
        comm_begin(m); m->comm_hold = 1;
        launch(1);
        STICKY(m, exch_nat(m, m->f[MSOM_PSI], nl, m->bc, 3));
        m->comm_hold = 0; comm_end(m);
        launch(2);
      } else {
        if (m->nranks > 1) STICKY(m, exch_nat(m, m->f[MSOM_PSI], nl, m->bc, 3));
        launch(0);
      }
    };
    // one pass over psi: zeta, Jacobians, beta, dissipation, drag, forcing, max|u| (kernels_fused.hip)
    if (stoch_fused) {
      double dts;
      int r = stoch_prepare(m, adv_dt, &dts);
      if (r) return r;
      m->res_ready = -1;
      // the relaxation -q_stage / tau and the noise are read in the finalisation of the pass: q_out = q_in - (dt / tau) q_stage + dts n + dt dq
      prof_begin(m, m->prof_rhs);
      with_psi_halo(true, [&](int region) {
        launch_rhs_lpw(m->st, m->opt, m->f[MSOM_PSI], m->f[MSOM_S], m->f[MSOM_QFORC], m->d_wind, nullptr, m->g, nl, m->walls & WALL_ALL, m->uniformS,
                       m->rc[0].S, with_qforcing && m->have_qforc, D, p.beta, iRe, iRe4, Eks / (p.Rom * 2 * m->dhf[0]),
                       Ekb / (p.Rom * 2 * m->dhf[nl - 1]), p.sbc > 0 ? p.sbc / ((0.5 * p.sbc + 1) * D * D) : 0., m->lc, m->f[adv_in],
                       m->f[adv_out], adv_dt, 1, m->f[qfield], m->f[MSOM_NOISE], -adv_dt * p.itr_stoch, dts, region);
      });
      prof_end(m, m->prof_rhs);
      ps.advanced = true;
      return MSOM_OK;
    }
    prof_begin(m, m->prof_rhs);
    with_psi_halo(variant == 6, [&](int region) {
      launch_rhs_fused(m->st, m->opt, m->f[MSOM_PSI], m->f[MSOM_S], m->f[MSOM_QFORC], m->d_wind, m->f[dqfield], nullptr,
                       nullptr, m->g, nl, m->walls & WALL_ALL, m->uniformS, m->rc[0].S, with_qforcing && m->have_qforc, D, p.beta, iRe,
                       iRe4, Eks / (p.Rom * 2 * m->dhf[0]), Ekb / (p.Rom * 2 * m->dhf[nl - 1]),
                       p.sbc > 0 ? p.sbc / ((0.5 * p.sbc + 1) * D * D) : 0., m->lc, variant, adv_out >= 0 ? m->f[adv_in] : nullptr,
                       adv_out >= 0 ? (ps.out ? ps.out : m->f[adv_out]) : nullptr, adv_dt, use_rr ? &rr : nullptr, region,
                       variant == 6 ? ps.dt_dev : nullptr);
    });
    prof_end(m, m->prof_rhs);
    if (use_rr) {
      m->res_ready = adv_out;
      m->rr_nparts = variant == 6 ? rhs_lpw_blocks(m->opt, m->g, nl) : rhs_pipe_blocks(m->g);
    }
    ps.advanced = adv_out >= 0;
    return MSOM_OK;
  }
  HIPCHK(hipMemsetAsync(m->f[dqfield], 0, m->g.ls * nl * sizeof(double), m->st));  // updates = 0, msqg/qg.h:611-613
  comp_del2(m, MSOM_PSI, MSOM_ZETA, 0., 1.0);
  launch_advection(m->st, m->f[MSOM_ZETA], m->f[MSOM_PSI], m->f[MSOM_PSIPG], m->f[MSOM_ZETAPG], m->f[MSOM_S], m->f[qfield], m->f[dqfield],
                   m->g, nl, m->have_pg, m->have_zpg, m->stochastic, D, p.beta, p.itr_stoch, m->lc);
  // dissip :407-422 (terms with a zero coefficient add exactly 0 and are skipped)
  if (iRe != 0) comp_stretch(m, MSOM_ZETA, dqfield, 1., iRe);
  if (iRe != 0 || iRe4 != 0) comp_del2(m, MSOM_ZETA, MSOM_TMP, 0., 1.);
  if (iRe != 0) launch_axpy(m->st, m->f[dqfield], m->f[MSOM_TMP], m->g, nl, iRe);
  if (iRe4 != 0) {
    comp_stretch(m, MSOM_TMP, dqfield, 1., iRe4);
    comp_del2(m, MSOM_TMP, dqfield, 1., iRe4);
  }
  launch_forcing(m->st, m->f[MSOM_ZETA], m->f[MSOM_PSI], m->f[MSOM_QFORC], m->f[MSOM_TOPO], m->f[MSOM_RO], m->d_wind, m->f[dqfield], m->g,
                 nl, with_qforcing && m->have_qforc, m->flag_topo, Eks / (p.Rom * 2 * m->dhf[0]), Ekb / (p.Rom * 2 * m->dhf[nl - 1]), D,
                 m->dhf[nl - 1]);
  return MSOM_OK;
}

static int tracer_update(msom *m, int cfield);

// first half of update_qg (msqg/qg.h:621-623): invert q -> psi, then the CFL part of
// advection_pv (:383-391): 2*nl limiter calls (psi_l then psipg_l) sharing one static
// `previous`.  max|u| of psi comes out of the solver's last pass (k_residual2<CORRECT>), so dt
// is known BEFORE the tendency pass and the advance can ride in it.
// The same on the device, for the speculative tendency pass of the first RK stage: the 2 nl limiter calls of advection_pv on
// max|u| of psi (d_scal) and of psi_pg, then dtnext() of run() -- the functions of step_dt_inl.h that the host calls.
// The kernel also PUBLISHES the scalar block to the host: 64 threads copy the 64 slots into coherent pinned memory, a system-scope
// fence, then a sequence word the host spins on -- no copy command and no event between the residual pass and the tendency pass.
struct StepDtArgs { double umax_pg[MSOM_MAXNL]; double D, CFL, previous, dtmax, t, tnext; int nl, with_dt; long seq; };
__global__ void __launch_bounds__(64) k_step_dt(double *scal, StepDtArgs a, double *pub) {
  if (threadIdx.x == 0 && a.with_dt) {
    const double *umax = scal + SC_UMAX;
    double *out = scal + SC_SPEC;
    double dtmax = a.dtmax, previous = a.previous, tnext;
    for (int k = 0; k < 2 * a.nl; k++) dtmax = step_limit((k & 1) ? a.umax_pg[k >> 1] : umax[k >> 1], dtmax, a.D, a.CFL, &previous);
    const double dt = step_dtnext(a.t, a.tnext, dtmax, &tnext);
    out[0] = dtmax; out[1] = dt; out[2] = tnext; out[3] = dt / 2.;
  }
  __syncthreads();
  if (pub) {
    pub[threadIdx.x] = scal[threadIdx.x];      // SC_COUNT = 64 slots
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __atomic_store_n(reinterpret_cast<long *>(pub + SC_COUNT), a.seq, __ATOMIC_RELEASE);
  }
}
static_assert(SC_COUNT == 64, "k_step_dt publishes one slot per thread");

// mg_solve's speculative pass: the tendency pass sp->pass and, beside it, k_step_dt.  Stage 1: the kernel computes dt in front of the
// pass, which reads it from the device.  Either stage: the kernel publishes the scalars in front of the pass, or -- the pass closes the
// solve (cls: max|res|, stage 2 max|u| too, come out of it) -- behind it
static void spec_queue(msom *m, SpecPass *sp) {
  const Params &p = m->p;
  const bool closes = sp->pass.cls != 0;
  StepDtArgs a;
  memset(&a, 0, sizeof a);
  if (sp->stage == 1) {
    for (int l = 0; l < MSOM_MAXNL; l++) a.umax_pg[l] = m->umax_pg[l];
    a.D = p.L0 / m->gnx; a.CFL = p.CFL; a.previous = m->previous; a.dtmax = p.DT; a.t = m->t; a.tnext = m->tnext; a.nl = m->nl;
    a.with_dt = 1;
  }
  a.seq = ++m->pub_seq;
  if (a.with_dt || !closes) hipLaunchKernelGGL(k_step_dt, dim3(1), dim3(64), 0, m->st, m->d_scal, a, closes ? nullptr : m->d_pub);
  sp->rc = rhs_terms(m, sp->pass);
  if (!sp->pass.advanced && !sp->rc) sp->rc = MSOM_ERR_STATE;
  if (closes) {
    a.with_dt = 0;
    hipLaunchKernelGGL(k_step_dt, dim3(1), dim3(64), 0, m->st, m->d_scal, a, m->d_pub);
  }
  sp->launched = true;
}

// sp: see mg_solve.  Where its pass counts in the first RK stage, the device has run the limiter as well
static double solve_and_dt(msom *m, int qfield, double dtmax, SpecPass *sp = nullptr) {
  const int nl = m->nl;
  if (invertq(m, m->f[qfield], sp)) return -1;
  if (sp && sp->counts && sp->stage == 1) {   // adopt its state
    m->previous = m->h_scal[SC_SPEC];
    return m->h_scal[SC_SPEC];
  }
  if (!m->umax_ready) {
    launch_umax(m->st, m->f[MSOM_PSI], m->partial_umax, m->d_scal + SC_UMAX, m->g, nl, m->p.L0 / m->gnx);
    if (reduce_scal(m, SC_UMAX, nl, RED_MAX)) return -1;
  }
  if (m->sticky) return -1;
  for (int l = 0; l < nl; l++) {
    dtmax = limiter(m, m->h_scal[SC_UMAX + l], dtmax);
    dtmax = limiter(m, m->umax_pg[l], dtmax);
  }
  return dtmax;
}

// update_qg, msqg/qg.h:609-650
static double update_qg(msom *m, int qfield, int dqfield, double dtmax) {
  dtmax = solve_and_dt(m, qfield, dtmax);
  if (dtmax < 0) return -1;
  RhsPass ps{qfield, dqfield, 1};
  if (rhs_terms(m, ps)) return -1;
  if (m->p.nptr > 0 && tracer_update(m, qfield == MSOM_QPRED ? MSOM_PTR_PRED : MSOM_PTR)) return -1;
  return dtmax;
}

// reference-exact noise: Box-Muller on the serial rand() stream in foreach order
// (x outer, y inner, layer innermost), msqg/qg_stochastic.h:9,117-126
static int generate_noise_host(msom *m) {
  const int nl = m->nl, nx = m->nx, ny = m->ny;
  std::vector<double> sig((size_t)nl * nx * ny), n((size_t)nl * nx * ny);
  int r = download(m, MSOM_SIGMA, sig.data());
  if (r) return r;
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++)
      for (int l = 0; l < nl; l++) {
        const double a = sqrt(-2. * log(((double)(rand()) + 1.) / ((double)(RAND_MAX) + 2.)));
        const double nn = a * cos(2 * M_PI * rand() / (double)RAND_MAX);
        const size_t k = ((size_t)l * ny + j) * nx + i;
        n[k] = m->p.amp_stoch * sig[k] * nn;
      }
  return upload(m, MSOM_NOISE, n.data());
}

// the stochastic part of advance_qg (msqg/qg_stochastic.h:128-138): every other call draws new noise and uses
// sqrt(dt)/sqrt(2), computed in float as the reference does
static int stoch_prepare(msom *m, double dt, double *dts) {
  // refused before any state changes: one rand() stream per process would repeat the same numbers on every tile
  if (m->noise_mode == 0 && m->nranks > 1) {
    msom_set_error("stochastic forcing on tiles: the serial rand() stream (noise_mode = 0) exists on a single tile only, use noise_mode = 1");
    return MSOM_ERR_STATE;
  }
  m->corrector_step = (m->corrector_step + 1) % 2;
  float fdts = sqrt(dt);
  if (m->corrector_step) {
    if (m->noise_mode == 0) {  // reference-exact serial rand() stream
      int r = generate_noise_host(m);
      if (r) return r;
    } else  // counter-based device generator
      launch_noise(m->st, m->f[MSOM_NOISE], m->f[MSOM_SIGMA], m->g, m->nl, m->p.amp_stoch, m->seed, m->noise_draw++, m->ix * m->nx,
                   m->iy * m->ny, m->gnx);
    fdts = fdts / sqrt(2);
  }
  *dts = fdts;
  return MSOM_OK;
}

// advance_qg, msqg/qg.h:594-606 / msqg/qg_stochastic.h:128-149
static int advance_qg(msom *m, int out, int in, int dq, double dt) {
  m->res_ready = -1;
  const double *noise = nullptr;
  double dts = 0;
  if (m->stochastic) {
    int r = stoch_prepare(m, dt, &dts);
    if (r) return r;
    noise = m->f[MSOM_NOISE];
  }
  launch_advance(m->st, m->f[out], m->f[in], m->f[dq], noise, m->g, m->nl, dt, dts);
  fill_bc(m, out);
  return MSOM_OK;
}

extern "C" double msom_update(msom_t *m, const double *q, double *dqdt, double dtmax) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  if (!m) return -1;
  if (m->model) return nq_update(m, q, dqdt, dtmax);
  if (!m->const_set && msom_set_const(m)) return -1;
  int qf = MSOM_Q;
  if (q) {
    if (upload(m, MSOM_QPRED, q)) return -1;
    qf = MSOM_QPRED;
  }
  double d = update_qg(m, qf, MSOM_DQ, dtmax);
  if (d < 0) return d;
  if (dqdt && download(m, MSOM_DQ, dqdt)) return -1;
  return d;
}

extern "C" int msom_advance(msom_t *m, double *qout, const double *qin, const double *dqdt, double dt) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  if (m && m->model) return nq_advance(m, qout, qin, dqdt, dt);
  NEED_CONST(m);
  int in = MSOM_Q, out = MSOM_Q, r;
  if (qin) {
    if ((r = upload(m, MSOM_QPRED, qin))) return r;
    in = out = MSOM_QPRED;
  }
  if (dqdt && (r = upload(m, MSOM_DQ, dqdt))) return r;
  if ((r = advance_qg(m, out, in, MSOM_DQ, dt))) return r;
  if (qout) return download(m, out, qout);
  return sync_stream(m);
}

extern "C" int msom_invertq(msom_t *m, const double *q, double *psi, msom_mgstats *st) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  if (m && m->model) return nq_invertq(m, q, psi, st);
  NEED_CONST(m);
  int qf = MSOM_Q, r;
  if (q) {
    if ((r = upload(m, MSOM_QPRED, q))) return r;
    qf = MSOM_QPRED;
  }
  if (psi && (r = upload(m, MSOM_PSI, psi))) return r;
  if ((r = invertq(m, m->f[qf]))) return r;
  if (st) *st = m->mg;
  if (psi) return download(m, MSOM_PSI, psi);
  return sync_stream(m);
}

extern "C" int msom_comp_q(msom_t *m, const double *psi, double *q) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  if (m && m->model) return nq_comp_q_api(m, psi, q);
  NEED_CONST(m);
  int r;
  if (psi && (r = upload(m, MSOM_PSI, psi))) return r;
  comp_del2(m, MSOM_PSI, MSOM_Q, 0., 1.);
  comp_stretch(m, MSOM_PSI, MSOM_Q, 1., 1.);
  if (q) return download(m, MSOM_Q, q);
  return sync_stream(m);
}

extern "C" int msom_last_mgstats(msom_t *m, msom_mgstats *st) {
  if (!m || !st) return MSOM_ERR_ARG;
  *st = m->mg;
  return MSOM_OK;
}

extern "C" int msom_modes_mgstats(msom_t *m, int mode, msom_mgstats *st) {
  MSQG_ONLY(m);
  if (!m || !st) return MSOM_ERR_ARG;
  if (!m->const_set || !m->helm_solved) { msom_set_error("msom_modes_mgstats: no modal solve since msom_set_const"); return MSOM_ERR_STATE; }
  if (mode < 0 || mode >= m->nl) { msom_set_error("msom_modes_mgstats: mode %d outside 0 .. %d", mode, m->nl - 1); return MSOM_ERR_ARG; }
  *st = m->helm.s[mode];
  return MSOM_OK;
}

// ------------------------------------------------------------------ pystep_bfn & co

int check_shape(msom *m, int a, int b, int c) {
  if (a != m->nl || b != m->ny || c != m->nx) {
    msom_set_error("array shape (%d,%d,%d) != (nl,N,N) = (%d,%d,%d)", a, b, c, m->nl, m->ny, m->nx);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}

// the signs of the dissipation and of the drag for an integration forward (direction > 0) or backward in time, msqg/qg_bfn.h:30-41
static void bfn_direction(Params &p, double direction) {
  const double s = direction > 0 ? 1 : -1;
  p.iRe = p.Re == 0 ? 0. : s / p.Re;
  p.iRe4 = p.Re4 == 0 ? 0. : -s / p.Re4;
  p.Eks = s * fabs(p.Eks); p.Ekb = s * fabs(p.Ekb);
}

// msqg/qg_bfn.h:21-80
extern "C" int pystep_bfn(msom_t *m, double *varin_py, int len1, int len2, int len3, double *tend_py, int len4, int len5, int len6,
                          double direction, int vartype) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  if (check_shape(m, len1, len2, len3) || check_shape(m, len4, len5, len6)) return MSOM_ERR_ARG;
  Params &p = m->p;
  int r;
  bfn_direction(p, direction);
  if (vartype != 1) HIPCHK(hipMemsetAsync(m->f[MSOM_DQ], 0, m->g.ls * m->nl * sizeof(double), m->st));  // reset_layer_var(bfn_tendl)
  if (vartype == 1) {
    if ((r = upload(m, MSOM_Q, varin_py))) return r;
    if (solve_and_dt(m, MSOM_Q, p.DT) < 0) return MSOM_ERR_HIP;  // invertq + the dt limiter inside advection_pv
    RhsPass ps{MSOM_Q, MSOM_DQ, 0};
    if ((r = rhs_terms(m, ps))) return r;
  } else if (!m->quiet)
    fprintf(stdout, "temporary disabled psi tendency\n");  // msqg/qg_bfn.h:48
  return download(m, MSOM_DQ, tend_py);
}
// msqg/qg_bfn.h:85-93
extern "C" int pyq2p(msom_t *m, double *po_py, int len7, int len8, int len9, double *qo_py, int len10, int len11, int len12) {
  MSQG_ONLY(m);
  NEED_CONST(m);
  if (check_shape(m, len7, len8, len9) || check_shape(m, len10, len11, len12)) return MSOM_ERR_ARG;
  int r;
  m->res_ready = -1;
  HIPCHK(hipMemsetAsync(m->f[MSOM_PSI], 0, m->g.ls * m->nl * sizeof(double), m->st));
  if ((r = upload(m, MSOM_Q, qo_py))) return r;
  if ((r = invertq(m, m->f[MSOM_Q]))) return r;
  return download(m, MSOM_PSI, po_py);
}
// msqg/qg_bfn.h:95-103
extern "C" int pyp2q(msom_t *m, double *po_py, int len13, int len14, int len15, double *qo_py, int len16, int len17, int len18) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  if (check_shape(m, len13, len14, len15) || check_shape(m, len16, len17, len18)) return MSOM_ERR_ARG;
  return msom_comp_q(m, po_py, qo_py);
}

// ------------------------------------------------------------------ the loop of msqg/qg_bfn.py:47-73 on the device

// msqg/qg_bfn.py:49-51: zero history; the AB3 weights apply from the first step on
extern "C" int msom_bfn_begin(msom_t *m) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  int r;
  for (int k = MSOM_BFN_F1; k <= MSOM_BFN_F3; k++) {
    if ((r = ensure_field(m, k))) return r;
    HIPCHK(hipMemsetAsync(m->f[k], 0, m->g.ls * m->nl * sizeof(double), m->st));
  }
  m->bfn_begun = 1;
  return sync_stream(m);
}

// msqg/qg_bfn.py:62-73 with the nudging term of :67-68
extern "C" int msom_bfn_steps(msom_t *m, int nsteps, double dt, double direction, double k) {
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  if (nsteps < 0) { msom_set_error("msom_bfn_steps: nsteps = %d", nsteps); return MSOM_ERR_ARG; }
  if (!m->const_set || !m->bfn_begun) { msom_set_error("msom_bfn_steps before msom_bfn_begin"); return MSOM_ERR_STATE; }
  if (k != 0 && !m->bfn_obs_set) { msom_set_error("msom_bfn_steps: k != 0 and MSOM_BFN_OBS was never set"); return MSOM_ERR_STATE; }
  if (nsteps == 0) return MSOM_OK;
  Params &p = m->p;
  int r;
  bfn_direction(p, direction);   // as pystep_bfn
  const double dt12 = dt / 12;
  const double *obs = k != 0 ? m->f[MSOM_BFN_OBS] : nullptr, *gain = (k != 0 && m->bfn_gain_set) ? m->f[MSOM_BFN_GAIN] : nullptr;
  for (int n = 0; n < nsteps; n++) {
    if (solve_and_dt(m, MSOM_Q, p.DT) < 0) return m->sticky ? m->sticky : MSOM_ERR_HIP;  // invertq + the dt limiter inside advection_pv
    RhsPass ps{MSOM_Q, MSOM_BFN_F1, 0};   // the tendency goes straight into the F1 slot
    if ((r = rhs_terms(m, ps))) return r;
    launch_bfn_ab3(m->st, m->f[MSOM_Q], m->f[MSOM_BFN_F1], m->f[MSOM_BFN_F2], m->f[MSOM_BFN_F3], obs, gain, m->g, m->nl, dt12, k);
    fill_bc(m, MSOM_Q);    // boundary(q), as upload does after its pack
    m->res_ready = -1;     // what the handle caches from q
    m->umax_ready = 0;
    double *f1 = m->f[MSOM_BFN_F1];   // F3 = F2; F2 = F1 (:72-73) as a rotation of the slots
    m->f[MSOM_BFN_F1] = m->f[MSOM_BFN_F3];
    m->f[MSOM_BFN_F3] = m->f[MSOM_BFN_F2];
    m->f[MSOM_BFN_F2] = f1;
  }
  return sync_stream(m);
}

extern "C" int msom_bfn_misfit(msom_t *m, double *misfit) {
  MSQG_ONLY(m);
  if (!m || !misfit) return MSOM_ERR_ARG;
  if (!m->bfn_obs_set) { msom_set_error("msom_bfn_misfit: MSOM_BFN_OBS was never set"); return MSOM_ERR_STATE; }
  if (!m->bfn_partial) HIPCHK(hipMalloc(&m->bfn_partial, 2 * ((size_t)bfn_misfit_blocks(m->g) + 64) * sizeof(double)));
  launch_bfn_misfit(m->st, m->f[MSOM_Q], m->f[MSOM_BFN_OBS], m->bfn_gain_set ? m->f[MSOM_BFN_GAIN] : nullptr, m->bfn_partial,
                    m->d_scal + SC_LSUM, m->g, m->nl);
  int r = reduce_scal(m, SC_LSUM, 2, RED_SUM);
  if (r) return r;
  *misfit = sqrt(m->h_scal[SC_LSUM] / m->h_scal[SC_LSUM + 1]);
  return MSOM_OK;
}

// ------------------------------------------------------------------ time loop

double dtnext(msom *m, double dt, double *tnext_out) { return step_dtnext(m->t, m->tnext, dt, tnext_out); }

// tracer part of update_qg (msqg/qg.h:634-647): dpdt = ptr_rhs(tracers, psi) with `updates` zeroed
static int tracer_update(msom *m, int cfield) {
  const int nt = m->nl * m->p.nptr;
  HIPCHK(hipMemsetAsync(m->f[MSOM_DPTR], 0, m->g.ls * nt * sizeof(double), m->st));
  launch_ptr_rhs(m->st, m->f[MSOM_PSI], m->f[cfield], m->f[MSOM_PTR_RELAX], m->f[MSOM_DPTR], m->g, m->nl, m->p.nptr, m->p.iPe, m->p.ptr_ir,
                 m->p.L0 / m->gnx);
  return MSOM_OK;
}
// tracer part of advance_qg (msqg/qg.h:597-605)
static int tracer_advance(msom *m, int out, int in, double dt) {
  launch_advance(m->st, m->f[out], m->f[in], m->f[MSOM_DPTR], nullptr, m->g, m->nl * m->p.nptr, dt, 0.);
  return fill_bc(m, out);
}

// one iteration of run() [Basilisk predictor-corrector.h]:
//   dt = dtnext(update(evolving, updates, DT)); advance(predictor, evolving, updates, dt/2);
//   update(predictor, updates, dt); advance(evolving, evolving, updates, dt)
// dt is known right after each inversion, so both advances ride in the tendency kernel
// (q_out = q_in + dt * dq) whenever the fused kernel applies; dq is then never stored.
// can a stage's tendency pass be queued speculatively?  One tile, the fused one-layer-per-wavefront kernel with the advance
// folded in, max|u| out of the solver's last pass, nothing with side effects in the pass (noise draws, tracers)
static bool spec_ok(const msom *m) {
  return layered_fusions(m) && m->async_solve && m->nranks == 1 && m->fused && m->adv_fused && m->rhs_variant == 6 && m->mg_fused && m->nlev > 1 &&
         m->nl <= MSOM_FASTNL && !m->have_pg && !m->have_zpg && !m->flag_topo && !m->stochastic && m->p.nptr == 0 && m->p.nitermin >= 1 && !m->dbg_nosync;
}

// One RK stage of msom_step: the solve with the stage's tendency + advance pass queued behind its first cycle (spec: struct
// SpecPass), the same pass afterwards where that one does not count, then the tracers.
//   stage 1: q -> psi, dt = dtnext(limiter), predictor = q + dt/2 dq; speculatively with dt computed and read on the device
//   stage 2: predictor -> psi, q += dt dq; speculatively into q_alt, which becomes q only if the solve ended after its first cycle
static int rk_stage(msom *m, int stage, bool spec, double *tnext) {
  const bool first = stage == 1;
  const int qf = first ? MSOM_Q : MSOM_QPRED, out = first ? MSOM_QPRED : MSOM_Q;
  RhsPass ps{qf, MSOM_DQ, 1, out, MSOM_Q};
  SpecPass sp{stage, ps};
  if (first) sp.pass.dt_dev = m->d_scal + SC_SPEC + 3;
  else { sp.pass.adv_dt = m->dt; sp.pass.out = m->q_alt; }
  const double d = solve_and_dt(m, qf, first ? m->p.DT : m->dt, spec ? &sp : nullptr);
  const bool hit = spec && sp.counts && !sp.rc;
  // a speculative pass may have emitted the next solve's first residual (rhs_resid): it counts only with the pass itself.  Discarded:
  // the solve went on and regenerated res[0], res[1] behind it; the re-run below emits them again.  Kept in stage 2: the residual
  // of q_alt, which is q from here on, is what the next step's first solve is handed
  if (!hit) m->res_ready = -1;
  if (d < 0) return m->sticky ? m->sticky : MSOM_ERR_HIP;
  if (first) {
    if (hit) {   // the device's dtnext
      m->dt = m->h_scal[SC_SPEC + 1];
      *tnext = m->h_scal[SC_SPEC + 2];
    } else
      m->dt = dtnext(m, d, tnext);
  } else if (hit)
    std::swap(m->f[MSOM_Q], m->q_alt);
  const double adv_dt = first ? m->dt / 2. : m->dt;
  int r;
  if (!hit) {
    ps.adv_dt = adv_dt;
    if ((r = rhs_terms(m, ps))) return r;
    if (!ps.advanced && (r = advance_qg(m, out, MSOM_Q, MSOM_DQ, adv_dt))) return r;
  }
  // option "stats": one sample of (q_n, psi_n = what the first inversion left, dt_n) before stage 2 overwrites psi.  Queued behind the
  // stage's tendency pass; on the speculative path the weight is the device scalar k_step_dt wrote (no host value is waited for)
  if (first && m->stats_on && m->stats_count++ % m->stats_every == 0) {
    stats_sample(m, hit ? m->d_scal + SC_SPEC + 1 : nullptr, m->dt);
    m->stats_ndev += hit;
  }
  // the floats' RK2 stages ride behind the model's: stage 1 reads psi_n behind the first tendency pass, stage 2 psi_{n+1/2} behind the second
  if (m->floats.on) floats_hook(m, stage, *tnext);
  if (m->p.nptr > 0 && ((r = tracer_update(m, first ? MSOM_PTR : MSOM_PTR_PRED)) || (r = tracer_advance(m, first ? MSOM_PTR_PRED : MSOM_PTR, MSOM_PTR, adv_dt))))
    return r;
  return MSOM_OK;
}

extern "C" int msom_step(msom_t *m, double *dt_used) {
  if (m && m->model) return nq_step(m, dt_used);
  NEED_CONST(m);
  if (m->stats_on && !m->stats_mask) { msom_set_error("msom_step: option stats = 1 and no msom_stats_begin since msom_set_const"); return MSOM_ERR_STATE; }
  double tnext;
  int r;
  const bool spec = spec_ok(m);
  if ((r = rk_stage(m, 1, spec, &tnext))) return r;
  if (spec && !m->q_alt) {   // pads and ghost cells as q has them: the pass writes interior cells only
    HIPCHK(hipMalloc(&m->q_alt, m->g.ls * m->nl * sizeof(double)));
    HIPCHK(hipMemcpyAsync(m->q_alt, m->f[MSOM_Q], m->g.ls * m->nl * sizeof(double), hipMemcpyDeviceToDevice, m->st));
  }
  if ((r = rk_stage(m, 2, spec, &tnext))) return r;
  // With the speculative tendency pass the host already follows the GPU solve by solve (it waits for the published residual of every
  // solve) and everything it returns -- dt, t -- is known: with step_sync = 0 the last tendency pass is left running and the next step's
  // launches queue up behind it (every call that hands device data to the host synchronises the stream itself, msom_sync on request)
  const bool lazy = m->step_sync == 0 || (m->step_sync < 0 && (size_t)m->g.nx * m->g.ny * m->nl < ((size_t)1 << 23));
  if (!spec || !lazy) { if ((r = sync_stream(m))) return r; }
  else if (m->sticky) return m->sticky;
  m->t = tnext;
  m->iter++;
  if (dt_used) *dt_used = m->dt;
  return MSOM_OK;
}
extern "C" int msom_sync(msom_t *m) {
  if (!m) return MSOM_ERR_ARG;
  return sync_stream(m);
}
extern "C" int msom_set_tnext(msom_t *m, double tnext) {
  if (!m) return MSOM_ERR_ARG;
  m->tnext = tnext;
  return MSOM_OK;
}
extern "C" double msom_time(msom_t *m) { return m ? m->t : NAN; }
extern "C" int msom_iter(msom_t *m) { return m ? m->iter : -1; }

// msqg/qg.c:101-109
extern "C" double msom_ke(msom_t *m) {
  if (!m) return NAN;
  launch_ke(m->st, m->f[MSOM_PSI], m->partial, m->d_scal + SC_KE, m->g, m->p.L0 / m->gnx);
  if (reduce_scal(m, SC_KE, 1, RED_SUM)) return NAN;
  return -m->h_scal[SC_KE];
}

// ------------------------------------------------------------------ tiling (single tile for now)

extern "C" int msom_set_device(int device) {
  HIPCHK(hipSetDevice(device));
  return MSOM_OK;
}

extern "C" int msom_comm_unique_id(void *id128) {
  if (!id128) return MSOM_ERR_ARG;
  return comm_unique_id(id128);
}
// One tile of a px x py decomposition.  id128 = ncclUniqueId from msom_comm_unique_id (RCCL
// transport, one process per GPU), or "MSOMLOCL" + 8-byte key for the in-process test
// transport (one host thread per tile).
extern "C" msom_t *msom_create_tiled(const char *params_text, int px, int py, int rank, const void *id128) {
  if (!params_text || px < 1 || py < 1 || rank < 0 || rank >= px * py || (px * py > 1 && !id128)) {
    msom_set_error("msom_create_tiled: bad arguments");
    return nullptr;
  }
  Params p;
  msom_params_defaults(&p);
  msom_params_parse_text(&p, params_text);
  msom *m = create_common(p, px, py, rank, id128);
  if (m) m->params_text = params_text;
  return m;
}
extern "C" int msom_tile_info(msom_t *m, int *px, int *py, int *ix, int *iy, int *nx_local, int *ny_local) {
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  if (px) *px = m->px;
  if (py) *py = m->py;
  if (ix) *ix = m->ix;
  if (iy) *iy = m->iy;
  if (nx_local) *nx_local = m->nx;
  if (ny_local) *ny_local = m->ny;
  return MSOM_OK;
}
