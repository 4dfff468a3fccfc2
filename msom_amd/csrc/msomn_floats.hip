// msomn_floats.hip -- Lagrangian floats of the vertex-grid model, advected with the model's RK2 stages (include/msomn_floats.h,
// DESIGN.md section 8l): the msomn_floats_* entry points and the hook msomn_step (msom_node.hip) calls behind its first update and
// behind its final advance.  Arithmetic: the vertex part of floats_inl.h; kernels: kernels_node_floats.hip.  On tiles (option
// floats_tiles, "On tiles" in section 8l) every call is collective: each rank holds the floats it owns in n slots, a migration pass
// behind every stage kernel takes them to their new owner (the kernels of kernels_floats.hip), readouts are combined over the ranks.
// Without the option a handle of more than one tile answers every call with MSOM_ERR_CONFIG.
#include <cmath>

#include "msomn_host.h"

#include "../../include/msomn_floats.h"

bool is_device_ptr(const void *p);   // msom_diag.hip

enum { NFC_CLAMPED = 0, NFC_LOST = 1, NFC_UNSENT = 2, NFC_MIGRATED = 3, NFC_LAND = 4, NFC_COUNT = 5 };

struct NFloatsState {
  int n = 0;
  double *buf = nullptr;               // x, y, xh, yh and two output arrays of the by-hand calls, n doubles each
  int *layer = nullptr;
  unsigned long long *cnt = nullptr;   // NFC_*: clamped, lost, (tiles) unsent and records sent, and the scratch word of "floats_on_land"
  int staged = 0;                      // a stage 1 since msomn_floats_begin or the last stage 2
  // trajectory buffer [cap][2 or 3][n]; times on the host
  double *rec = nullptr;
  int every = 1, cap = 0, nrec = 0;
  int field = -1;                      // the field recorded along the trajectories (< 0: positions only)
  long steps = 0, dropped = 0;         // stage-2 hooks seen since msomn_floats_record; records that found the buffer full
  std::vector<double> t;
  // on tiles (option floats_tiles, more than one tile): the arrays above are n slots of which this rank fills those of the floats it
  // owns; records are [cap][3 or 6][n], indexed by id: x, y and a presence word, then the value, a row not used and its presence word
  int tiled = 0, K = 0;                // K: records a message can carry (option floats_msg_cap)
  int *id = nullptr, *live = nullptr;
  int *ctl = nullptr;                  // high-water mark, free slots, records taken in the lo / hi message of the running phase
  int *freest = nullptr;               // free stack
  double *msg = nullptr;               // send W E S N, receive W E S N: 1 + 6 K doubles each
  double *gs = nullptr, *gr = nullptr; // readouts: this rank's [3][n] by id, all ranks' [ntiles][3][n]
  double *dsum = nullptr;              // the counters as doubles, for the sum over the ranks
};

static FloatsDev nfl_dev(const NFloatsState *s) {
  return FloatsDev{s->buf, s->buf + s->n, s->buf + 2 * (size_t)s->n, s->buf + 3 * (size_t)s->n, s->layer, s->cnt};
}
// the global geometry, on a tile too
static FloatsGeom nfl_geom(const msomn *m) { return FloatsGeom{m->N, m->N, 0, m->N / m->p.L0, m->p.L0, m->p.L0}; }
static FloatsTiling nfl_tiling(const msomn *m) { return FloatsTiling{m->px, m->py, m->rank % m->px, m->rank / m->px, m->g.nx - 1, m->g.ny - 1}; }
static FloatsTileDev nfl_tile(const msomn *m, const NFloatsState *s) { return FloatsTileDev{s->id, s->live, s->ctl, m->ox, m->oy}; }
static FloatsMig nfl_mig(const NFloatsState *s) {
  const size_t n = s->n;
  return FloatsMig{s->buf, s->buf + n, s->buf + 2 * n, s->buf + 3 * n, s->layer, s->id, s->live, s->ctl, s->ctl + 1, s->freest, s->ctl + 2, s->cnt};
}
static size_t nfl_msgcount(const NFloatsState *s) { return 1 + 6 * (size_t)s->K; }
static const double *nfl_pg(const msomn *m) { return m->pg_set ? m->f[MSOMN_PSIPG] : nullptr; }
static size_t nfl_rows(const NFloatsState *s) { return s->tiled ? (s->field < 0 ? 3 : 6) : (s->field < 0 ? 2 : 3); }
static void nfl_free(NFloatsState *s) {
  if (!s) return;
  for (void *p : {(void *)s->buf, (void *)s->layer, (void *)s->cnt, (void *)s->rec, (void *)s->id, (void *)s->live, (void *)s->ctl, (void *)s->freest,
                  (void *)s->msg, (void *)s->gs, (void *)s->gr, (void *)s->dsum})
    if (p) (void)hipFree(p);
  delete s;
}

void nfloats_drop(msomn *m) {
  if (!m->floats) return;
  (void)hipStreamSynchronize(m->st);   // a stage may still be running
  nfl_free(m->floats);
  m->floats = nullptr;
  m->floats_on = 0;
}

// The migration pass behind a stage kernel (tiles): two phases, W / E, then S / N over all residents, arrivals of the first phase
// included, so a diagonal move needs no diagonal message.  Every rank posts every message of the fixed count 1 + 6 K, with or
// without emigrants, and both phases, with or without neighbours: nothing is read on the host and the in-process barriers match.
// half: the floats are homed by (xh, yh), what stage 2 evaluates.  On the handle's stream, like everything on a vertex tile
static int nfl_migrate(msomn *m, int half) {
  NFloatsState *s = m->floats;
  const size_t mc = nfl_msgcount(s);
  const FloatsMig mg = nfl_mig(s);
  const FloatsGeom fg = nfl_geom(m);
  const FloatsTiling tl = nfl_tiling(m);
  for (int ph = 0; ph < 2; ph++) {
    const int lo = ph ? DIR_S : DIR_W, hi = ph ? DIR_N : DIR_E;
    Xfer x[2];
    int nx = 0;
    double *sb[2] = {nullptr, nullptr}, *rb[2] = {nullptr, nullptr};
    for (int e = 0; e < 2; e++) {
      const int dir = e ? hi : lo;
      if (m->nb[dir] < 0) continue;
      sb[e] = s->msg + dir * mc;
      rb[e] = s->msg + (4 + dir) * mc;
      x[nx++] = {m->nb[dir], dir, sb[e], rb[e], mc};
    }
    if (nx) launch_floats_emigrate(m->st, mg, s->n, fg, tl, ph, half, sb[0], sb[1], s->K, true);
    if (int r = comm_exchange(m->comm, x, nx)) return r;
    if (nx) launch_floats_immigrate(m->st, mg, s->n, m->nl, rb[0], rb[1], s->K);
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

// one stage and, on tiles, what goes with it; rec: the record slot that is due (stage 2), or null
static int nfl_stage(msomn *m, int stage, double dt, double *rec) {
  NFloatsState *s = m->floats;
  const double *rf = rec && s->field >= 0 ? m->f[s->field] : nullptr;
  if (!s->tiled) {
    launch_nfloats_stage(m->st, stage, nfl_dev(s), s->n, m->f[MSOMN_PSI], nfl_pg(m), m->g, nfl_geom(m), dt, rec, rf);
    HIPCHK(hipGetLastError());
    s->staged = stage == 1;
    return MSOM_OK;
  }
  int r;
  const FloatsTileDev td = nfl_tile(m, s);
  if (rec) HIPCHK(hipMemsetAsync(rec, 0, nfl_rows(s) * s->n * sizeof(double), m->st));   // the presence words
  if (stage == 1 && s->staged && (r = nfl_migrate(m, 0))) return r;   // a stage 1 without its stage 2: home by (x, y) again
  // the positions of a record are written by the rank the float is resident on, before the pass takes it elsewhere ...
  launch_nfloats_stage(m->st, stage, nfl_dev(s), s->n, m->f[MSOMN_PSI], nfl_pg(m), m->g, nfl_geom(m), dt, rec, nullptr, &td);
  HIPCHK(hipGetLastError());
  s->staged = stage == 1;
  if ((r = nfl_migrate(m, stage == 1))) return r;
  // ... and the value of the recorded field by the new position's owner, behind the pass: the corners are vertices it holds
  if (rf) {
    launch_nfloats_interp(m->st, nfl_dev(s), s->n, rf, nullptr, m->g, nfl_geom(m), rec + 3 * (size_t)s->n, nullptr, &td);
    HIPCHK(hipGetLastError());
  }
  return MSOM_OK;
}

int nfloats_hook(msomn *m, int stage, double tnext) {
  NFloatsState *s = m->floats;
  double *rec = nullptr;
  if (stage == 2 && s->rec && ++s->steps % s->every == 0) {
    if (s->nrec < s->cap) {
      rec = s->rec + (size_t)s->nrec++ * nfl_rows(s) * s->n;
      s->t.push_back(tnext);
    } else
      s->dropped++;
  }
  return nfl_stage(m, stage, m->dt, rec);
}

// readouts on tiles: send [3][n] by id with its presence words -> the values of every id, taken from the rank that holds it, in the
// two output arrays behind the slots; then to the caller's u0, u1 (host or device, either may be null)
static int nfl_combine(msomn *m, const double *send, double *u0, double *u1) {
  NFloatsState *s = m->floats;
  const size_t n = s->n;
  double *o0 = s->buf + 4 * n, *o1 = o0 + n;
  if (int r = comm_allgather(m->comm, send, s->gr, 3 * n)) return r;
  launch_floats_select(m->st, s->gr, m->ntiles, s->n, o0, o1);
  HIPCHK(hipGetLastError());
  if (u0) HIPCHK(hipMemcpyAsync(u0, o0, n * sizeof(double), hipMemcpyDefault, m->st));
  if (u1) HIPCHK(hipMemcpyAsync(u1, o1, n * sizeof(double), hipMemcpyDefault, m->st));
  return MSOM_OK;
}

bool nfloats_param(msomn *m, const char *key, double *v) {
  if (strncmp(key, "floats", 6)) return false;
  const NFloatsState *s = m->floats;
  const char *k = key + 6;
  static const char *const counters[NFC_COUNT] = {"_clamped", "_lost", "_unsent", "_migrated", "_on_land"};
  int which = -1;
  for (int c = 0; c < NFC_COUNT; c++)
    if (!strcmp(k, counters[c])) which = c;
  if (!*k) *v = s ? s->n : 0;
  else if (!strcmp(k, "_records")) *v = s ? s->nrec : 0;
  else if (!strcmp(k, "_dropped")) *v = s ? (double)s->dropped : 0;
  else if (!strcmp(k, "_tiles")) *v = m->floats_tiles;
  else if (!strcmp(k, "_msg_cap")) *v = s && s->tiled ? s->K : m->floats_msg_cap;
  else if (!strcmp(k, "_resident")) {   // the rank's own: slots below the mark that are not on the free stack
    int c[2] = {s ? s->n : 0, 0};
    if (s && s->tiled && (hipStreamSynchronize(m->st) != hipSuccess || hipMemcpy(c, s->ctl, sizeof c, hipMemcpyDeviceToHost) != hipSuccess)) { *v = NAN; return true; }
    *v = c[0] - c[1];
  } else if (which >= 0) {
    unsigned long long c[NFC_COUNT] = {0, 0, 0, 0, 0};
    *v = NAN;
    if (s) {
      if (which == NFC_LAND) {   // counted now, behind whatever the stream still holds
        const FloatsTileDev td = s->tiled ? nfl_tile(m, s) : FloatsTileDev{};
        if (hipMemsetAsync(s->cnt + NFC_LAND, 0, sizeof(unsigned long long), m->st) != hipSuccess) return true;
        launch_nfloats_on_land(m->st, nfl_dev(s), s->n, m->f[MSOMN_MASK], m->g, nfl_geom(m), s->cnt + NFC_LAND, s->tiled ? &td : nullptr);
      }
      if (hipStreamSynchronize(m->st) != hipSuccess || hipMemcpy(c, s->cnt, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return true;
    }
    double h[NFC_COUNT];
    for (int q = 0; q < NFC_COUNT; q++) h[q] = (double)c[q];
    if (s && s->tiled) {   // collective: the sum over the ranks (whole numbers far below 2^53: exact in any order)
      if (hipMemcpy(s->dsum, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return true;
      if (comm_allreduce(m->comm, s->dsum, h, NFC_COUNT, RED_SUM)) return true;
    }
    *v = h[which];
  } else
    return false;
  return true;
}

// what every call checks first: the handle, one tile or option floats_tiles; need: floats begun
static int nfl_guard(msomn *m, const char *fn, bool need) {
  if (!m) { msom_set_error("%s: null handle", fn); return MSOM_ERR_ARG; }
  if (!m->floats_tiles)
    if (int r = nt_refuse(m, fn)) return r;
  if (need && !m->floats) { msom_set_error("%s: no msomn_floats_begin since msomn_set_const", fn); return MSOM_ERR_STATE; }
  return MSOM_OK;
}
// a field of nl layers
static int nfl_field(msomn *m, const char *fn, int field) {
  if (field < 0 || field >= MSOMN_NFIELDS || !m->f[field] || m->fl[field] != m->nl) {
    msom_set_error("%s: field id %d is not a field of %d layers of this handle", fn, field, m->nl);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}
static int nfl_sync(msomn *m) {
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
// the arguments of msomn_floats_begin, arrays on the host
static int nfl_check(const msomn *m, int n, const double *x, const double *y, const int *layer) {
  if (n < 1 || !x || !y || !layer) { msom_set_error("msomn_floats_begin: n = %d, x, y or layer null", n); return MSOM_ERR_ARG; }
  const double L0 = m->p.L0;
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(x[k]) || !std::isfinite(y[k])) { msom_set_error("msomn_floats_begin: float %d at (%g, %g)", k, x[k], y[k]); return MSOM_ERR_ARG; }
    if (!(x[k] >= 0 && x[k] <= L0 && y[k] >= 0 && y[k] <= L0)) {
      msom_set_error("msomn_floats_begin: float %d at (%g, %g) outside [0, %g] x [0, %g]", k, x[k], y[k], L0, L0);
      return MSOM_ERR_ARG;
    }
    if (layer[k] < 0 || layer[k] >= m->nl) { msom_set_error("msomn_floats_begin: float %d in layer %d of %d", k, layer[k], m->nl); return MSOM_ERR_ARG; }
  }
  return MSOM_OK;
}

extern "C" int msomn_floats_begin(msomn_t *m, int n, const double *x, const double *y, const int *layer) {
  int r = nfl_guard(m, "msomn_floats_begin", false);
  if (r) return r;
  const bool tiled = m->ntiles > 1;
  if (!tiled && (n < 1 || !x || !y || !layer)) { msom_set_error("msomn_floats_begin: n = %d, x, y or layer null", n); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msomn_floats_begin before msomn_set_const"); return MSOM_ERR_STATE; }
  // the arrays on the host, for the checks
  std::vector<double> hx, hy;
  std::vector<int> hl;
  if (n >= 1 && x && y && layer) {
    if (is_device_ptr(x)) { hx.resize(n); HIPCHK(hipMemcpy(hx.data(), x, n * sizeof(double), hipMemcpyDeviceToHost)); x = hx.data(); }
    if (is_device_ptr(y)) { hy.resize(n); HIPCHK(hipMemcpy(hy.data(), y, n * sizeof(double), hipMemcpyDeviceToHost)); y = hy.data(); }
    if (is_device_ptr(layer)) { hl.resize(n); HIPCHK(hipMemcpy(hl.data(), layer, n * sizeof(int), hipMemcpyDeviceToHost)); layer = hl.data(); }
  }
  r = nfl_check(m, n, x, y, layer);
  if (tiled) {
    // the messages of a pass have a size that follows from n: ranks that do not pass the same n, or of which one refuses its
    // arrays, all leave here, before a float message is posted.  One reduction: max n, max -n, +inf from a rank that refuses
    const double mine[2] = {r ? (double)INFINITY : (double)n, r ? (double)INFINITY : -(double)n};
    HIPCHK(hipMemcpyAsync(m->d_scal + NSC_FLOATS, mine, sizeof mine, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    if (int rr = nt_reduce(m, NSC_FLOATS, 2, RED_MAX)) return rr;
    const double hi = m->h_scal[NSC_FLOATS], lo = -m->h_scal[NSC_FLOATS + 1];
    if (!r && hi != lo) {
      if (std::isfinite(hi)) msom_set_error("msomn_floats_begin: n = %d here, %g .. %g over the ranks: every rank passes the same floats", n, lo, hi);
      else msom_set_error("msomn_floats_begin: another rank refuses its arguments");
      return MSOM_ERR_ARG;
    }
  }
  if (r) return r;
  NFloatsState *s = new NFloatsState;
  s->n = n;
  s->tiled = tiled;
  const size_t nb = n * sizeof(double);
  bool ok = hipMalloc(&s->buf, 6 * nb) == hipSuccess && hipMalloc(&s->layer, n * sizeof(int)) == hipSuccess &&
            hipMalloc(&s->cnt, NFC_COUNT * sizeof(unsigned long long)) == hipSuccess;
  if (ok && tiled) {
    // a message carries the floats that cross one edge of the tile in one stage: with a CFL-limited step those within a fraction of
    // a cell of the edge, n / N or so of a uniform cloud; a sixteenth of all floats leaves room for a front, 1024 for small n
    s->K = m->floats_msg_cap > 0 ? m->floats_msg_cap : std::min(n, std::max(1024, n / 16));
    ok = hipMalloc(&s->id, n * sizeof(int)) == hipSuccess && hipMalloc(&s->live, n * sizeof(int)) == hipSuccess &&
         hipMalloc(&s->ctl, 4 * sizeof(int)) == hipSuccess && hipMalloc(&s->freest, n * sizeof(int)) == hipSuccess &&
         hipMalloc(&s->msg, 8 * nfl_msgcount(s) * sizeof(double)) == hipSuccess && hipMalloc(&s->gs, 3 * nb) == hipSuccess &&
         hipMalloc(&s->gr, (size_t)m->ntiles * 3 * nb) == hipSuccess && hipMalloc(&s->dsum, NFC_COUNT * sizeof(double)) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    nfl_free(s);
    msom_set_error("msomn_floats_begin: no device memory for %d floats", n);
    return MSOM_ERR_HIP;
  }
  nfloats_drop(m);   // a second begin replaces the first
  m->floats = s;
  m->floats_on = 1;
  HIPCHK(hipMemsetAsync(s->buf, 0, 6 * nb, m->st));
  HIPCHK(hipMemsetAsync(s->cnt, 0, NFC_COUNT * sizeof(unsigned long long), m->st));
  std::vector<double> tx, ty;
  std::vector<int> tl, tid;
  int nmine = n;
  if (tiled) {   // the floats this rank owns, in the first slots.  The host locates with the kernels' own function (no contraction
                 // in nfloats_axis, in either build): every float starts on the rank the kernels take for its owner, no pass is needed
    const FloatsGeom fg = nfl_geom(m);
    const FloatsTiling t = nfl_tiling(m);
    for (int k = 0; k < n; k++) {
      int col, row;
      nfloats_owner(nfloats_locate(x[k], y[k], fg), t, &col, &row);
      if (col != t.ix || row != t.iy) continue;
      tx.push_back(x[k]); ty.push_back(y[k]); tl.push_back(layer[k]); tid.push_back(k);
    }
    nmine = (int)tid.size();
    x = tx.data(); y = ty.data(); layer = tl.data();
    const int ctl[4] = {nmine, 0, 0, 0};
    std::vector<int> live(n, 0);
    std::fill(live.begin(), live.begin() + nmine, 1);
    HIPCHK(hipMemsetAsync(s->layer, 0, n * sizeof(int), m->st));
    HIPCHK(hipMemsetAsync(s->id, 0, n * sizeof(int), m->st));
    HIPCHK(hipMemsetAsync(s->freest, 0, n * sizeof(int), m->st));
    HIPCHK(hipMemsetAsync(s->msg, 0, 8 * nfl_msgcount(s) * sizeof(double), m->st));
    HIPCHK(hipMemcpyAsync(s->ctl, ctl, sizeof ctl, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(s->live, live.data(), n * sizeof(int), hipMemcpyHostToDevice, m->st));
    if (nmine) HIPCHK(hipMemcpyAsync(s->id, tid.data(), nmine * sizeof(int), hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));   // live goes out of scope
  }
  if (nmine) {
    HIPCHK(hipMemcpyAsync(s->buf, x, nmine * sizeof(double), hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(s->buf + n, y, nmine * sizeof(double), hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(s->layer, layer, nmine * sizeof(int), hipMemcpyHostToDevice, m->st));
  }
  return nfl_sync(m);   // the host copies go out of scope
}

extern "C" int msomn_floats_end(msomn_t *m) {
  int r = nfl_guard(m, "msomn_floats_end", false);
  if (r) return r;
  nfloats_drop(m);
  return MSOM_OK;
}

extern "C" int msomn_floats_get(msomn_t *m, double *x, double *y) {
  int r = nfl_guard(m, "msomn_floats_get", true);
  if (r) return r;
  if (!x || !y) { msom_set_error("msomn_floats_get: null array"); return MSOM_ERR_ARG; }
  const NFloatsState *s = m->floats;
  if (s->tiled) {
    HIPCHK(hipMemsetAsync(s->gs, 0, 3 * (size_t)s->n * sizeof(double), m->st));
    launch_floats_scatter(m->st, s->buf, s->buf + s->n, nfl_tile(m, s), s->n, s->gs);
    if ((r = nfl_combine(m, s->gs, x, y))) return r;
    return nfl_sync(m);
  }
  HIPCHK(hipMemcpyAsync(x, s->buf, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(y, s->buf + s->n, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return nfl_sync(m);
}

// velocity and sample on tiles: each float on its owner, which between a stage 1 and its stage 2 is the owner of (xh, yh), not of (x, y)
static int nfl_tiled_interp(msomn *m, const char *fn, const double *f, const double *pg, bool vel, double *u0, double *u1) {
  const NFloatsState *s = m->floats;
  if (s->staged) { msom_set_error("%s: on tiles not between a stage 1 and its stage 2", fn); return MSOM_ERR_STATE; }
  const FloatsTileDev td = nfl_tile(m, s);
  HIPCHK(hipMemsetAsync(s->gs, 0, 3 * (size_t)s->n * sizeof(double), m->st));
  launch_nfloats_interp(m->st, nfl_dev(s), s->n, f, pg, m->g, nfl_geom(m), s->gs, vel ? s->gs : nullptr, &td);
  HIPCHK(hipGetLastError());
  if (int r = nfl_combine(m, s->gs, u0, u1)) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_velocity(msomn_t *m, double *u, double *v) {
  int r = nfl_guard(m, "msomn_floats_velocity", true);
  if (r) return r;
  if (!u || !v) { msom_set_error("msomn_floats_velocity: null array"); return MSOM_ERR_ARG; }
  const NFloatsState *s = m->floats;
  if (s->tiled) return nfl_tiled_interp(m, "msomn_floats_velocity", m->f[MSOMN_PSI], nfl_pg(m), true, u, v);
  double *o0 = s->buf + 4 * (size_t)s->n, *o1 = o0 + s->n;
  launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[MSOMN_PSI], nfl_pg(m), m->g, nfl_geom(m), o0, o1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(u, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(v, o1, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return nfl_sync(m);
}

extern "C" int msomn_floats_sample(msomn_t *m, int field, double *out) {
  int r = nfl_guard(m, "msomn_floats_sample", true);
  if (r || (r = nfl_field(m, "msomn_floats_sample", field))) return r;
  if (!out) { msom_set_error("msomn_floats_sample: null array"); return MSOM_ERR_ARG; }
  const NFloatsState *s = m->floats;
  if (s->tiled) return nfl_tiled_interp(m, "msomn_floats_sample", m->f[field], nullptr, false, out, nullptr);
  double *o0 = s->buf + 4 * (size_t)s->n;
  launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[field], nullptr, m->g, nfl_geom(m), o0, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return nfl_sync(m);
}

extern "C" int msomn_floats_stage(msomn_t *m, int stage, double dt) {
  int r = nfl_guard(m, "msomn_floats_stage", true);
  if (r) return r;
  if ((stage != 1 && stage != 2) || !std::isfinite(dt)) { msom_set_error("msomn_floats_stage: stage %d, dt = %g", stage, dt); return MSOM_ERR_ARG; }
  NFloatsState *s = m->floats;
  if (stage == 2 && !s->staged) { msom_set_error("msomn_floats_stage: stage 2 without a stage 1 before it"); return MSOM_ERR_STATE; }
  if ((r = nfl_stage(m, stage, dt, nullptr))) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_record(msomn_t *m, int every, int capacity, int field) {
  int r = nfl_guard(m, "msomn_floats_record", true);
  if (r) return r;
  if (every < 1 || capacity < 1) { msom_set_error("msomn_floats_record: every = %d, capacity = %d", every, capacity); return MSOM_ERR_ARG; }
  if (field >= 0 && (r = nfl_field(m, "msomn_floats_record", field))) return r;
  NFloatsState *s = m->floats;
  if (s->tiled && field >= 0 && s->staged) {   // record 0 samples the field at (x, y), on the owner of (x, y)
    msom_set_error("msomn_floats_record: on tiles a field is not recorded from between a stage 1 and its stage 2");
    return MSOM_ERR_STATE;
  }
  HIPCHK(hipStreamSynchronize(m->st));   // a stage may still be writing a record
  double *rec = nullptr;
  const size_t rows = s->tiled ? (field < 0 ? 3 : 6) : (field < 0 ? 2 : 3);
  HIPCHK(hipMalloc(&rec, (size_t)capacity * rows * s->n * sizeof(double)));
  if (s->rec) (void)hipFree(s->rec);
  s->rec = rec;
  s->every = every;
  s->cap = capacity;
  s->field = field < 0 ? -1 : field;
  s->nrec = 1;
  s->steps = s->dropped = 0;
  s->t.assign(1, m->t);
  // record 0: x then y, as they lie, and the sample of the field at them; on tiles by id, as the later ones are written
  if (s->tiled) {
    const FloatsTileDev td = nfl_tile(m, s);
    HIPCHK(hipMemsetAsync(rec, 0, rows * s->n * sizeof(double), m->st));
    launch_floats_scatter(m->st, s->buf, s->buf + s->n, td, s->n, rec);
    if (field >= 0) launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[field], nullptr, m->g, nfl_geom(m), rec + 3 * (size_t)s->n, nullptr, &td);
    HIPCHK(hipGetLastError());
    return nfl_sync(m);
  }
  HIPCHK(hipMemcpyAsync(rec, s->buf, 2 * (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, m->st));
  if (field >= 0) {
    launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[field], nullptr, m->g, nfl_geom(m), rec + 2 * (size_t)s->n, nullptr);
    HIPCHK(hipGetLastError());
  }
  return nfl_sync(m);
}

extern "C" int msomn_floats_track(msomn_t *m, int first, int count, double *t, double *x, double *y, double *val) {
  int r = nfl_guard(m, "msomn_floats_track", true);
  if (r) return r;
  const NFloatsState *s = m->floats;
  if (!s->rec) { msom_set_error("msomn_floats_track: no msomn_floats_record since msomn_floats_begin"); return MSOM_ERR_STATE; }
  if (first < 0 || count < 1 || first > s->nrec - count) {
    msom_set_error("msomn_floats_track: records %d .. %d of %d", first, first + count - 1, s->nrec);
    return MSOM_ERR_ARG;
  }
  if (val && s->field < 0) { msom_set_error("msomn_floats_track: val given, but msomn_floats_record chose no field"); return MSOM_ERR_ARG; }
  for (int k = 0; t && k < count; k++) t[k] = s->t[first + k];
  const size_t n = s->n, nb = n * sizeof(double), rs = nfl_rows(s);
  const double *src = s->rec + (size_t)first * rs * n;
  if (s->tiled) {   // every record is combined over the ranks the way msomn_floats_get combines the positions; so is its value.
                    // Every rank makes the same gathers: the arrays a rank leaves out change nothing in them
    for (int k = 0; k < count; k++) {
      const double *rk = src + (size_t)k * rs * n;
      if ((r = nfl_combine(m, rk, x ? x + k * n : nullptr, y ? y + k * n : nullptr))) return r;
      if (s->field >= 0 && (r = nfl_combine(m, rk + 3 * n, val ? val + k * n : nullptr, nullptr))) return r;
    }
    return nfl_sync(m);
  }
  if (x) HIPCHK(hipMemcpy2DAsync(x, nb, src, rs * nb, nb, count, hipMemcpyDefault, m->st));
  if (y) HIPCHK(hipMemcpy2DAsync(y, nb, src + n, rs * nb, nb, count, hipMemcpyDefault, m->st));
  if (val) HIPCHK(hipMemcpy2DAsync(val, nb, src + 2 * n, rs * nb, nb, count, hipMemcpyDefault, m->st));
  return nfl_sync(m);
}
