// msom_floats.hip -- Lagrangian floats advected with the model's RK2 stages (include/msom_floats.h): the
// msom_floats_* entry points and the hook rk_stage calls behind each of its two tendency passes.  Arithmetic: floats_inl.h; kernels:
// kernels_floats.hip.  On tiles (option floats_tiles, "On tiles" in section 8k) every call is collective: each rank holds the floats
// it owns in n slots, a migration pass behind every stage kernel takes them to their new owner, readouts are combined over the ranks.
#include "msom_host.h"

#include "../../include/msom_floats.h"

struct FloatsState {
  int n = 0;
  double *buf = nullptr;               // x, y, xh, yh and two output arrays of the by-hand calls, n doubles each
  int *layer = nullptr;
  unsigned long long *cnt = nullptr;   // clamped, lost
  int staged = 0;                      // a stage 1 since msom_floats_begin or the last stage 2
  // trajectory buffer [cap][2][n]; times on the host
  double *rec = nullptr;
  int every = 1, cap = 0, nrec = 0;
  long steps = 0, dropped = 0;         // stage-2 hooks seen since msom_floats_record; records that found the buffer full
  std::vector<double> t;
  // on tiles (option floats_tiles, more than one rank): the arrays above are n slots of which this rank fills those of the floats it
  // owns; records are [cap][3][n], indexed by id, with a presence word
  int tiled = 0, K = 0;                // K: records a message can carry (option floats_msg_cap)
  int *id = nullptr, *live = nullptr;
  int *ctl = nullptr;                  // high-water mark, free slots, records taken in the lo / hi message of the running phase
  int *freest = nullptr;               // free stack
  double *msg = nullptr;               // send W E S N, receive W E S N: 1 + 6 K doubles each
  double *gs = nullptr, *gr = nullptr; // readouts: this rank's [3][n] by id, all ranks' [nranks][3][n]
  double *dsum = nullptr;              // the four counters as doubles, for the sum over the ranks
};

static FloatsDev fl_dev(const FloatsState *s) {
  return FloatsDev{s->buf, s->buf + s->n, s->buf + 2 * (size_t)s->n, s->buf + 3 * (size_t)s->n, s->layer, s->cnt};
}
static FloatsGeom fl_geom(const msom *m) {
  return FloatsGeom{m->gnx, m->gny, m->bc == BC_PERIODIC, m->gnx / m->p.L0, m->p.L0, m->p.L0 * m->gny / m->gnx};
}
static FloatsTiling fl_tiling(const msom *m) { return FloatsTiling{m->px, m->py, m->ix, m->iy, m->nx, m->ny}; }
static FloatsTileDev fl_tile(const msom *m, const FloatsState *s) { return FloatsTileDev{s->id, s->live, s->ctl, m->ix * m->nx, m->iy * m->ny}; }
static FloatsMig fl_mig(const FloatsState *s) {
  const size_t n = s->n;
  return FloatsMig{s->buf, s->buf + n, s->buf + 2 * n, s->buf + 3 * n, s->layer, s->id, s->live, s->ctl, s->ctl + 1, s->freest, s->ctl + 2, s->cnt};
}
static size_t fl_msgcount(const FloatsState *s) { return 1 + 6 * (size_t)s->K; }
static const double *fl_pg(const msom *m) { return m->have_pg ? m->f[MSOM_PSIPG] : nullptr; }
static void fl_free(FloatsState *s) {
  if (!s) return;
  if (s->buf) hipFree(s->buf);
  if (s->layer) hipFree(s->layer);
  if (s->cnt) hipFree(s->cnt);
  if (s->rec) hipFree(s->rec);
  for (void *p : {(void *)s->id, (void *)s->live, (void *)s->ctl, (void *)s->freest, (void *)s->msg, (void *)s->gs, (void *)s->gr, (void *)s->dsum})
    if (p) hipFree(p);
  delete s;
}

void floats_drop(msom *m) {
  if (!m->fl) return;
  hipStreamSynchronize(m->st);   // a stage may still be running
  if (m->st2) hipStreamSynchronize(m->st2);
  fl_free(m->fl);
  m->fl = nullptr;
  m->fl_on = 0;
}

// The migration pass behind a stage kernel (tiles): two phases in exch_nat's order, W / E, then S / N over all residents, arrivals of
// the first phase included, so a diagonal move needs no diagonal message.  Every rank posts every message of the fixed count
// 1 + 6 K, with or without emigrants: nothing is read on the host.  half: the floats are homed by (xh, yh), what stage 2 evaluates
static int fl_migrate(msom *m, int half) {
  FloatsState *s = m->fl;
  const size_t mc = fl_msgcount(s);
  const FloatsMig mg = fl_mig(s);
  const FloatsGeom fg = fl_geom(m);
  const FloatsTiling tl = fl_tiling(m);
  hipStream_t cs = m->st2;
  int r = MSOM_OK;
  comm_begin(m);
  for (int ph = 0; ph < 2 && !r; ph++) {
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
    if (nx) {
      prof_begin(m, m->prof_floats_emig, cs);
      launch_floats_emigrate(cs, mg, s->n, fg, tl, ph, half, sb[0], sb[1], s->K);
      prof_end(m, m->prof_floats_emig, cs);
    }
    r = comm_exchange(m->comm, x, nx);
    if (!r && nx) {
      prof_begin(m, m->prof_floats_immig, cs);
      launch_floats_immigrate(cs, mg, s->n, m->nl, rb[0], rb[1], s->K);
      prof_end(m, m->prof_floats_immig, cs);
    }
  }
  comm_end(m);
  return r;
}

void floats_hook(msom *m, int stage, double tnext) {
  FloatsState *s = m->fl;
  double *rec = nullptr;
  const size_t rs = (s->tiled ? 3 : 2) * (size_t)s->n;
  if (stage == 2 && s->rec && ++s->steps % s->every == 0) {
    if (s->nrec < s->cap) {
      rec = s->rec + (size_t)s->nrec++ * rs;
      s->t.push_back(tnext);
    } else
      s->dropped++;
  }
  if (s->tiled && rec) hipMemsetAsync(rec, 0, rs * sizeof(double), m->st);   // the presence words
  if (s->tiled && stage == 1 && s->staged) STICKY(m, fl_migrate(m, 0));      // a stage 1 by hand without its stage 2: home by (x, y) again
  const FloatsTileDev td = s->tiled ? fl_tile(m, s) : FloatsTileDev{};
  prof_begin(m, m->prof_floats);
  launch_floats_stage(m->st, stage, fl_dev(s), s->n, m->f[MSOM_PSI], fl_pg(m), m->g, fl_geom(m), m->dt, rec, s->tiled ? &td : nullptr);
  prof_end(m, m->prof_floats);
  s->staged = stage == 1;
  if (s->tiled) STICKY(m, fl_migrate(m, stage == 1));
}

// readouts on tiles: send [3][n] by id with its presence words -> the values of every id, taken from the rank that holds it, in the
// two output arrays behind the slots; then to the caller's u0, u1 (host or device, u1 may be null)
static int fl_combine(msom *m, const double *send, double *u0, double *u1) {
  FloatsState *s = m->fl;
  const size_t n = s->n;
  double *o0 = s->buf + 4 * n, *o1 = o0 + n;
  comm_begin(m);
  const int r = comm_allgather(m->comm, send, s->gr, 3 * n);
  if (!r) launch_floats_select(m->st2, s->gr, m->nranks, s->n, o0, o1);
  comm_end(m);
  if (r) return r;
  if (u0) HIPCHK(hipMemcpyAsync(u0, o0, n * sizeof(double), hipMemcpyDefault, m->st));
  if (u1) HIPCHK(hipMemcpyAsync(u1, o1, n * sizeof(double), hipMemcpyDefault, m->st));
  return MSOM_OK;
}

bool floats_param(msom *m, const char *key, double *v) {
  if (strncmp(key, "floats", 6)) return false;
  const FloatsState *s = m->fl;
  const char *k = key + 6;
  if (!*k) *v = s ? s->n : 0;
  else if (!strcmp(k, "_records")) *v = s ? s->nrec : 0;
  else if (!strcmp(k, "_dropped")) *v = s ? (double)s->dropped : 0;
  else if (!strcmp(k, "_tiles")) *v = m->fl_tiles;
  else if (!strcmp(k, "_msg_cap")) *v = s && s->tiled ? s->K : m->fl_msg_cap;
  else if (!strcmp(k, "_resident")) {   // the rank's own: slots below the mark that are not on the free stack
    int c[2] = {s ? s->n : 0, 0};
    if (s && s->tiled && (hipStreamSynchronize(m->st) != hipSuccess || hipMemcpy(c, s->ctl, sizeof c, hipMemcpyDeviceToHost) != hipSuccess)) { *v = NAN; return true; }
    *v = c[0] - c[1];
  } else if (!strcmp(k, "_clamped") || !strcmp(k, "_lost") || !strcmp(k, "_unsent") || !strcmp(k, "_migrated")) {
    unsigned long long c[4] = {0, 0, 0, 0};
    if (s && (hipStreamSynchronize(m->st) != hipSuccess || hipMemcpy(c, s->cnt, sizeof c, hipMemcpyDeviceToHost) != hipSuccess)) { *v = NAN; return true; }
    double h[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
    if (s && s->tiled) {   // collective: the sum over the ranks (whole numbers far below 2^53: exact in any order)
      if (hipMemcpy(s->dsum, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) { *v = NAN; return true; }
      comm_begin(m);
      const int r = comm_allreduce(m->comm, s->dsum, h, 4, RED_SUM);
      comm_end(m);
      if (r) { *v = NAN; return true; }
    }
    *v = h[k[1] == 'c' ? 0 : k[1] == 'l' ? 1 : k[1] == 'u' ? 2 : 3];
  } else
    return false;
  return true;
}

// what every call checks first: the dialect, the handle, one rank or option floats_tiles; need: floats begun
static int fl_guard(msom *m, const char *fn, bool need) {
  if (!m) { msom_set_error("%s: null handle", fn); return MSOM_ERR_ARG; }
  if (m->nranks > 1 && !m->fl_tiles) { msom_set_error("%s: floats that cross tiles are not supported (%d ranks)", fn, m->nranks); return MSOM_ERR_CONFIG; }
  if (need && !m->fl) { msom_set_error("%s: no msom_floats_begin since msom_set_const", fn); return MSOM_ERR_STATE; }
  return MSOM_OK;
}

extern "C" int msom_floats_begin(msom_t *m, int n, const double *x, const double *y, const int *layer) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_begin", false);
  if (r) return r;
  if (n < 1 || !x || !y || !layer) { msom_set_error("msom_floats_begin: n = %d, x, y or layer null", n); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msom_floats_begin before msom_set_const"); return MSOM_ERR_STATE; }
  // the arrays on the host, for the checks
  std::vector<double> hx, hy;
  std::vector<int> hl;
  if (is_device_ptr(x)) { hx.resize(n); HIPCHK(hipMemcpy(hx.data(), x, n * sizeof(double), hipMemcpyDeviceToHost)); x = hx.data(); }
  if (is_device_ptr(y)) { hy.resize(n); HIPCHK(hipMemcpy(hy.data(), y, n * sizeof(double), hipMemcpyDeviceToHost)); y = hy.data(); }
  if (is_device_ptr(layer)) { hl.resize(n); HIPCHK(hipMemcpy(hl.data(), layer, n * sizeof(int), hipMemcpyDeviceToHost)); layer = hl.data(); }
  const FloatsGeom fg = fl_geom(m);
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(x[k]) || !std::isfinite(y[k])) { msom_set_error("msom_floats_begin: float %d at (%g, %g)", k, x[k], y[k]); return MSOM_ERR_ARG; }
    if (!fg.periodic && !(x[k] >= 0 && x[k] <= fg.Lx && y[k] >= 0 && y[k] <= fg.Ly)) {
      msom_set_error("msom_floats_begin: float %d at (%g, %g) outside [0, %g] x [0, %g]", k, x[k], y[k], fg.Lx, fg.Ly);
      return MSOM_ERR_ARG;
    }
    if (layer[k] < 0 || layer[k] >= m->nl) { msom_set_error("msom_floats_begin: float %d in layer %d of %d", k, layer[k], m->nl); return MSOM_ERR_ARG; }
  }
  FloatsState *s = new FloatsState;
  s->n = n;
  s->tiled = m->nranks > 1;
  const size_t nb = n * sizeof(double);
  bool ok = hipMalloc(&s->buf, 6 * nb) == hipSuccess && hipMalloc(&s->layer, n * sizeof(int)) == hipSuccess &&
            hipMalloc(&s->cnt, 4 * sizeof(unsigned long long)) == hipSuccess;
  if (ok && s->tiled) {
    // a message carries the floats that cross one edge of the tile in one stage: with a CFL-limited step those within a fraction of
    // a cell of the edge, n / tnx or so of a uniform cloud; a sixteenth of all floats leaves room for a front, 1024 for small n
    s->K = m->fl_msg_cap > 0 ? m->fl_msg_cap : std::min(n, std::max(1024, n / 16));
    ok = hipMalloc(&s->id, n * sizeof(int)) == hipSuccess && hipMalloc(&s->live, n * sizeof(int)) == hipSuccess &&
         hipMalloc(&s->ctl, 4 * sizeof(int)) == hipSuccess && hipMalloc(&s->freest, n * sizeof(int)) == hipSuccess &&
         hipMalloc(&s->msg, 8 * fl_msgcount(s) * sizeof(double)) == hipSuccess && hipMalloc(&s->gs, 3 * nb) == hipSuccess &&
         hipMalloc(&s->gr, (size_t)m->nranks * 3 * nb) == hipSuccess && hipMalloc(&s->dsum, 4 * sizeof(double)) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    fl_free(s);
    msom_set_error("msom_floats_begin: no device memory for %d floats", n);
    return MSOM_ERR_HIP;
  }
  floats_drop(m);   // a second begin replaces the first
  m->fl = s;
  m->fl_on = 1;
  HIPCHK(hipMemsetAsync(s->buf, 0, 6 * nb, m->st));
  HIPCHK(hipMemsetAsync(s->cnt, 0, 4 * sizeof(unsigned long long), m->st));
  std::vector<double> tx, ty;
  std::vector<int> tl, tid;
  int nmine = n;
  if (s->tiled) {   // the floats this rank owns, in the first slots
    const FloatsTiling t = fl_tiling(m);
    for (int k = 0; k < n; k++) {
      int col, row;
      floats_owner(floats_locate(x[k], y[k], fg), t, &col, &row);
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
    HIPCHK(hipMemsetAsync(s->msg, 0, 8 * fl_msgcount(s) * sizeof(double), m->st));
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
  // The host formed x * idx - 0.5 with two roundings; the product build's kernels fuse it.  A float within an ulp of a cell-centre line
  // may thus belong to the neighbour in the kernels' eyes: one pass by their own rule takes it there (and counts it in floats_migrated)
  if (s->tiled && (r = fl_migrate(m, 0))) return r;
  return sync_stream(m);   // the host copies go out of scope
}

extern "C" int msom_floats_end(msom_t *m) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_end", false);
  if (r) return r;
  floats_drop(m);
  return MSOM_OK;
}

extern "C" int msom_floats_get(msom_t *m, double *x, double *y) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_get", true);
  if (r) return r;
  if (!x || !y) { msom_set_error("msom_floats_get: null array"); return MSOM_ERR_ARG; }
  const FloatsState *s = m->fl;
  if (s->tiled) {
    HIPCHK(hipMemsetAsync(s->gs, 0, 3 * (size_t)s->n * sizeof(double), m->st));
    launch_floats_scatter(m->st, s->buf, s->buf + s->n, fl_tile(m, s), s->n, s->gs);
    if ((r = fl_combine(m, s->gs, x, y))) return r;
    return sync_stream(m);
  }
  HIPCHK(hipMemcpyAsync(x, s->buf, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(y, s->buf + s->n, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

// velocity and sample on tiles: each float on its owner, which between a stage 1 and its stage 2 is the owner of (xh, yh), not of (x, y)
static int fl_tiled_interp(msom *m, const char *fn, const double *f, const double *pg, bool vel, double *u0, double *u1) {
  const FloatsState *s = m->fl;
  if (s->staged) { msom_set_error("%s: on tiles not between a stage 1 and its stage 2", fn); return MSOM_ERR_STATE; }
  const FloatsTileDev td = fl_tile(m, s);
  HIPCHK(hipMemsetAsync(s->gs, 0, 3 * (size_t)s->n * sizeof(double), m->st));
  launch_floats_interp(m->st, fl_dev(s), s->n, f, pg, m->g, fl_geom(m), s->gs, vel ? s->gs : nullptr, &td);
  return fl_combine(m, s->gs, u0, u1);
}

extern "C" int msom_floats_velocity(msom_t *m, double *u, double *v) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_velocity", true);
  if (r) return r;
  if (!u || !v) { msom_set_error("msom_floats_velocity: null array"); return MSOM_ERR_ARG; }
  const FloatsState *s = m->fl;
  double *o0 = s->buf + 4 * (size_t)s->n, *o1 = o0 + s->n;
  if (s->tiled) {
    if ((r = fl_tiled_interp(m, "msom_floats_velocity", m->f[MSOM_PSI], fl_pg(m), true, u, v))) return r;
    return sync_stream(m);
  }
  launch_floats_interp(m->st, fl_dev(s), s->n, m->f[MSOM_PSI], fl_pg(m), m->g, fl_geom(m), o0, o1);
  HIPCHK(hipMemcpyAsync(u, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(v, o1, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

// a field of nl layers that the handle holds
static int fl_field(msom *m, const char *fn, int field) {
  if (field < 0 || field >= MSOM_NFIELDS || !m->f[field] || m->flayers[field] != m->nl) {
    msom_set_error("%s: field id %d is not a field of %d layers of this handle", fn, field, m->nl);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}

extern "C" int msom_floats_sample(msom_t *m, int field, double *out) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_sample", true);
  if (r || (r = fl_field(m, "msom_floats_sample", field))) return r;
  if (!out) { msom_set_error("msom_floats_sample: null array"); return MSOM_ERR_ARG; }
  const FloatsState *s = m->fl;
  double *o0 = s->buf + 4 * (size_t)s->n;
  if (s->tiled) {
    if ((r = fl_tiled_interp(m, "msom_floats_sample", m->f[field], nullptr, false, out, nullptr))) return r;
    return sync_stream(m);
  }
  launch_floats_interp(m->st, fl_dev(s), s->n, m->f[field], nullptr, m->g, fl_geom(m), o0, nullptr);
  HIPCHK(hipMemcpyAsync(out, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

extern "C" int msom_floats_stage(msom_t *m, int stage, double dt) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_stage", true);
  if (r) return r;
  if ((stage != 1 && stage != 2) || !std::isfinite(dt)) { msom_set_error("msom_floats_stage: stage %d, dt = %g", stage, dt); return MSOM_ERR_ARG; }
  FloatsState *s = m->fl;
  if (stage == 2 && !s->staged) { msom_set_error("msom_floats_stage: stage 2 without a stage 1 before it"); return MSOM_ERR_STATE; }
  const FloatsTileDev td = s->tiled ? fl_tile(m, s) : FloatsTileDev{};
  if (s->tiled && stage == 1 && s->staged && (r = fl_migrate(m, 0))) return r;   // a second stage 1: home by (x, y) again
  launch_floats_stage(m->st, stage, fl_dev(s), s->n, m->f[MSOM_PSI], fl_pg(m), m->g, fl_geom(m), dt, nullptr, s->tiled ? &td : nullptr);
  s->staged = stage == 1;
  if (s->tiled && (r = fl_migrate(m, stage == 1))) return r;
  return sync_stream(m);
}

extern "C" int msom_floats_record(msom_t *m, int every, int capacity) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_record", true);
  if (r) return r;
  if (every < 1 || capacity < 1) { msom_set_error("msom_floats_record: every = %d, capacity = %d", every, capacity); return MSOM_ERR_ARG; }
  FloatsState *s = m->fl;
  HIPCHK(hipStreamSynchronize(m->st));   // a stage may still be writing a record
  double *rec = nullptr;
  const size_t rs = (s->tiled ? 3 : 2) * (size_t)s->n;
  HIPCHK(hipMalloc(&rec, (size_t)capacity * rs * sizeof(double)));
  if (s->rec) hipFree(s->rec);
  s->rec = rec;
  s->every = every;
  s->cap = capacity;
  s->nrec = 1;
  s->steps = s->dropped = 0;
  s->t.assign(1, m->t);
  if (s->tiled) {   // record 0 by id, as the stage-2 kernel writes the later ones
    HIPCHK(hipMemsetAsync(rec, 0, rs * sizeof(double), m->st));
    launch_floats_scatter(m->st, s->buf, s->buf + s->n, fl_tile(m, s), s->n, rec);
  } else
    HIPCHK(hipMemcpyAsync(rec, s->buf, 2 * (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, m->st));   // record 0: x then y, as they lie
  return sync_stream(m);
}

extern "C" int msom_floats_track(msom_t *m, int first, int count, double *t, double *x, double *y) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_track", true);
  if (r) return r;
  const FloatsState *s = m->fl;
  if (!s->rec) { msom_set_error("msom_floats_track: no msom_floats_record since msom_floats_begin"); return MSOM_ERR_STATE; }
  if (first < 0 || count < 1 || first > s->nrec - count) {
    msom_set_error("msom_floats_track: records %d .. %d of %d", first, first + count - 1, s->nrec);
    return MSOM_ERR_ARG;
  }
  for (int k = 0; t && k < count; k++) t[k] = s->t[first + k];
  if (s->tiled) {   // every record is combined over the ranks the way msom_floats_get combines the positions
    for (int k = 0; k < count; k++)
      if ((r = fl_combine(m, s->rec + (size_t)(first + k) * 3 * s->n, x ? x + (size_t)k * s->n : nullptr, y ? y + (size_t)k * s->n : nullptr))) return r;
    return sync_stream(m);
  }
  const size_t nb = s->n * sizeof(double);
  const double *src = s->rec + (size_t)first * 2 * s->n;
  if (x) HIPCHK(hipMemcpy2DAsync(x, nb, src, 2 * nb, nb, count, hipMemcpyDefault, m->st));
  if (y) HIPCHK(hipMemcpy2DAsync(y, nb, src + s->n, 2 * nb, nb, count, hipMemcpyDefault, m->st));
  return sync_stream(m);
}

extern "C" int msom_floats_dbg_ghosted(msom_t *m, int field, double *out) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_dbg_ghosted", false);
  if (r || (r = fl_field(m, "msom_floats_dbg_ghosted", field))) return r;
  if (!out) { msom_set_error("msom_floats_dbg_ghosted: null array"); return MSOM_ERR_ARG; }
  const size_t w = (size_t)(m->nx + 2) * sizeof(double), h = m->ny + 2;
  for (int l = 0; l < m->nl; l++)
    HIPCHK(hipMemcpy2DAsync(out + (size_t)l * h * (m->nx + 2), w, m->f[field] + nat_idx(m->g, l, -1, -1), m->g.pitch * sizeof(double), w, h,
                            hipMemcpyDefault, m->st));
  return sync_stream(m);
}
