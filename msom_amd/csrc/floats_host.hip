// floats_host.hip -- the host side of the Lagrangian floats of both models (floats_host.h).  Arithmetic and owner rules: floats_inl.h;
// kernels: kernels_floats.hip, kernels_node_floats.hip.
#include "floats_host.h"

#include <string.h>

#include <algorithm>
#include <cmath>

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e__ = (x);                                                                  \
    if (e__ != hipSuccess) {                                                               \
      msom_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e__), __FILE__, __LINE__, #x); \
      return MSOM_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)

bool is_device_ptr(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // an address the runtime does not know: host
  return a.type == hipMemoryTypeDevice;
}

namespace fh {

void free_state(State *s) {
  if (!s) return;
  for (void *p : {(void *)s->buf, (void *)s->layer, (void *)s->cnt, (void *)s->rec, (void *)s->id, (void *)s->live, (void *)s->ctl, (void *)s->freest,
                  (void *)s->msg, (void *)s->gs, (void *)s->gr, (void *)s->dsum})
    if (p) (void)hipFree(p);
  delete s;
}

int set_option(Opts &o, const char *key, double v) {
  if (!strcmp(key, "floats")) o.on = o.s && (int)v != 0;   // pauses / resumes the floats of the model's step; without floats: nothing
  else if (!strcmp(key, "floats_tiles")) o.tiles = (int)v != 0;   // before begin, alike on all ranks
  else if (!strcmp(key, "floats_msg_cap")) {
    if (!(v >= 0) || v > 1e8) { msom_set_error("option floats_msg_cap = %g", v); return MSOM_ERR_ARG; }
    o.msg_cap = (int)v;
  } else { msom_set_error("unknown option %s", key); return MSOM_ERR_ARG; }
  return MSOM_OK;
}

static FloatsDev dev(const State *s) {
  const size_t n = s->n;
  return FloatsDev{s->buf, s->buf + n, s->buf + 2 * n, s->buf + 3 * n, s->layer, s->cnt};
}
static FloatsTileDev tile(const Ctx &c, const State *s) { return FloatsTileDev{s->id, s->live, s->ctl, c.ox, c.oy}; }
static FloatsMig mig(const State *s) {
  const size_t n = s->n;
  return FloatsMig{s->buf, s->buf + n, s->buf + 2 * n, s->buf + 3 * n, s->layer, s->id, s->live, s->ctl, s->ctl + 1, s->freest, s->ctl + 2, s->cnt};
}
static void bracket(const Ctx &c, bool open) { if (c.bracket) c.bracket(c.h, open); }
static void prof(const Ctx &c, int slot, bool begin, hipStream_t st) { if (c.prof) c.prof(c.h, slot, begin, st); }

int migrate(const Ctx &c, State *s, int half) {
  const size_t mc = s->msgcount();
  const FloatsMig mg = mig(s);
  int r = MSOM_OK;
  bracket(c, true);
  for (int ph = 0; ph < 2 && !r; ph++) {
    const int lo = ph ? DIR_S : DIR_W, hi = ph ? DIR_N : DIR_E;
    Xfer x[2];
    int nx = 0;
    double *sb[2] = {nullptr, nullptr}, *rb[2] = {nullptr, nullptr};
    for (int e = 0; e < 2; e++) {
      const int dir = e ? hi : lo;
      if (c.nb[dir] < 0) continue;
      sb[e] = s->msg + dir * mc;
      rb[e] = s->msg + (4 + dir) * mc;
      x[nx++] = {c.nb[dir], dir, sb[e], rb[e], mc};
    }
    if (nx) {
      prof(c, PROF_EMIGRATE, true, c.cst);
      launch_floats_emigrate(c.cst, mg, s->n, c.fg, c.tl, ph, half, sb[0], sb[1], s->K, c.node);
      prof(c, PROF_EMIGRATE, false, c.cst);
    }
    r = comm_exchange(c.comm, x, nx);
    if (!r && nx) {
      prof(c, PROF_IMMIGRATE, true, c.cst);
      launch_floats_immigrate(c.cst, mg, s->n, c.nl, rb[0], rb[1], s->K);
      prof(c, PROF_IMMIGRATE, false, c.cst);
    }
  }
  bracket(c, false);
  if (r) return r;
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

int stage(const Ctx &c, State *s, int stage, double dt, double *rec, bool timed) {
  const double *rf = rec ? c.rf : nullptr;
  const FloatsTileDev td = s->tiled ? tile(c, s) : FloatsTileDev{};
  int r;
  if (s->tiled && rec) HIPCHK(hipMemsetAsync(rec, 0, s->rows() * s->n * sizeof(double), c.st));   // the presence words
  if (s->tiled && stage == 1 && s->staged && (r = migrate(c, s, 0))) return r;   // a stage 1 without its stage 2: home by (x, y) again
  // on tiles the positions of a record are written by the rank the float is resident on, before the pass takes it elsewhere ...
  if (timed) prof(c, PROF_STAGE, true, c.st);
  c.stage(c.st, stage, dev(s), s->n, c.psi, c.pg, c.g, c.fg, dt, rec, s->tiled ? nullptr : rf, s->tiled ? &td : nullptr);
  if (timed) prof(c, PROF_STAGE, false, c.st);
  HIPCHK(hipGetLastError());
  s->staged = stage == 1;
  if (!s->tiled) return MSOM_OK;
  if ((r = migrate(c, s, stage == 1))) return r;
  // ... and the value of the recorded field by the new position's owner, behind the pass: the corners are points it holds
  if (rf) {
    c.interp(c.st, dev(s), s->n, rf, nullptr, c.g, c.fg, rec + 3 * (size_t)s->n, nullptr, &td);
    HIPCHK(hipGetLastError());
  }
  return MSOM_OK;
}

int hook(const Ctx &c, State *s, int stg, double dt, double tnext) {
  double *rec = nullptr;
  if (stg == 2 && s->rec && ++s->steps % s->every == 0) {
    if (s->nrec < s->cap) {
      rec = s->rec + (size_t)s->nrec++ * s->rows() * s->n;
      s->t.push_back(tnext);
    } else
      s->dropped++;
  }
  return stage(c, s, stg, dt, rec, true);
}

int stage_by_hand(const Ctx &c, State *s, int stg, double dt) {
  if ((stg != 1 && stg != 2) || !std::isfinite(dt)) { msom_set_error("%s_floats_stage: stage %d, dt = %g", c.model, stg, dt); return MSOM_ERR_ARG; }
  if (stg == 2 && !s->staged) { msom_set_error("%s_floats_stage: stage 2 without a stage 1 before it", c.model); return MSOM_ERR_STATE; }
  return stage(c, s, stg, dt, nullptr);
}

// readouts on tiles: send [3][n] by id with its presence words -> the values of every id, taken from the rank that holds it, in the
// two output arrays behind the slots; then to the caller's u0, u1 (host or device, either may be null)
static int combine(const Ctx &c, State *s, const double *send, double *u0, double *u1) {
  const size_t n = s->n;
  double *o0 = s->buf + 4 * n, *o1 = o0 + n;
  bracket(c, true);
  const int r = comm_allgather(c.comm, send, s->gr, 3 * n);
  if (!r) launch_floats_select(c.cst, s->gr, c.nranks, s->n, o0, o1);
  bracket(c, false);
  if (r) return r;
  HIPCHK(hipGetLastError());
  if (u0) HIPCHK(hipMemcpyAsync(u0, o0, n * sizeof(double), hipMemcpyDefault, c.st));
  if (u1) HIPCHK(hipMemcpyAsync(u1, o1, n * sizeof(double), hipMemcpyDefault, c.st));
  return MSOM_OK;
}

int begin_args(const Ctx &c, int n, const double *x, const double *y, const int *layer) {
  if (n < 1 || !x || !y || !layer) { msom_set_error("%s_floats_begin: n = %d, x, y or layer null", c.model, n); return MSOM_ERR_ARG; }
  return MSOM_OK;
}

int begin_check(const Ctx &c, int n, const double *&x, const double *&y, const int *&layer, HostArrays &h) {
  if (int r = begin_args(c, n, x, y, layer)) return r;
  if (is_device_ptr(x)) { h.hx.resize(n); HIPCHK(hipMemcpy(h.hx.data(), x, n * sizeof(double), hipMemcpyDeviceToHost)); x = h.hx.data(); }
  if (is_device_ptr(y)) { h.hy.resize(n); HIPCHK(hipMemcpy(h.hy.data(), y, n * sizeof(double), hipMemcpyDeviceToHost)); y = h.hy.data(); }
  if (is_device_ptr(layer)) { h.hl.resize(n); HIPCHK(hipMemcpy(h.hl.data(), layer, n * sizeof(int), hipMemcpyDeviceToHost)); layer = h.hl.data(); }
  const FloatsGeom &fg = c.fg;
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(x[k]) || !std::isfinite(y[k])) { msom_set_error("%s_floats_begin: float %d at (%g, %g)", c.model, k, x[k], y[k]); return MSOM_ERR_ARG; }
    if (!fg.periodic && !(x[k] >= 0 && x[k] <= fg.Lx && y[k] >= 0 && y[k] <= fg.Ly)) {
      msom_set_error("%s_floats_begin: float %d at (%g, %g) outside [0, %g] x [0, %g]", c.model, k, x[k], y[k], fg.Lx, fg.Ly);
      return MSOM_ERR_ARG;
    }
    if (layer[k] < 0 || layer[k] >= c.nl) { msom_set_error("%s_floats_begin: float %d in layer %d of %d", c.model, k, layer[k], c.nl); return MSOM_ERR_ARG; }
  }
  return MSOM_OK;
}

State *begin_alloc(const Ctx &c, int n) {
  State *s = new State;
  s->n = n;
  s->ncnt = c.ncnt;
  s->tiled = c.nranks > 1;
  const size_t nb = n * sizeof(double);
  bool ok = hipMalloc(&s->buf, 6 * nb) == hipSuccess && hipMalloc(&s->layer, n * sizeof(int)) == hipSuccess &&
            hipMalloc(&s->cnt, s->ncnt * sizeof(unsigned long long)) == hipSuccess;
  if (ok && s->tiled) {
    // a message carries the floats that cross one edge of the tile in one stage: with a CFL-limited step those within a fraction of
    // a cell of the edge, n / (points a side) or so of a uniform cloud; a sixteenth of all floats leaves room for a front, 1024 for small n
    s->K = c.msg_cap > 0 ? c.msg_cap : std::min(n, std::max(1024, n / 16));
    ok = hipMalloc(&s->id, n * sizeof(int)) == hipSuccess && hipMalloc(&s->live, n * sizeof(int)) == hipSuccess &&
         hipMalloc(&s->ctl, 4 * sizeof(int)) == hipSuccess && hipMalloc(&s->freest, n * sizeof(int)) == hipSuccess &&
         hipMalloc(&s->msg, 8 * s->msgcount() * sizeof(double)) == hipSuccess && hipMalloc(&s->gs, 3 * nb) == hipSuccess &&
         hipMalloc(&s->gr, (size_t)c.nranks * 3 * nb) == hipSuccess && hipMalloc(&s->dsum, s->ncnt * sizeof(double)) == hipSuccess;
  }
  if (ok) return s;
  (void)hipGetLastError();
  free_state(s);
  msom_set_error("%s_floats_begin: no device memory for %d floats", c.model, n);
  return nullptr;
}

int begin_fill(const Ctx &c, State *s, const double *x, const double *y, const int *layer, HostArrays &h) {
  const int n = s->n;
  HIPCHK(hipMemsetAsync(s->buf, 0, 6 * n * sizeof(double), c.st));
  HIPCHK(hipMemsetAsync(s->cnt, 0, s->ncnt * sizeof(unsigned long long), c.st));
  std::vector<int> tid;
  int nmine = n;
  if (s->tiled) {   // the floats this rank owns, in the first slots, located with the kernels' own functions
    const FloatsTiling &t = c.tl;
    for (int k = 0; k < n; k++) {
      int col, row;
      if (c.node) nfloats_owner(nfloats_locate(x[k], y[k], c.fg), t, &col, &row);
      else floats_owner(floats_locate(x[k], y[k], c.fg), t, &col, &row);
      if (col != t.ix || row != t.iy) continue;
      h.tx.push_back(x[k]); h.ty.push_back(y[k]); h.tl.push_back(layer[k]); tid.push_back(k);
    }
    nmine = (int)tid.size();
    x = h.tx.data(); y = h.ty.data(); layer = h.tl.data();
    const int ctl[4] = {nmine, 0, 0, 0};
    std::vector<int> live(n, 0);
    std::fill(live.begin(), live.begin() + nmine, 1);
    HIPCHK(hipMemsetAsync(s->layer, 0, n * sizeof(int), c.st));
    HIPCHK(hipMemsetAsync(s->id, 0, n * sizeof(int), c.st));
    HIPCHK(hipMemsetAsync(s->freest, 0, n * sizeof(int), c.st));
    HIPCHK(hipMemsetAsync(s->msg, 0, 8 * s->msgcount() * sizeof(double), c.st));
    HIPCHK(hipMemcpyAsync(s->ctl, ctl, sizeof ctl, hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(s->live, live.data(), n * sizeof(int), hipMemcpyHostToDevice, c.st));
    if (nmine) HIPCHK(hipMemcpyAsync(s->id, tid.data(), nmine * sizeof(int), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipStreamSynchronize(c.st));   // live and tid go out of scope
  }
  if (nmine) {
    HIPCHK(hipMemcpyAsync(s->buf, x, nmine * sizeof(double), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(s->buf + n, y, nmine * sizeof(double), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(s->layer, layer, nmine * sizeof(int), hipMemcpyHostToDevice, c.st));
  }
  return MSOM_OK;
}

int get(const Ctx &c, State *s, double *x, double *y) {
  if (!x || !y) { msom_set_error("%s_floats_get: null array", c.model); return MSOM_ERR_ARG; }
  const size_t n = s->n;
  if (s->tiled) {
    HIPCHK(hipMemsetAsync(s->gs, 0, 3 * n * sizeof(double), c.st));
    launch_floats_scatter(c.st, s->buf, s->buf + n, tile(c, s), s->n, s->gs);
    return combine(c, s, s->gs, x, y);
  }
  HIPCHK(hipMemcpyAsync(x, s->buf, n * sizeof(double), hipMemcpyDefault, c.st));
  HIPCHK(hipMemcpyAsync(y, s->buf + n, n * sizeof(double), hipMemcpyDefault, c.st));
  return MSOM_OK;
}

int interp(const Ctx &c, State *s, const char *call, const double *f, const double *pg, bool vel, double *u0, double *u1) {
  if (!u0 || (vel && !u1)) { msom_set_error("%s_%s: null array", c.model, call); return MSOM_ERR_ARG; }
  const size_t n = s->n;
  if (s->tiled) {   // each float on its owner, which between a stage 1 and its stage 2 is the owner of (xh, yh), not of (x, y)
    if (s->staged) { msom_set_error("%s_%s: on tiles not between a stage 1 and its stage 2", c.model, call); return MSOM_ERR_STATE; }
    const FloatsTileDev td = tile(c, s);
    HIPCHK(hipMemsetAsync(s->gs, 0, 3 * n * sizeof(double), c.st));
    c.interp(c.st, dev(s), s->n, f, pg, c.g, c.fg, s->gs, vel ? s->gs : nullptr, &td);
    HIPCHK(hipGetLastError());
    return combine(c, s, s->gs, u0, vel ? u1 : nullptr);
  }
  double *o0 = s->buf + 4 * n, *o1 = o0 + n;
  c.interp(c.st, dev(s), s->n, f, pg, c.g, c.fg, o0, vel ? o1 : nullptr, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(u0, o0, n * sizeof(double), hipMemcpyDefault, c.st));
  if (vel) HIPCHK(hipMemcpyAsync(u1, o1, n * sizeof(double), hipMemcpyDefault, c.st));
  return MSOM_OK;
}

int record(const Ctx &c, State *s, int every, int capacity, int field, const double *f, double tnow) {
  if (every < 1 || capacity < 1) { msom_set_error("%s_floats_record: every = %d, capacity = %d", c.model, every, capacity); return MSOM_ERR_ARG; }
  if (s->tiled && field >= 0 && s->staged) {   // record 0 samples the field at (x, y), on the owner of (x, y)
    msom_set_error("%s_floats_record: on tiles a field is not recorded from between a stage 1 and its stage 2", c.model);
    return MSOM_ERR_STATE;
  }
  HIPCHK(hipStreamSynchronize(c.st));   // a stage may still be writing a record
  double *rec = nullptr;
  const size_t n = s->n, rows = s->rows(field);
  HIPCHK(hipMalloc(&rec, (size_t)capacity * rows * n * sizeof(double)));
  if (s->rec) (void)hipFree(s->rec);
  s->rec = rec;
  s->every = every;
  s->cap = capacity;
  s->field = field < 0 ? -1 : field;
  s->nrec = 1;
  s->steps = s->dropped = 0;
  s->t.assign(1, tnow);
  // record 0: x then y, as they lie, and the sample of the field at them; on tiles by id, as the later ones are written
  if (s->tiled) {
    const FloatsTileDev td = tile(c, s);
    HIPCHK(hipMemsetAsync(rec, 0, rows * n * sizeof(double), c.st));
    launch_floats_scatter(c.st, s->buf, s->buf + n, td, s->n, rec);
    if (field >= 0) c.interp(c.st, dev(s), s->n, f, nullptr, c.g, c.fg, rec + 3 * n, nullptr, &td);
  } else {
    HIPCHK(hipMemcpyAsync(rec, s->buf, 2 * n * sizeof(double), hipMemcpyDeviceToDevice, c.st));
    if (field >= 0) c.interp(c.st, dev(s), s->n, f, nullptr, c.g, c.fg, rec + 2 * n, nullptr, nullptr);
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

int track(const Ctx &c, State *s, int first, int count, double *t, double *x, double *y, double *val) {
  if (!s->rec) { msom_set_error("%s_floats_track: no %s_floats_record since %s_floats_begin", c.model, c.model, c.model); return MSOM_ERR_STATE; }
  if (first < 0 || count < 1 || first > s->nrec - count) {
    msom_set_error("%s_floats_track: records %d .. %d of %d", c.model, first, first + count - 1, s->nrec);
    return MSOM_ERR_ARG;
  }
  if (val && s->field < 0) { msom_set_error("%s_floats_track: val given, but %s_floats_record chose no field", c.model, c.model); return MSOM_ERR_ARG; }
  for (int k = 0; t && k < count; k++) t[k] = s->t[first + k];
  const size_t n = s->n, nb = n * sizeof(double), rs = s->rows();
  const double *src = s->rec + (size_t)first * rs * n;
  if (s->tiled) {   // every record is combined over the ranks the way get combines the positions; so is its value.  Every rank makes
                    // the same gathers: the arrays a rank leaves out change nothing in them
    for (int k = 0; k < count; k++) {
      const double *rk = src + (size_t)k * rs * n;
      if (int r = combine(c, s, rk, x ? x + k * n : nullptr, y ? y + k * n : nullptr)) return r;
      if (s->field >= 0)
        if (int r = combine(c, s, rk + 3 * n, val ? val + k * n : nullptr, nullptr)) return r;
    }
    return MSOM_OK;
  }
  if (x) HIPCHK(hipMemcpy2DAsync(x, nb, src, rs * nb, nb, count, hipMemcpyDefault, c.st));
  if (y) HIPCHK(hipMemcpy2DAsync(y, nb, src + n, rs * nb, nb, count, hipMemcpyDefault, c.st));
  if (val) HIPCHK(hipMemcpy2DAsync(val, nb, src + 2 * n, rs * nb, nb, count, hipMemcpyDefault, c.st));
  return MSOM_OK;
}

bool param(const Ctx &c, const Opts &o, const char *k, double *v) {
  State *s = o.s;
  static const char *const counters[] = {"_clamped", "_lost", "_unsent", "_migrated", "_on_land"};
  int which = -1;
  for (int q = 0; q < c.ncnt; q++)
    if (!strcmp(k, counters[q])) which = q;
  if (!*k) *v = s ? s->n : 0;
  else if (!strcmp(k, "_records")) *v = s ? s->nrec : 0;
  else if (!strcmp(k, "_dropped")) *v = s ? (double)s->dropped : 0;
  else if (!strcmp(k, "_tiles")) *v = o.tiles;
  else if (!strcmp(k, "_msg_cap")) *v = s && s->tiled ? s->K : o.msg_cap;
  else if (!strcmp(k, "_resident")) {   // the rank's own: slots below the mark that are not on the free stack
    int h[2] = {s ? s->n : 0, 0};
    if (s && s->tiled && (hipStreamSynchronize(c.st) != hipSuccess || hipMemcpy(h, s->ctl, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)) { *v = NAN; return true; }
    *v = h[0] - h[1];
  } else if (which >= 0) {
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    *v = NAN;
    if (s) {
      if (which == CNT_LAND) {   // counted now, behind whatever the stream still holds
        const FloatsTileDev td = s->tiled ? tile(c, s) : FloatsTileDev{};
        if (hipMemsetAsync(s->cnt + CNT_LAND, 0, sizeof(unsigned long long), c.st) != hipSuccess) return true;
        c.on_land(c.st, dev(s), s->n, c.mask, c.g, c.fg, s->cnt + CNT_LAND, s->tiled ? &td : nullptr);
      }
      if (hipStreamSynchronize(c.st) != hipSuccess || hipMemcpy(cnt, s->cnt, s->ncnt * sizeof cnt[0], hipMemcpyDeviceToHost) != hipSuccess) return true;
    }
    double h[5];
    for (int q = 0; q < 5; q++) h[q] = (double)cnt[q];
    if (s && s->tiled) {   // collective: the sum over the ranks (whole numbers far below 2^53: exact in any order)
      if (hipMemcpy(s->dsum, h, s->ncnt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return true;
      bracket(c, true);
      const int r = comm_allreduce(c.comm, s->dsum, h, s->ncnt, RED_SUM);
      bracket(c, false);
      if (r) return true;
    }
    *v = h[which];
  } else
    return false;
  return true;
}

}  // namespace fh
