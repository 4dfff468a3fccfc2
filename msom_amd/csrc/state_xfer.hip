// state_xfer.hip -- the engine of the state files of both models (state_xfer.h; format: DESIGN "State file").  Field records move
// through kernels_state.hip; nothing here knows a handle, and nothing here runs inside a step.
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include "state_xfer.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e__ = (x);                                                                  \
    if (e__ != hipSuccess) {                                                               \
      msom_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e__), __FILE__, __LINE__, #x); \
      return MSOM_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)

namespace sx {

int Pipe::init(size_t doubles, int nranks) {
  cap = doubles;
  for (int b = 0; b < 2; b++) {
    HIPCHK(hipMalloc(&d[b], cap * sizeof(double)));
    HIPCHK(hipHostMalloc(&h[b], cap * sizeof(double)));
    HIPCHK(hipEventCreateWithFlags(&packed[b], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
  }
  HIPCHK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
  HIPCHK(hipMalloc(&dig, (size_t)(nranks + 1) * sizeof(unsigned long long)));
  HIPCHK(hipHostMalloc(&h_dig, (size_t)(nranks + 1) * sizeof(unsigned long long)));
  return MSOM_OK;
}

Pipe::~Pipe() {
  if (s2) { (void)hipStreamSynchronize(s2); (void)hipStreamDestroy(s2); }
  for (int b = 0; b < 2; b++) {
    if (d[b]) (void)hipFree(d[b]);
    if (h[b]) (void)hipHostFree(h[b]);
    if (packed[b]) (void)hipEventDestroy(packed[b]);
    if (copied[b]) (void)hipEventDestroy(copied[b]);
  }
  if (dig) (void)hipFree(dig);
  if (h_dig) (void)hipHostFree(h_dig);
}

size_t pipe_capacity(size_t W, size_t H) {
  const size_t cap = W * H;
  return cap > CHUNK_DOUBLES ? std::max(CHUNK_DOUBLES, W) : cap;
}

StateChunk chunk_of(const RecView &v, int layer, int y0, int rows, int sx0, int sw) {
  StateChunk c;
  c.g = v.g; c.ring = v.ring; c.layer = layer; c.y0 = y0; c.rows = rows; c.ox = v.ox; c.oy = v.oy;
  c.gW = v.W(); c.gH = v.H(); c.sx0 = sx0; c.sw = sw;
  return c;
}

int digest_word0(hipStream_t st, Pipe &pp, uint64_t *out) {
  HIPCHK(hipMemcpyAsync(pp.h_dig, pp.dig, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *out = pp.h_dig[0];
  return MSOM_OK;
}

namespace {

// whole record rows [ylo, yhi) of every layer, as many per chunk as the pipe holds (never less than one)
struct Rows { int layer, y0, rows; };
std::vector<Rows> chunk_plan(const Pipe &pp, int W, int layers, int ylo, int yhi) {
  int rows_max = (int)std::min<size_t>(pp.cap / W, (size_t)(yhi - ylo));
  if (rows_max < 1) rows_max = 1;
  std::vector<Rows> cs;
  for (int l = 0; l < layers; l++)
    for (int y = ylo; y < yhi; y += rows_max) cs.push_back({l, y, std::min(rows_max, yhi - y)});
  return cs;
}

}  // namespace

// ---- save

int save_record(hipStream_t st, Pipe &pp, const Field &f, FILE *fp, bool *io_ok) {
  const int W = f.v.W();
  const std::vector<Rows> cs = chunk_plan(pp, W, f.layers, 0, f.v.H());
  const int n = (int)cs.size();
  for (int c = 0; c <= n; c++) {
    if (c < n) {
      const int b = c & 1;
      launch_state_pack(st, f.dev, pp.d[b], chunk_of(f.v, cs[c].layer, cs[c].y0, cs[c].rows, 0, W), pp.dig);
      HIPCHK(hipEventRecord(pp.packed[b], st));
      HIPCHK(hipStreamWaitEvent(pp.s2, pp.packed[b], 0));
      HIPCHK(hipMemcpyAsync(pp.h[b], pp.d[b], (size_t)cs[c].rows * W * sizeof(double), hipMemcpyDeviceToHost, pp.s2));
      HIPCHK(hipEventRecord(pp.copied[b], pp.s2));
    }
    if (c >= 1) {
      const int b = (c - 1) & 1;
      HIPCHK(hipEventSynchronize(pp.copied[b]));   // the next pack into d[b] is launched after this: no event needed the other way
      const size_t cnt = (size_t)cs[c - 1].rows * W;
      if (*io_ok && fwrite(pp.h[b], sizeof(double), cnt, fp) != cnt) *io_ok = false;
    }
  }
  return MSOM_OK;
}

int write_file(const char *entry, const char *path, bool root, hipStream_t st, size_t cap, int nranks, msom_sfile &sf,
               const std::vector<Scal> &scal, const std::vector<Field> &fields, const SaveRecord &save, const DigestTotal &total) {
  Pipe pp;
  int r = pp.init(cap, nranks);
  if (r) return r;
  const std::string tmp = std::string(path) + ".tmp";
  FILE *fp = root ? fopen(tmp.c_str(), "wb") : nullptr;   // the other ranks of a tiled save hold no file and report no I/O failure
  struct Abandon {   // a return before the file is closed: a device error
    FILE *&fp; const std::string &tmp;
    ~Abandon() { if (fp) { fclose(fp); unlink(tmp.c_str()); } }
  } abandon{fp, tmp};
  bool io_ok = !root || fp != nullptr;
  sf.nrec = (uint32_t)(fields.size() + scal.size());
  if (fp && msom_swrite_header(fp, &sf)) io_ok = false;
  uint64_t dsum = 0;
  msom_srec rec;
  for (const Scal &s : scal) {
    memset(&rec, 0, sizeof rec);
    snprintf(rec.name, sizeof rec.name, "%s", s.name);
    rec.kind = MSOM_SK_SCALARS; rec.layers = (uint32_t)s.v.size(); rec.ny = rec.nx = 1;
    rec.nbytes = 8 * (uint64_t)s.v.size();
    rec.digest = msom_state_digest(s.v.data(), s.v.size(), 0);
    dsum += rec.digest;
    if (fp && io_ok && (msom_swrite_rechdr(fp, &rec) || fwrite(s.v.data(), sizeof(double), s.v.size(), fp) != s.v.size())) io_ok = false;
  }
  for (const Field &f : fields) {
    memset(&rec, 0, sizeof rec);
    snprintf(rec.name, sizeof rec.name, "%s", f.name);
    rec.kind = MSOM_SK_FIELD; rec.layers = (uint32_t)f.layers; rec.ny = (uint32_t)f.v.gny; rec.nx = (uint32_t)f.v.gnx; rec.ring = (uint32_t)f.v.ring;
    rec.nbytes = 8 * msom_srec_count(&rec);
    const long at = fp && io_ok ? ftell(fp) : -1;
    if (fp && io_ok && msom_swrite_rechdr(fp, &rec)) io_ok = false;   // digest 0 for now: it is known after the payload
    HIPCHK(hipMemsetAsync(pp.dig, 0, sizeof(unsigned long long), st));
    if ((r = save(pp, f, fp, &io_ok)) || (r = total(pp, &rec.digest))) return r;
    dsum += rec.digest;
    if (fp && io_ok && (fseek(fp, at, SEEK_SET) || msom_swrite_rechdr(fp, &rec) || fseek(fp, 0, SEEK_END))) io_ok = false;
  }
  if (fp && io_ok && msom_swrite_trailer(fp, dsum)) io_ok = false;
  if (fp && fclose(fp)) io_ok = false;
  fp = nullptr;
  if (root && io_ok && rename(tmp.c_str(), path)) io_ok = false;
  if (io_ok) return MSOM_OK;
  if (root) unlink(tmp.c_str());
  msom_set_error("%s: cannot write %s", entry, path);
  return MSOM_ERR_IO;
}

// ---- load

int read_scalars(const char *path, const msom_srec *r, std::vector<double> &v) {
  v.resize(r->layers);
  FILE *fp = fopen(path, "rb");
  const bool ok = fp && !fseek(fp, r->offset, SEEK_SET) && fread(v.data(), sizeof(double), v.size(), fp) == v.size();
  if (fp) fclose(fp);
  if (!ok) { msom_set_error("state file %s: short read in record %s", path, r->name); return MSOM_ERR_IO; }
  if (msom_state_digest(v.data(), v.size(), 0) != r->digest) { msom_set_error("state file %s: record %s: digest mismatch", path, r->name); return MSOM_ERR_IO; }
  return MSOM_OK;
}

int read_known_scalars(const char *entry, const char *path, const msom_srec *rec, const std::vector<KnownScalar> &known,
                       std::map<std::string, std::vector<double>> &sc) {
  bool ok = false;
  for (const KnownScalar &kn : known) ok |= !strcmp(kn.name, rec->name) && rec->layers == kn.n;
  if (!ok) { msom_set_error("%s: %s: scalar record %s with %u numbers is not one this library reads", entry, path, rec->name, rec->layers); return MSOM_ERR_CONFIG; }
  return read_scalars(path, rec, sc[rec->name]);
}

Temps::~Temps() {
  for (Loaded &l : v)
    if (l.nat) (void)hipFree(l.nat);
}
const Loaded *Temps::find(const char *name) const {
  for (const Loaded &l : v)
    if (!strcmp(l.rec->name, name)) return &l;
  return nullptr;
}

namespace {

// the record's rows of this tile into l.nat, then the digest of what the natural array holds
int load_record(hipStream_t st, Pipe &pp, FILE *fp, const char *path, const Loaded &l, long flip, const DigestTotal &total, uint64_t *digest) {
  const RecView &v = l.v;
  const int W = v.W(), H = v.H(), layers = (int)l.rec->layers;
  const std::vector<Rows> cs = chunk_plan(pp, W, layers, l.ylo, l.yhi);
  bool short_read = false;
  for (int c = 0; c < (int)cs.size(); c++) {
    const int b = c & 1;
    const size_t cnt = (size_t)cs[c].rows * W;
    if (c >= 2) HIPCHK(hipEventSynchronize(pp.packed[b]));   // the unpack of chunk c - 2 has read d[b]; its copy has left h[b] before that
    if (fseek(fp, l.rec->offset + (long)((((size_t)cs[c].layer * H + cs[c].y0) * W) * sizeof(double)), SEEK_SET) ||
        fread(pp.h[b], sizeof(double), cnt, fp) != cnt) {
      short_read = true;
      break;
    }
    HIPCHK(hipMemcpyAsync(pp.d[b], pp.h[b], cnt * sizeof(double), hipMemcpyHostToDevice, pp.s2));
    HIPCHK(hipEventRecord(pp.copied[b], pp.s2));
    HIPCHK(hipStreamWaitEvent(st, pp.copied[b], 0));
    launch_state_unpack(st, pp.d[b], l.nat, chunk_of(v, cs[c].layer, cs[c].y0, cs[c].rows, 0, W));
    HIPCHK(hipEventRecord(pp.packed[b], st));
  }
  RecView dv = v;   // what the digest covers
  if (l.own_nx) { dv.g.nx = l.own_nx; dv.g.ny = l.own_ny; }
  const int drows = l.own_nx ? l.own_ny : l.yhi - l.ylo;
  if (flip >= 0) {
    const size_t e = (size_t)flip % ((size_t)dv.g.nx * dv.g.ny);
    launch_state_flip(st, l.nat, nat_idx(v.g, 0, (int)(e / dv.g.nx), (int)(e % dv.g.nx)));
  }
  HIPCHK(hipMemsetAsync(pp.dig, short_read ? 0xA5 : 0, sizeof(unsigned long long), st));
  for (int k = 0; k < layers && !short_read; k++) launch_state_digest(st, l.nat, chunk_of(dv, k, l.ylo, drows, 0, W), pp.dig);
  const int r = total(pp, digest);
  if (short_read) {
    msom_set_error("state file %s: short read in record %s", path, l.rec->name);
    return MSOM_ERR_IO;
  }
  return r;
}

}  // namespace

int stage_records(const char *entry, const char *path, hipStream_t st, size_t cap, int nranks, Temps &tmp, long *state_flip,
                  const std::function<const double *(const Loaded &)> &current, const DigestTotal &total) {
  long flip = *state_flip;
  *state_flip = -1;
  Pipe pp;
  int r = pp.init(cap, nranks);
  if (r) return r;
  FILE *fp = fopen(path, "rb");
  if (!fp) { msom_set_error("state file %s not found", path); return MSOM_ERR_IO; }
  struct Close { FILE *f; ~Close() { fclose(f); } } close_fp{fp};
  for (Loaded &l : tmp.v) {
    HIPCHK(hipMalloc(&l.nat, l.bytes()));
    const double *cur = current(l);
    if (cur) HIPCHK(hipMemcpyAsync(l.nat, cur, l.bytes(), hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemsetAsync(l.nat, 0, l.bytes(), st));
    uint64_t d = 0;
    r = load_record(st, pp, fp, path, l, flip, total, &d);
    flip = -1;
    if (r) { (void)hipStreamSynchronize(pp.s2); (void)hipStreamSynchronize(st); return r; }
    if (d != l.rec->digest) {
      msom_set_error("%s: %s: record %s: the device holds digest %016llx, the file says %016llx", entry, path, l.rec->name,
                     (unsigned long long)d, (unsigned long long)l.rec->digest);
      return MSOM_ERR_IO;
    }
  }
  return MSOM_OK;
}

void destroy_keeping_error(const std::function<void()> &destroy) {
  const std::string keep = msom_last_error();
  destroy();
  msom_set_error("%s", keep.c_str());
}

}  // namespace sx
