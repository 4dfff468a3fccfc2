/* state_io.c -- the lossless state file of include/msom_state.h on the host: reader, writer, checker (format: DESIGN "State file").
 * Plain C, no HIP: msom_state_check / msom_state_info need no handle and no GPU.  Little-endian throughout; integers of the headers
 * are assembled byte by byte, payloads are the host's doubles (a big-endian host is refused at compile time). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/msom_state.h"
#include "msom_params.h"
#include "state_io.h"

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "the state file's payload is the host's fp64 in little-endian order"
#endif

#define ERR_IO (-2)   /* MSOM_ERR_IO of msom.h */
static const char MAGIC[8] = {'M', 'S', 'O', 'M', 'S', 'T', 'A', 'T'};
static const char ENDTAG[8] = {'M', 'S', 'O', 'M', 'E', 'N', 'D', 0};

static uint64_t mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ULL;
  z ^= z >> 27; z *= 0x94d049bb133111ebULL;
  z ^= z >> 31;
  return z;
}
uint64_t msom_state_digest(const double *x, size_t n, uint64_t k0) {
  uint64_t d = 0;
  for (size_t k = 0; k < n; k++) {
    uint64_t b;
    memcpy(&b, &x[k], 8);
    d += mix64(b + 0x9E3779B97F4A7C15ULL * (k0 + k + 1));
  }
  return d;
}
uint64_t msom_srec_count(const msom_srec *r) {
  const uint64_t g = r->ring ? 2 : 0;
  return (uint64_t)r->layers * (r->ny + g) * (r->nx + g);
}

static void put32(unsigned char *b, uint32_t v) { for (int k = 0; k < 4; k++) b[k] = (unsigned char)(v >> (8 * k)); }
static void put64(unsigned char *b, uint64_t v) { for (int k = 0; k < 8; k++) b[k] = (unsigned char)(v >> (8 * k)); }
static uint32_t get32(const unsigned char *b) { uint32_t v = 0; for (int k = 0; k < 4; k++) v |= (uint32_t)b[k] << (8 * k); return v; }
static uint64_t get64(const unsigned char *b) { uint64_t v = 0; for (int k = 0; k < 8; k++) v |= (uint64_t)b[k] << (8 * k); return v; }

/* ---- writer */
int msom_swrite_header(FILE *fp, const msom_sfile *sf) {
  unsigned char h[MSOM_STATE_HDR];
  memset(h, 0, sizeof h);
  memcpy(h, MAGIC, 8);
  const uint32_t v[12] = {sf->version, sf->dialect, sf->nx, sf->ny, sf->nl, sf->nptr, sf->stochastic, sf->noise_mode,
                          sf->mode_pv_invert, sf->flag_topo, sf->nrec, sf->params_len};
  for (int k = 0; k < 12; k++) put32(h + 8 + 4 * k, v[k]);
  if (fwrite(h, 1, sizeof h, fp) != sizeof h) return -1;
  if (sf->params_len && fwrite(sf->params, 1, sf->params_len, fp) != sf->params_len) return -1;
  const unsigned char zero[8] = {0};
  const size_t pad = (8 - sf->params_len % 8) % 8;
  if (pad && fwrite(zero, 1, pad, fp) != pad) return -1;
  return 0;
}
int msom_swrite_rechdr(FILE *fp, const msom_srec *r) {
  unsigned char h[MSOM_STATE_RECHDR];
  memset(h, 0, sizeof h);
  memcpy(h, r->name, strnlen(r->name, 16));
  put32(h + 16, r->kind); put32(h + 20, r->layers); put32(h + 24, r->ny); put32(h + 28, r->nx); put32(h + 32, r->ring);
  put64(h + 40, r->nbytes); put64(h + 48, r->digest);
  return fwrite(h, 1, sizeof h, fp) == sizeof h ? 0 : -1;
}
int msom_swrite_trailer(FILE *fp, uint64_t digest_sum) {
  unsigned char h[MSOM_STATE_TRAILER];
  memcpy(h, ENDTAG, 8);
  put64(h + 8, digest_sum);
  return fwrite(h, 1, sizeof h, fp) == sizeof h ? 0 : -1;
}

/* ---- reader */
void msom_sfile_free(msom_sfile *sf) {
  if (!sf) return;
  free(sf->params);
  free(sf->rec);
  sf->params = NULL;
  sf->rec = NULL;
}
const msom_srec *msom_sfile_find(const msom_sfile *sf, const char *name) {
  for (uint32_t k = 0; k < sf->nrec; k++)
    if (!strcmp(sf->rec[k].name, name)) return &sf->rec[k];
  return NULL;
}

static int fail(FILE *fp, msom_sfile *sf) {
  if (fp) fclose(fp);
  msom_sfile_free(sf);
  return ERR_IO;
}

int msom_sfile_open(const char *path, msom_sfile *sf, int verify) {
  memset(sf, 0, sizeof *sf);
  FILE *fp = fopen(path, "rb");
  if (!fp) { msom_set_error("state file %s not found", path); return ERR_IO; }
  if (fseek(fp, 0, SEEK_END)) { msom_set_error("state file %s: cannot seek", path); return fail(fp, sf); }
  const long fsize = ftell(fp);
  rewind(fp);
  unsigned char h[MSOM_STATE_HDR];
  if (fsize < MSOM_STATE_HDR || fread(h, 1, sizeof h, fp) != sizeof h) {
    msom_set_error("state file %s: short file (%ld bytes, the header has %d)", path, fsize, MSOM_STATE_HDR);
    return fail(fp, sf);
  }
  if (memcmp(h, MAGIC, 8)) { msom_set_error("state file %s: bad magic", path); return fail(fp, sf); }
  uint32_t *v[12] = {&sf->version, &sf->dialect, &sf->nx, &sf->ny, &sf->nl, &sf->nptr, &sf->stochastic, &sf->noise_mode,
                     &sf->mode_pv_invert, &sf->flag_topo, &sf->nrec, &sf->params_len};
  for (int k = 0; k < 12; k++) *v[k] = get32(h + 8 + 4 * k);
  if (sf->version != MSOM_STATE_VERSION) {
    msom_set_error("state file %s: unknown version %u (this library reads %u)", path, sf->version, MSOM_STATE_VERSION);
    sf->nrec = 0;
    return fail(fp, sf);
  }
  const uint32_t nrec = sf->nrec;
  sf->nrec = 0;
  long pos = MSOM_STATE_HDR;
  const uint64_t plen = (uint64_t)sf->params_len + (8 - sf->params_len % 8) % 8;
  if (nrec > MSOM_STATE_MAXREC || plen > (uint64_t)(fsize - pos)) {
    msom_set_error("state file %s: short file (header announces %u records and %u bytes of params, the file has %ld bytes)", path, nrec,
                   sf->params_len, fsize);
    return fail(fp, sf);
  }
  sf->params = (char *)malloc((size_t)sf->params_len + 1);
  sf->rec = (msom_srec *)calloc(nrec ? nrec : 1, sizeof(msom_srec));
  if (!sf->params || !sf->rec) { msom_set_error("state file %s: out of memory", path); return fail(fp, sf); }
  if (fread(sf->params, 1, sf->params_len, fp) != sf->params_len) { msom_set_error("state file %s: short read (params)", path); return fail(fp, sf); }
  sf->params[sf->params_len] = 0;
  pos += (long)plen;
  uint64_t dsum = 0;
  enum { CHUNK = 1 << 16 };
  double *buf = verify ? (double *)malloc(CHUNK * sizeof(double)) : NULL;
  if (verify && !buf) { msom_set_error("state file %s: out of memory", path); return fail(fp, sf); }
  for (uint32_t k = 0; k < nrec; k++) {
    msom_srec *r = &sf->rec[k];
    unsigned char rh[MSOM_STATE_RECHDR];
    if (fseek(fp, pos, SEEK_SET) || fsize - pos < MSOM_STATE_RECHDR || fread(rh, 1, sizeof rh, fp) != sizeof rh) {
      msom_set_error("state file %s: short file inside the header of record %u", path, k);
      free(buf);
      return fail(fp, sf);
    }
    memcpy(r->name, rh, 16);
    r->name[16] = 0;
    r->kind = get32(rh + 16); r->layers = get32(rh + 20); r->ny = get32(rh + 24); r->nx = get32(rh + 28); r->ring = get32(rh + 32);
    r->nbytes = get64(rh + 40); r->digest = get64(rh + 48);
    pos += MSOM_STATE_RECHDR;
    r->offset = pos;
    if (r->kind > MSOM_SK_SCALARS || r->ring > 1 || r->layers == 0 || r->ny == 0 || r->nx == 0 || r->ny > (1u << 20) || r->nx > (1u << 20) ||
        r->layers > (1u << 20) || r->nbytes != 8 * msom_srec_count(r)) {
      msom_set_error("state file %s: record %u (%s): shape %u x %u x %u, ring %u, kind %u does not match its %llu bytes", path, k, r->name,
                     r->layers, r->ny, r->nx, r->ring, r->kind, (unsigned long long)r->nbytes);
      free(buf);
      return fail(fp, sf);
    }
    if (r->nbytes > (uint64_t)(fsize - pos)) {
      msom_set_error("state file %s: short file: record %u (%s) announces %llu bytes, %ld are left", path, k, r->name,
                     (unsigned long long)r->nbytes, fsize - pos);
      free(buf);
      return fail(fp, sf);
    }
    if (verify) {
      uint64_t d = 0, done = 0;
      const uint64_t n = r->nbytes / 8;
      while (done < n) {
        const size_t c = n - done < CHUNK ? (size_t)(n - done) : (size_t)CHUNK;
        if (fread(buf, sizeof(double), c, fp) != c) {
          msom_set_error("state file %s: short read in record %u (%s)", path, k, r->name);
          free(buf);
          return fail(fp, sf);
        }
        d += msom_state_digest(buf, c, done);
        done += c;
      }
      if (d != r->digest) {
        msom_set_error("state file %s: record %u (%s): digest %016llx of the payload, %016llx in its header", path, k, r->name,
                       (unsigned long long)d, (unsigned long long)r->digest);
        free(buf);
        return fail(fp, sf);
      }
    }
    dsum += r->digest;
    pos += (long)r->nbytes;
    sf->nrec = k + 1;
  }
  free(buf);
  unsigned char t[MSOM_STATE_TRAILER];
  if (fseek(fp, pos, SEEK_SET) || fsize - pos < MSOM_STATE_TRAILER || fread(t, 1, sizeof t, fp) != sizeof t) {
    msom_set_error("state file %s: short file: no trailer", path);
    return fail(fp, sf);
  }
  if (memcmp(t, ENDTAG, 8) || get64(t + 8) != dsum) {
    msom_set_error("state file %s: trailer does not hold the sum of the record digests", path);
    return fail(fp, sf);
  }
  fclose(fp);
  return 0;
}

/* ---- host-only entry points of msom_state.h */
int msom_state_check(const char *path, int *nrecords) {
  if (!path) { msom_set_error("msom_state_check: null path"); return -1; }
  msom_sfile sf;
  const int r = msom_sfile_open(path, &sf, 1);
  if (r) return r;
  if (nrecords) *nrecords = (int)sf.nrec;
  msom_sfile_free(&sf);
  return 0;
}

int msom_state_info(const char *path, msom_state_info_t *info, char *names, size_t names_len) {
  if (!path || !info) { msom_set_error("msom_state_info: null argument"); return -1; }
  msom_sfile sf;
  const int r = msom_sfile_open(path, &sf, 0);
  if (r) return r;
  memset(info, 0, sizeof *info);
  info->version = (int)sf.version; info->dialect = (int)sf.dialect;
  info->nx = (int)sf.nx; info->ny = (int)sf.ny; info->nl = (int)sf.nl; info->nptr = (int)sf.nptr;
  info->stochastic = (int)sf.stochastic; info->noise_mode = (int)sf.noise_mode;
  info->mode_pv_invert = (int)sf.mode_pv_invert; info->flag_topo = (int)sf.flag_topo;
  info->nrecords = (int)sf.nrec;
  const msom_srec *tr = msom_sfile_find(&sf, "time");   /* t, dt, previous, tnext, iter */
  if (tr && tr->kind == MSOM_SK_SCALARS && tr->layers >= 5) {
    double v[5];
    FILE *fp = fopen(path, "rb");
    if (fp && !fseek(fp, tr->offset, SEEK_SET) && fread(v, sizeof(double), 5, fp) == 5) {
      info->t = v[0]; info->dt = v[1];
      info->iter = v[4] >= 0 && v[4] < 9e15 ? (long)v[4] : -1;
    }
    if (fp) fclose(fp);
  }
  if (names && names_len) {   /* comma-separated, cut at names_len - 1 */
    size_t at = 0;
    names[0] = 0;
    for (uint32_t k = 0; k < sf.nrec; k++) {
      const size_t l = strlen(sf.rec[k].name);
      if (at + l + 2 > names_len) break;
      if (k) names[at++] = ',';
      memcpy(names + at, sf.rec[k].name, l);
      at += l;
      names[at] = 0;
    }
  }
  msom_sfile_free(&sf);
  return 0;
}
