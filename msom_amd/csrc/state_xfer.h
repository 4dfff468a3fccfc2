// state_xfer.h -- what lies between the container of a state file (state_io.c) and a handle, once for the layered model (msom_state.hip)
// and the vertex model (msomn_state.hip): the staging buffers, the chunk plan, the save and the load of one field record through them,
// the file writer, and the load-side helpers.  It knows a stream and a view of a record, no handle: what is a handle's own comes in as
// arguments or callables.
#ifndef MSOM_STATE_XFER_H
#define MSOM_STATE_XFER_H

#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "state_io.h"

namespace sx {

const size_t CHUNK_DOUBLES = (size_t)4 << 20;   // 32 MB per staging chunk

// staging of one save or load: two device chunks and two pinned host chunks, a second stream for the copies, events between the two
// streams, the device digest words
struct Pipe {
  double *d[2] = {nullptr, nullptr}, *h[2] = {nullptr, nullptr};
  hipStream_t s2 = nullptr;
  hipEvent_t packed[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
  unsigned long long *dig = nullptr, *h_dig = nullptr;   // device digest words (this rank's, then one per rank), pinned copy
  size_t cap = 0;
  int init(size_t doubles, int nranks);
  ~Pipe();
};
// doubles per chunk for records of W x H: a layer, at most CHUNK_DOUBLES (and never less than a row)
size_t pipe_capacity(size_t W, size_t H);

// a field record as this rank sees it
struct RecView {
  NatGeom g;      // the tile's natural layout
  int ring;       // 1: the record carries the ghost ring (one tile only)
  int ox, oy;     // the tile's offset in the global grid (cells)
  int gnx, gny;   // the global grid (cells); a record row is W() wide, a layer has H() rows
  int W() const { return gnx + 2 * ring; }
  int H() const { return gny + 2 * ring; }
};
// rows y0 .. y0 + rows - 1 of a layer, staged from record column sx0 on in rows of sw
StateChunk chunk_of(const RecView &v, int layer, int y0, int rows, int sx0, int sw);

// this rank's digest word pp.dig[0] -> the record's digest; word0 is the answer of everything that is one tile
using DigestTotal = std::function<int(Pipe &, uint64_t *)>;
int digest_word0(hipStream_t st, Pipe &pp, uint64_t *out);

struct Field { const char *name; const double *dev; int layers; RecView v; };
struct Scal { const char *name; std::vector<double> v; };

// one tile: the record's rows go through the two chunk buffers -- while chunk c is packed and copied to the host on the second stream,
// chunk c - 1 is written -- and the digest ends in pp.dig[0].  A failed write clears *io_ok and the device work goes on
int save_record(hipStream_t st, Pipe &pp, const Field &f, FILE *fp, bool *io_ok);
using SaveRecord = std::function<int(Pipe &, const Field &, FILE *, bool *io_ok)>;

// The file: <path>.tmp (root rank only) with the header sf (nrec is set here), the scalar records, every field record through `save`
// with its digest from `total` patched into its header, the trailer; then the rename.  Any failure unlinks the temporary file; an I/O
// failure is reported as "<entry>: cannot write <path>" after the device work of every record is done.
int write_file(const char *entry, const char *path, bool root, hipStream_t st, size_t cap, int nranks, msom_sfile &sf,
               const std::vector<Scal> &scal, const std::vector<Field> &fields, const SaveRecord &save, const DigestTotal &total);

// ---- load

int read_scalars(const char *path, const msom_srec *r, std::vector<double> &v);
// a scalar record must be in the table with that many numbers; then it is read into sc[name]
struct KnownScalar { const char *name; uint32_t n; };
int read_known_scalars(const char *entry, const char *path, const msom_srec *rec, const std::vector<KnownScalar> &known,
                       std::map<std::string, std::vector<double>> &sc);

struct Loaded {   // a field record verified on the device, not yet in the handle
  int name = -1;                   // index into the model's table of record names
  const msom_srec *rec = nullptr;
  RecView v;
  int ylo = 0, yhi = 0;            // the record rows of this tile
  int own_nx = 0, own_ny = 0;      // tiles that hold shared vertices: the part of the tile, from its origin, that this rank's digest
                                   // word and the test flip cover (0: the whole tile)
  double *nat = nullptr;
  size_t bytes() const { return v.g.ls * rec->layers * sizeof(double); }
};
struct Temps {
  std::vector<Loaded> v;
  ~Temps();
  const Loaded *find(const char *name) const;
};

// Every record of tmp into a spare natural array (pads: those of current(l), or zero where the handle has no such array yet) and its
// digest recomputed there on the device: file -> pinned chunk -> device chunk (second stream) -> natural layout, two chunks in flight.
// *state_flip >= 0 alters that element (modulo the tile, or its own_nx x own_ny part) of layer 0 of the first record after its upload;
// it is -1 on return.  A short read on this rank does not keep it out of `total` (on tiles a collective): its word is spoilt first, so
// that every rank ends the record with MSOM_ERR_IO.
int stage_records(const char *entry, const char *path, hipStream_t st, size_t cap, int nranks, Temps &tmp, long *state_flip,
                  const std::function<const double *(const Loaded &)> &current, const DigestTotal &total);

// destroy() without losing the message of the error that led to it
void destroy_keeping_error(const std::function<void()> &destroy);

}  // namespace sx

#endif
