// floats_host.h -- the host side of the Lagrangian floats, once for the layered model (msom_floats.hip) and the
// vertex model (msomn_floats.hip, section 8l): the state, the views the kernels take, the migration pass, the stage, the record slots,
// the readouts, the "floats*" keys and options.  It knows streams and geometries, no handle: what is a handle's own comes in through a
// Ctx that the model fills per call.  No function here waits for the stream at its end: the closing wait is the model's.
#ifndef MSOM_FLOATS_HOST_H
#define MSOM_FLOATS_HOST_H

#include <vector>

#include "comm.h"
#include "kernels.h"
#include "msom_internal.h"

bool is_device_ptr(const void *p);

namespace fh {

enum { CNT_CLAMPED = 0, CNT_LOST = 1, CNT_UNSENT = 2, CNT_MIGRATED = 3, CNT_LAND = 4 /* vertex model: scratch word of "floats_on_land" */ };
enum { PROF_STAGE = 0, PROF_EMIGRATE = 1, PROF_IMMIGRATE = 2 };

struct State {
  int n = 0, ncnt = 4;
  double *buf = nullptr;               // x, y, xh, yh and two output arrays of the by-hand calls, n doubles each
  int *layer = nullptr;
  unsigned long long *cnt = nullptr;   // CNT_*, ncnt words
  int staged = 0;                      // a stage 1 since begin or the last stage 2
  // trajectory buffer [cap][rows()][n]; times on the host
  double *rec = nullptr;
  int every = 1, cap = 0, nrec = 0;
  int field = -1;                      // the field recorded along the trajectories (-1: positions only)
  long steps = 0, dropped = 0;         // stage-2 hooks seen since record; records that found the buffer full
  std::vector<double> t;
  // on tiles (option floats_tiles, more than one rank): the arrays above are n slots of which this rank fills those of the floats it
  // owns; records are indexed by id: x, y and a presence word, then (field) the value, a row not used and its presence word
  int tiled = 0, K = 0;                // K: records a message can carry (option floats_msg_cap)
  int *id = nullptr, *live = nullptr;
  int *ctl = nullptr;                  // high-water mark, free slots, records taken in the lo / hi message of the running phase
  int *freest = nullptr;               // free stack
  double *msg = nullptr;               // send W E S N, receive W E S N: msgcount() doubles each
  double *gs = nullptr, *gr = nullptr; // readouts: this rank's [3][n] by id, all ranks' [nranks][3][n]
  double *dsum = nullptr;              // the counters as doubles, for the sum over the ranks
  size_t msgcount() const { return 1 + 6 * (size_t)K; }
  size_t rows() const { return rows(field); }
  size_t rows(int fld) const { return tiled ? (fld < 0 ? 3 : 6) : (fld < 0 ? 2 : 3); }
};
void free_state(State *s);   // null: nothing

// what a handle keeps of its floats: the state (null until begin) and the options "floats", "floats_tiles", "floats_msg_cap"
struct Opts {
  State *s = nullptr;
  int on = 0;        // floats begun and option "floats" not 0: the model's step queues the two stages
  int tiles = 0;     // on more than one rank the floats calls are accepted and collective
  int msg_cap = 0;   // records per migration message (0: the default of begin)
};
// key: one of the three; anything else is "unknown option"
int set_option(Opts &o, const char *key, double v);

using StageFn = void (*)(hipStream_t, int stage, const FloatsDev &, int n, const double *psi, const double *pg, const NatGeom &,
                         const FloatsGeom &, double dt, double *rec, const double *rf, const FloatsTileDev *);
using InterpFn = void (*)(hipStream_t, const FloatsDev &, int n, const double *f, const double *pg, const NatGeom &, const FloatsGeom &,
                          double *o0, double *o1, const FloatsTileDev *);
using LandFn = void (*)(hipStream_t, const FloatsDev &, int n, const double *mk, const NatGeom &, const FloatsGeom &, unsigned long long *out,
                        const FloatsTileDev *);

struct Ctx {
  const char *model;         // "msom" or "msomn": the prefix of the calls' names in error texts
  hipStream_t st, cst;       // the handle's stream; the stream of the migration and gather launches
  Comm *comm;
  int nranks;
  const int *nb;             // [4] ranks behind W, E, S, N, -1: none
  int nl;
  FloatsGeom fg;             // the global geometry
  FloatsTiling tl;
  int ox, oy;                // the tile's origin (cells; vertex model: vertices)
  NatGeom g;
  const double *psi, *pg;    // pg: null without a background
  const double *rf;          // the field the state records, null when State::field < 0 or before begin
  int msg_cap, ncnt;         // option floats_msg_cap; counters of the model (4, vertex model 5)
  bool node;                 // the vertex grid's owner rule
  StageFn stage;
  InterpFn interp;
  LandFn on_land;            // null: "floats_on_land" is not a key of this model
  const double *mask;        // on_land's
  // the layered model's: the handle, comm_begin / comm_end around what goes to cst, prof_begin / prof_end of slot PROF_*.  Null: nothing
  void *h;
  void (*bracket)(void *h, bool open);
  void (*prof)(void *h, int slot, bool begin, hipStream_t st);
};

// The migration pass behind a stage kernel (tiles): two phases, W / E, then S / N over all residents, arrivals of the first phase
// included, so a diagonal move needs no diagonal message.  Every rank posts every message of the fixed count, with or without
// emigrants or neighbours: nothing is read on the host.  half: the floats are homed by (xh, yh), what stage 2 evaluates.  A failed
// exchange ends the pass, behind the closed bracket
int migrate(const Ctx &c, State *s, int half);
// one stage and, on tiles, what goes with it; rec: the record slot that is due (stage 2), or null
int stage(const Ctx &c, State *s, int stage, double dt, double *rec, bool timed = false);
// the model's step: the record slot of a due stage 2, then the stage, timed in PROF_STAGE
int hook(const Ctx &c, State *s, int stage, double dt, double tnext);
// msom(n)_floats_stage: its argument checks, then the stage
int stage_by_hand(const Ctx &c, State *s, int stage, double dt);

// begin, in three parts.  HostArrays: what the parts keep on the host until the model's closing wait -- the caller's device arrays and,
// on tiles, the floats of this rank.  The arguments: null or n < 1, then the arrays onto the host and every float finite, inside a
// domain that is not periodic, in a layer of nl
struct HostArrays {
  std::vector<double> hx, hy, tx, ty;
  std::vector<int> hl, tl;
};
int begin_args(const Ctx &c, int n, const double *x, const double *y, const int *layer);
int begin_check(const Ctx &c, int n, const double *&x, const double *&y, const int *&layer, HostArrays &h);
// a state for n floats (tiled: more than one rank), nothing uploaded; null with the error set (MSOM_ERR_HIP)
State *begin_alloc(const Ctx &c, int n);
// zeroes the state; on tiles the floats this rank owns go to its first slots
int begin_fill(const Ctx &c, State *s, const double *x, const double *y, const int *layer, HostArrays &h);

int get(const Ctx &c, State *s, double *x, double *y);
// velocity (vel) of f + pg to u0, u1, or the bilinear value of f to u0; call: "floats_velocity" or "floats_sample"
int interp(const Ctx &c, State *s, const char *call, const double *f, const double *pg, bool vel, double *u0, double *u1);
// f: the field to record (field >= 0), tnow: the time of record 0
int record(const Ctx &c, State *s, int every, int capacity, int field, const double *f, double tnow);
int track(const Ctx &c, State *s, int first, int count, double *t, double *x, double *y, double *val);
// key: what follows "floats" in a parameter's name; false: not a key of this model
bool param(const Ctx &c, const Opts &o, const char *key, double *v);

}  // namespace fh

#endif
