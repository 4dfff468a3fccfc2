/*
 * msom_state.h -- lossless checkpoint and bit-exact restart of a msom_t (both dialects: msqg and newqg; exported by both libraries).
 * The reference restarts from p0.bas / restart.nc: psi as float32, q recomputed, time loop and statistics from zero.  These calls
 * save the model state of a handle in fp64 with everything the next step reads, so that a run that is stopped, saved, destroyed,
 * re-created, loaded and continued gives the bits of the run that was never stopped.  File format: DESIGN.md, "State file".
 * The vertex model (msomn_t) has its own calls on the same container, dialect 2: msomn_state.h.
 *
 * What is saved: psi (the solver's first guess; with its ghost ring while they are stale after pystep_de), q, tracers, qof, the six
 *   MSOM_DE_* budgets, po_mft, the noise field, the AB3 history of the nudging loop by logical slot, the selected statistics
 *   accumulators with W and qo_me, the modal solver's warm start; t, dt, the dt limiter's previous, iter, tnext, the last mgstats
 *   (i, resb, resa, nrelax; not sum, whose last bit depends on the summation order of the path that made it: 0 after a load),
 *   seed / noise_draw / corrector_step, bfn_begun and the signs pystep_bfn left in iRe, iRe4, Eks, Ekb, stats_count / stats_every /
 *   option stats, nme_ft; newqg: psi, q and its time-loop scalars.  Nothing the handle caches (DESIGN "State a handle keeps across
 *   calls") is saved: a load drops all of it and the plain path rebuilds it.
 * msom_state_save: waits for the stream, writes `path`.tmp and renames it to `path`.  Changes nothing the next step reads.
 *   flags & MSOM_STATE_CONSTANTS: the constant inputs too (PSIPG, FR, RD, QFORC, TOPO, SIGMA, PTR_RELAX, BFN_OBS / BFN_GAIN where
 *   set, dh), so that the file alone restarts a run.  A stochastic handle with noise_mode = 0 draws from libc's process-wide rand(),
 *   whose state cannot be saved: MSOM_ERR_CONFIG (use noise_mode = 1).
 * Tiles: save and load are collective (every rank calls them, as msom_write_bas / msom_read_bas): each rank packs and digests its tile
 *   with global indices, rank 0 gathers and writes, the digests add up; every rank reads the shared file and takes its part.  A file
 *   does not know its tiling: one written on 2 x 2 loads on one tile, and the reverse.  A record that carries ghost values (psi after
 *   pystep_de, the modal warm start) is one tile's: MSOM_ERR_CONFIG on tiles.
 * msom_state_load: into a handle of the same grid, nl, nptr and dialect with the same stochastic, noise_mode, mode_pv_invert and
 *   flag_topo (else MSOM_ERR_CONFIG).  A handle without constants yet (no msom_set_const) takes the stored constants, if any, runs
 *   msom_set_const and then takes the evolving fields.  The whole file is validated on the host, then every field is uploaded into
 *   a spare array in the natural layout and its digest recomputed there on the device, before the handle changes: bad magic,
 *   unknown version, short file, digest mismatch: MSOM_ERR_IO, message in msom_last_error, handle as before the call.
 * msom_create_from_state: msom_create_str / msom_create_newqg_str of the params text in the file, then the options the file records
 *   (stochastic, noise_mode, seed, mode_pv_invert, flag_topo) and msom_state_load.  NULL on error.
 * msom_state_check, msom_state_info: host only, no handle, no GPU.  check walks the records and verifies every digest; info reports
 *   the header, t, dt, iter and the record names (comma-separated into names[names_len]; NULL: not wanted).
 * msom_state_dbg_flip: test aid.  The next msom_state_load on this handle flips the lowest mantissa bit of element `element` of the
 *   first field record on the device, between the upload and the device digest (element < 0: off).  That load must fail.
 * Options of msom_set_option that use these calls: "ckpt_steps" [0 = off]: msom_run writes <workdir>/state.msom (with constants) every
 *   that many steps; "resume" [0]: msom_run continues from <workdir>/state.msom if it exists.
 */
#ifndef MSOM_STATE_H
#define MSOM_STATE_H

#include <stddef.h>

#include "msom.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSOM_STATE_CONSTANTS 1u

typedef struct {
  int version, dialect;          /* dialect: 0 msqg, 1 newqg, 2 vertex model (msomn_state.h) */
  int nx, ny, nl, nptr;          /* global grid */
  int stochastic, noise_mode, mode_pv_invert, flag_topo;
  int nrecords;
  long iter;
  double t, dt;
} msom_state_info_t;

int msom_state_save(msom_t *m, const char *path, unsigned flags);
int msom_state_load(msom_t *m, const char *path);
msom_t *msom_create_from_state(const char *path);
int msom_state_check(const char *path, int *nrecords);
int msom_state_info(const char *path, msom_state_info_t *info, char *names, size_t names_len);
int msom_state_dbg_flip(msom_t *m, long element);

#ifdef __cplusplus
}
#endif
#endif
