/*
 * msom_floats.h -- Lagrangian floats advected on the device with the model's own RK2 stages (msqg dialect; one tile, or tiles with the
 * option "floats_tiles", see "On tiles" below; exported by both libraries).  DESIGN.md section 8k has the arithmetic, the ghost and corner rule and the counted memory traffic.
 *
 * A float is a position (x, y) in domain coordinates, [0, Lx] x [0, Ly] with Lx = L0 and Ly = L0 * gny / gnx, and a layer in [0, nl).
 * Its velocity is that of the bilinear interpolation of psi (psi + psipg where the handle has a background stream function) between
 * the four cell centres around it: with idx = gnx / L0 and cell centres at (i + 1/2) / idx,
 *     xi = x * idx - 0.5;  i0 = floor(xi);  a = xi - i0       (eta, j0, b likewise from y)
 *     u = -((1 - a) * (P01 - P00) + a * (P11 - P10)) * idx
 *     v =  ((1 - b) * (P10 - P00) + b * (P11 - P01)) * idx    Pcd = F[layer][j0 + d][i0 + c]
 *   exactly non-divergent inside a dual cell.  Walls: i0 is clamped to [-1, nx - 1] and the ghost ring of psi is read (psi = 0 on the
 *   wall face), so the wall-normal velocity on a wall is exactly +-0 and a float on a wall slides along it.  sbc = -1: i0 wraps into
 *   [0, nx - 1] and column i0 + 1 = nx is the wrapped ghost column; positions are kept unwrapped.
 * One step of the model moves every float by its two stages, with the step's dt and the two stream functions the step inverts:
 *     stage 1: (xh, yh) = (x, y) + dt / 2 U(x, y; psi_n)        stage 2: (x, y) += dt U(xh, yh; psi_{n + 1/2})
 *   On walls both results are clamped to the box (counted in "floats_clamped", once per float and stage).  A position that is not
 *   finite makes the float lost: both coordinates become NaN and stay so, nothing is read for it, "floats_lost" counts it once.
 *
 * msom_floats_begin: n >= 1 floats after msom_set_const (else MSOM_ERR_STATE).  x, y [n] doubles, layer [n] ints, host or device
 *   pointers.  Walls: a value that is not finite, a position outside the box or a layer outside [0, nl): MSOM_ERR_ARG, nothing is
 *   allocated and earlier floats stay.  sbc = -1: any finite position.  A second begin replaces the first.  Sets option "floats" = 1:
 *   from here on msom_step queues the two stages behind its own (no host wait is added).
 * msom_floats_end: frees everything (as msom_destroy and msom_set_const do); without floats: MSOM_OK.
 * msom_floats_get: the current positions in the caller's order, x, y [n], host or device.  Waits for the stream.
 * msom_floats_velocity: (u, v) [n] at the current positions from the psi the handle holds now.
 * msom_floats_sample: out [n] = (1 - b) * ((1 - a) * P00 + a * P10) + b * ((1 - a) * P01 + a * P11) of any field of nl layers, in
 *   each float's layer (ghost ring as the field holds it).  A lost float gives NaN in both calls.
 * msom_floats_stage: the advection by hand, for callers that drive msom_update / msom_advance themselves: stage 1 or 2 above with the
 *   psi the handle holds at the call.  Stage 2 without a stage 1 since msom_floats_begin or the last stage 2: MSOM_ERR_STATE.
 * msom_floats_record: a trajectory buffer [capacity][2][n] on the device.  Record 0 is the positions at the call; after that one record
 *   is written behind every `every`-th msom_step (by the stage-2 kernel).  A full buffer stops recording: "floats_dropped" counts the
 *   records that found no room.  msom_floats_track: records first .. first + count - 1: t [count] (host memory; times are kept on the
 *   host), x, y [count][n] (host or device); any of the three may be NULL.
 * msom_floats_dbg_ghosted: out [nl][ny + 2][nx + 2] (host or device) = the field with its one-cell ghost ring, as the kernels read it.
 * msom_get_param: "floats" (n, 0: none), "floats_clamped", "floats_lost", "floats_records", "floats_dropped" (each waits for the
 *   stream); "floats_unsent", "floats_migrated" (0 on one rank), "floats_resident", "floats_tiles", "floats_msg_cap".  Option "floats": 0 pauses the stages of msom_step, 1 resumes them; accepted and without effect on a handle without floats.
 * Errors: null handle or array, n < 1, stage not 1 or 2, dt not finite, every < 1, capacity < 1, a range outside the records
 *   written: MSOM_ERR_ARG; any call but begin / end without floats: MSOM_ERR_STATE; a newqg handle or a handle of more than one rank:
 *   without the option "floats_tiles": MSOM_ERR_CONFIG.  Every call names itself in msom_last_error.  The floats are not part of the
 *   state file: msom_floats_get, then msom_floats_begin with the same arrays at a step boundary, continues with the same bits.
 *
 * On tiles.  Option "floats_tiles" (default 0), set with msom_set_option before msom_floats_begin, alike on all ranks.  0: a handle of
 *   more than one rank answers every call with MSOM_ERR_CONFIG.  1 on such a handle: the calls are accepted and COLLECTIVE -- every
 *   rank makes the same call in the same order, like msom_step; the option is the caller's statement of this, and a collective call
 *   made by one rank alone blocks the others.  On one rank the option has no effect; newqg handles stay refused.  For every float id
 *   the position on tiles equals the single tile's bit for bit (same build).
 *   begin: every rank passes the same n, x, y, layer -- global arrays, domain coordinates, checked against the global box -- and
 *   keeps the floats it owns; "floats" is n on every rank.  Ownership: with i0 of the arithmetic above on the global grid, the owner
 *   column is max(i0, 0) / tnx (tnx: cells of a tile), rows likewise: the owner changes on the cell-centre line half a cell beyond
 *   a seam, and the owner's corners i0 - ox, i0 + 1 - ox lie in [-1, tnx]: its own cells, the wall ghost or the exchanged ghost ring.
 *   A float is homed by the position its next stage evaluates: (x, y) after begin and after stage 2, (xh, yh) after stage 1; a lost
 *   float stays where it is.  At every moment each id is resident on exactly one rank ("floats_resident": the rank's own count).
 *   Migration: behind every stage kernel (msom_step and msom_floats_stage alike) one pass of two phases, W / E, then S / N over all
 *   residents, arrivals included, so a diagonal move needs no diagonal message.  Every rank posts every message every stage with
 *   the fixed count 1 + 6 K doubles (header: number of records; record: id, x, y, xh, yh, layer), K = option "floats_msg_cap" (set
 *   before begin; 0 = default min(n, max(1024, n / 16))).  A float that finds its message full, or whose owner is farther than one
 *   of the 8 neighbouring tiles, is made lost on the sender: NaN, resident there, counted in "floats_unsent" (not in "floats_lost").
 *   The single tile has no such loss.  "floats_migrated": records sent.
 *   get, velocity, sample, track: every rank receives the full arrays in the caller's order; bits as on the single tile, NaN of
 *   lost floats and -0.0 included.  velocity and sample are computed by each float's owner; between a stage 1 and its stage 2 by
 *   hand they return MSOM_ERR_STATE.  sample reads the tile's ghost ring: the neighbours' cells for the fields the model exchanges
 *   (psi, the tracers, ...), not for q, dq and the predictor, whose ring on a seam the model never fills.  A stage 1 by hand that
 *   follows a stage 1 homes the floats by (x, y) again first.  dbg_ghosted is local: the tile's [nl][ny + 2][nx + 2].
 *   "floats_clamped", "floats_lost", "floats_unsent", "floats_migrated" are sums over the ranks (collective).  Option "floats" must
 *   be set alike on all ranks.  In the product build the kernels form x * idx - 0.5 fused, the host in two roundings: begin ends
 *   with one migration pass, which takes a float within an ulp of a cell-centre line to the owner the kernels see (and counts it).
 */
#ifndef MSOM_FLOATS_H
#define MSOM_FLOATS_H

#include "msom.h"

#ifdef __cplusplus
extern "C" {
#endif

int msom_floats_begin(msom_t *m, int n, const double *x, const double *y, const int *layer);
int msom_floats_end(msom_t *m);
int msom_floats_get(msom_t *m, double *x, double *y);
int msom_floats_velocity(msom_t *m, double *u, double *v);
int msom_floats_sample(msom_t *m, int field, double *out);
int msom_floats_stage(msom_t *m, int stage, double dt);
int msom_floats_record(msom_t *m, int every, int capacity);
int msom_floats_track(msom_t *m, int first, int count, double *t, double *x, double *y);
int msom_floats_dbg_ghosted(msom_t *m, int field, double *out);

#ifdef __cplusplus
}
#endif
#endif
