/* state_io.h -- host side of the lossless state file (include/msom_state.h, DESIGN "State file"): reader, writer, checker.
 * Plain C, no HIP.  Shared by state_io.c and msom_state.hip. */
#ifndef MSOM_STATE_IO_H
#define MSOM_STATE_IO_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSOM_STATE_VERSION 1u
#define MSOM_STATE_HDR 64      /* bytes of the file header before the params text */
#define MSOM_STATE_RECHDR 64   /* bytes of a record header */
#define MSOM_STATE_TRAILER 16
#define MSOM_STATE_MAXREC 4096 /* a file that claims more records is refused */

enum { MSOM_SK_FIELD = 0 /* [layers][ny][nx] of the global grid */, MSOM_SK_SCALARS = 1 /* `layers` numbers, ny = nx = 1 */ };

typedef struct {
  char name[17];                          /* 16 bytes in the file, NUL padded */
  uint32_t kind, layers, ny, nx, ring;    /* ring: the payload carries the ghost ring, [layers][ny + 2][nx + 2] */
  uint64_t nbytes, digest;
  long offset;                            /* of the payload in the file */
} msom_srec;

typedef struct {
  uint32_t version, dialect, nx, ny, nl, nptr, stochastic, noise_mode, mode_pv_invert, flag_topo, nrec, params_len;
  char *params;                           /* params_len bytes + NUL */
  msom_srec *rec;
} msom_sfile;

/* splitmix64 finaliser and the digest of n doubles whose first element has index k0 in its record */
uint64_t msom_state_digest(const double *x, size_t n, uint64_t k0);
/* doubles of a record's payload by its shape */
uint64_t msom_srec_count(const msom_srec *r);

/* Walks the whole file: header, every record header against the file size, trailer; verify != 0: every payload digest too.
 * 0, or MSOM_ERR_IO with a message in msom_last_error.  On success *sf owns params and rec (msom_sfile_free). */
int msom_sfile_open(const char *path, msom_sfile *sf, int verify);
void msom_sfile_free(msom_sfile *sf);
const msom_srec *msom_sfile_find(const msom_sfile *sf, const char *name);

/* writer: header (sf->nrec announced), then per record its header and payload, then the trailer.  0 or -1 */
int msom_swrite_header(FILE *fp, const msom_sfile *sf);
int msom_swrite_rechdr(FILE *fp, const msom_srec *r);
int msom_swrite_trailer(FILE *fp, uint64_t digest_sum);

#ifdef __cplusplus
}
#endif
#endif
