/* state_check -- walks a state file (include/msom_state.h) on the host and verifies every digest: no GPU, no library.
 * usage: msom_state_check FILE...   exit status 0: every file is good, 1: one was refused (message on stdout), 2: usage.
 * Stands alone on state_io.c and params.c, so that a sanitizer build of the reader is one compiler line:
 *   cc -fsanitize=address,undefined -o state_check driver/state_check.c state_io.c params.c -lm */
#include <stdio.h>

#include "../../../include/msom_state.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s FILE...\n", argv[0]);
    return 2;
  }
  int bad = 0;
  for (int k = 1; k < argc; k++) {
    int nrec = 0;
    char names[1024];
    msom_state_info_t info;
    int r = msom_state_check(argv[k], &nrec);
    if (!r) r = msom_state_info(argv[k], &info, names, sizeof names);
    if (r) {
      printf("%s: refused (%d): %s\n", argv[k], r, msom_last_error());
      bad = 1;
      continue;
    }
    static const char *const dialects[] = {"msqg", "newqg", "vertex"};
    printf("%s: ok, version %d, dialect %d (%s), %d x %d x %d, t = %.17g, iter = %ld, %d records: %s\n", argv[k], info.version, info.dialect,
           info.dialect >= 0 && info.dialect < 3 ? dialects[info.dialect] : "unknown", info.nx, info.ny, info.nl, info.t, info.iter, nrec, names);
  }
  return bad;
}
