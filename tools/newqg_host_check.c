/* newqg_host_check.c -- stand-alone driver of the newqg parser (msom_amd/csrc/params.c: msom_newqg_params_*), no GPU.
 *
 * Parses texts that stress the line rules -- over-long lines, a line of '=' only, arrays with more entries than the table holds,
 * empty values, no trailing newline, a file on disk -- and checks the derived values and the error codes.  Build together with
 * params.c with -fsanitize=address,undefined (tests/test_newqg_host.py does); exit status 0 = every case is as expected. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/msom.h"
#include "../msom_amd/csrc/msom_params.h"

static int fails = 0;
static void check(const char *name, int ok) {
  printf("%s: %s\n", name, ok ? "ok" : "FAIL");
  if (!ok) fails++;
}
static int parse(struct NewqgParams *p, const char *text) {
  msom_newqg_params_defaults(p);
  msom_newqg_params_parse_text(p, text);
  return msom_newqg_params_derive(p);
}

int main(int argc, char **argv) {
  struct NewqgParams p;
  check("sample", parse(&p, "N  = 128\nL0 = 100\nf0 = 46.5\nnu = 0.5\nsbc = 0. \ndh   = [1.0]\ngp_low = 2500.\nDT    = 5.e-2\nCFL   = 0.2\nTOLERANCE = 1e-5") == 0 &&
                      p.N == 128 && p.Ny == 128 && p.DT == 0.5 * fmin(5e-2, (100. / 128) * (100. / 128) / 0.5 / 4.) && p.bc_fac == 0. &&
                      p.iRd2_low == -(46.5 * 46.5) / (2500. * 1.0));
  check("defaults", parse(&p, "") == 0 && p.N == 64 && p.f0 == 1. && p.dh[0] == 1. && p.DT == 1e10 && p.iRd2_low == 0. && p.nitermax == 100);
  {   /* a line longer than the line buffer, then a key: the tail of the long line is parsed as a line of its own and matches nothing */
    char *t = (char *)malloc(2000);
    memset(t, 'x', 1500);
    strcpy(t + 1500, "\nN = 32\n=\n= 5\nL0 =\nsbc = 100\n");
    check("long line", parse(&p, t) == 0 && p.N == 32 && p.L0 == 1. && p.bc_fac == 100. / ((0.5 * 100. + 1) * ((1. / 32) * (1. / 32))));
    free(t);
  }
  {   /* more array entries than MSOM_MAXARR: the rest is dropped */
    char *t = (char *)malloc(4096), *s = t;
    s += sprintf(s, "dh = [");
    for (int k = 0; k < 100; k++) s += sprintf(s, "%d,", k + 1);
    sprintf(s, "]\n");
    /* the line is cut at the buffer's length as every line is; what is read are the first entries */
    check("long array", parse(&p, t) == 0 && p.dh[0] == 1. && p.dh[1] == 2. && p.bc_fac == 0.);
    free(t);
  }
  check("nl = 2", parse(&p, "nl = 2\n") == MSOM_ERR_CONFIG && strstr(msom_last_error(), "one layer"));
  check("N = 48", parse(&p, "N = 48\n") == MSOM_ERR_CONFIG);
  check("Ny = 24", parse(&p, "N = 32\nNy = 24\n") == MSOM_ERR_CONFIG);
  check("dh = 0", parse(&p, "dh = [0]\n") == MSOM_ERR_CONFIG);
  check("sbc", parse(&p, "sbc = -2\n") == MSOM_ERR_CONFIG && parse(&p, "sbc = -1\n") == 0 && parse(&p, "sbc = 0.5\n") == 0);
  {
    const char *path = argc > 1 ? argv[1] : "newqg_host_check.in";
    FILE *fp = fopen(path, "wt");
    int ok = fp != NULL;
    if (fp) {
      fputs("#!sh\nN = 16\nNy = 64\ngp_low = 4\nf0 = 2\ndh = [ 0.5 ]\nNITERMIN = 0", fp);
      fclose(fp);
      msom_newqg_params_defaults(&p);
      ok = msom_newqg_params_parse_file(&p, path) == 0 && msom_newqg_params_derive(&p) == 0 && p.N == 16 && p.Ny == 64 && p.nitermin == 0 &&
           p.iRd2_low == -(2. * 2.) / (4. * 0.5);
      remove(path);
      ok = ok && msom_newqg_params_parse_file(&p, path) == -2;
    }
    check("file", ok);
  }
  return fails ? 1 : 0;
}
