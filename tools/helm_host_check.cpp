// helm_host_check.cpp -- stand-alone driver of the modal solve's host bookkeeping (msom_amd/csrc/helm_inl.h), no GPU.
//
// A scripted residual history res[m][c] (max |res_m| after c cycles of mode m) plays the device.  The batched state machine is run on
// it as helm_solve runs it -- one "read" per cycle, every mode that still wants a cycle takes one -- and checked against nl separate
// mg_solve loops (mspg/elliptic.h:145-229) written out here one mode after the other: same i, nrelax, resb, resa, and a frozen mode
// is never swept again.  Build with -fsanitize=address,undefined (tests/test_helm_host.py does); exit status 0 = all cases agree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../msom_amd/csrc/helm_inl.h"

struct Case {
  const char *name;
  int nitermin, nitermax;
  double tol;
  std::vector<std::vector<double>> res;   // [mode][cycle], cycle 0 = warm start; the last entry repeats for later cycles
};

static double res_at(const std::vector<double> &r, int c) { return r[c < (int)r.size() ? c : (int)r.size() - 1]; }

// the reference loop for one mode
static msom_mgstats solve_one(const std::vector<double> &r, int nitermin, int nitermax, double tol) {
  msom_mgstats s = {};
  s.nrelax = 4;
  double resb = s.resb = s.resa = res_at(r, 0);
  for (s.i = 0; s.i < nitermax && (s.i < nitermin || s.resa > tol); s.i++) {
    s.resa = res_at(r, s.i + 1);
    if (s.resa > tol) {
      if (resb / s.resa < 1.2 && s.nrelax < 100) s.nrelax++;
      else if (resb / s.resa > 10 && s.nrelax > 2) s.nrelax--;
    }
    resb = s.resa;
  }
  return s;
}

static int run(const Case &c) {
  const int nl = (int)c.res.size();
  HelmSolve h;
  helm_begin(h, nl, c.nitermin, c.nitermax, c.tol);
  std::vector<double> res0(nl), sum(nl, 0.), resa(nl);
  std::vector<int> done(nl, 0), swept_after_freeze(nl, 0), frozen(nl, 0);
  for (int m = 0; m < nl; m++) res0[m] = res_at(c.res[m], 0);
  if (c.nitermin < 1) helm_first(h, res0.data(), sum.data());
  int count[MSOM_MAXNL], guard = 0, fails = 0;
  while (helm_counts(h, count) > 0) {
    if (++guard > 1000) { printf("%s: the batch does not end\n", c.name); return 1; }
    for (int m = 0; m < nl; m++) {
      if (count[m] > 0) {
        if (frozen[m]) swept_after_freeze[m] = 1;
        if (count[m] != h.s[m].nrelax) { printf("%s: mode %d sweeps %d != nrelax %d\n", c.name, m, count[m], h.s[m].nrelax); fails++; }
        done[m]++;
      } else frozen[m] = 1;
      resa[m] = res_at(c.res[m], done[m]);   // a frozen mode's residual is recomputed and must be ignored
    }
    helm_first(h, res0.data(), sum.data());
    helm_cycle_done(h, count, resa.data());
  }
  helm_first(h, res0.data(), sum.data());
  for (int m = 0; m < nl; m++) {
    const msom_mgstats want = solve_one(c.res[m], c.nitermin, c.nitermax, c.tol), &got = h.s[m];
    if (got.i != want.i || got.nrelax != want.nrelax || got.resb != want.resb || got.resa != want.resa || swept_after_freeze[m]) {
      printf("%s: mode %d: i %d / %d, nrelax %d / %d, resb %g / %g, resa %g / %g, swept after freeze %d\n", c.name, m, got.i, want.i, got.nrelax,
             want.nrelax, got.resb, want.resb, got.resa, want.resa, swept_after_freeze[m]);
      fails++;
    }
  }
  printf("%s: %s\n", c.name, fails ? "FAIL" : "ok");
  return fails;
}

int main() {
  std::vector<Case> cases = {
      {"three modes freeze at different cycles", 1, 100, 1e-3, {{1., 0.19, 0.011, 1.3e-3, 1.5e-4}, {1., 1.4e-5}, {1., 2.6e-7}}},
      {"slow mode raises nrelax to the cap of the rule", 1, 100, 1e-3, {{1., 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 1e-4}, {1., 1e-9}}},
      {"fast mode lowers nrelax to 2 and stays", 1, 100, 1e-12, {{1., 1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 1e-13}}},
      {"NITERMAX ends a mode that never converges", 1, 5, 1e-3, {{1., 0.99, 0.98, 0.97}, {1., 1e-6}}},
      {"NITERMIN 0 with a converged warm start: no cycle", 0, 100, 1e-3, {{1e-5, 1e-9}, {1e-6, 1e-9}}},
      {"NITERMIN 0, one mode converged and one not", 0, 100, 1e-3, {{1e-5, 1e-9}, {1., 1e-2, 1e-6}}},
      {"NITERMIN 3 keeps a converged mode running", 3, 100, 1e-3, {{1., 1e-6, 1e-7, 1e-8, 1e-9}, {1., 0.5, 0.2, 0.1, 1e-5}}},
      {"NITERMAX 0: nothing runs", 1, 0, 1e-3, {{1., 0.1}, {2., 0.1}}},
      {"sixteen modes", 1, 100, 1e-3, {}},
  };
  for (int m = 0; m < MSOM_MAXNL; m++) {   // mode m needs m + 1 cycles
    std::vector<double> r(1, 1.);
    for (int c = 0; c < m; c++) r.push_back(0.3 / (c + 1));
    r.push_back(1e-6);
    cases.back().res.push_back(r);
  }
  int fails = 0;
  for (const Case &c : cases) fails += run(c);
  return fails ? 1 : 0;
}
