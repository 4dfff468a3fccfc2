// prof_slot.h -- option profile of both models: HIP-event pairs around launches, read back as a total and a count per slot.
// Included by msom_host.h and msomn_host.h; which slots are on is the handle's business (the flag `on`).
#ifndef MSOM_PROF_SLOT_H
#define MSOM_PROF_SLOT_H

#include <hip/hip_runtime.h>

#include <vector>

struct ProfSlot {
  std::vector<hipEvent_t> ev;  // pairs (start, stop)
  size_t used = 0;
  double total_ms = 0;
  long launches = 0;
};
// begin and end bracket what is queued to st between them
static inline void prof_slot_begin(ProfSlot &ps, hipStream_t st, bool on) {
  if (!on) return;
  if (ps.used + 2 > ps.ev.size()) {
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    ps.ev.push_back(a); ps.ev.push_back(b);
  }
  hipEventRecord(ps.ev[ps.used], st);
}
static inline void prof_slot_end(ProfSlot &ps, hipStream_t st, bool on) {
  if (!on) return;
  hipEventRecord(ps.ev[ps.used + 1], st);
  ps.used += 2;
}
// waits for st (the handle's stream), then adds the recorded pairs to total_ms and launches
static inline void prof_slot_collect(ProfSlot &ps, hipStream_t st) {
  hipStreamSynchronize(st);
  for (size_t k = 0; k + 1 < ps.used; k += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ps.ev[k], ps.ev[k + 1]) == hipSuccess) { ps.total_ms += ms; ps.launches++; }
  }
  ps.used = 0;
}

#endif
