// state_pipe.h -- staging of one save or load of a state file, shared by msom_state.hip and msomn_state.hip: two device chunks and
// two pinned host chunks, a second stream for the copies, events between the two streams, the device digest words.
// Needs HIPCHK of the including unit's host header.
#ifndef MSOM_STATE_PIPE_H
#define MSOM_STATE_PIPE_H

#include <hip/hip_runtime.h>

const size_t CHUNK_DOUBLES = (size_t)4 << 20;   // 32 MB per staging chunk

struct Pipe {
  double *d[2] = {nullptr, nullptr}, *h[2] = {nullptr, nullptr};
  hipStream_t s2 = nullptr;
  hipEvent_t packed[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
  unsigned long long *dig = nullptr, *h_dig = nullptr;   // device digest words (this rank's, then one per rank), pinned copy
  size_t cap = 0;
  int init(size_t doubles, int nranks) {
    cap = doubles;
    for (int b = 0; b < 2; b++) {
      HIPCHK(hipMalloc(&d[b], cap * sizeof(double)));
      HIPCHK(hipHostMalloc(&h[b], cap * sizeof(double)));
      HIPCHK(hipEventCreateWithFlags(&packed[b], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
    }
    HIPCHK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&dig, (size_t)(nranks + 1) * sizeof(unsigned long long)));
    HIPCHK(hipHostMalloc(&h_dig, (size_t)(nranks + 1) * sizeof(unsigned long long)));
    return MSOM_OK;
  }
  ~Pipe() {
    if (s2) { (void)hipStreamSynchronize(s2); (void)hipStreamDestroy(s2); }
    for (int b = 0; b < 2; b++) {
      if (d[b]) (void)hipFree(d[b]);
      if (h[b]) (void)hipHostFree(h[b]);
      if (packed[b]) (void)hipEventDestroy(packed[b]);
      if (copied[b]) (void)hipEventDestroy(copied[b]);
    }
    if (dig) (void)hipFree(dig);
    if (h_dig) (void)hipHostFree(h_dig);
  }
};

#endif
