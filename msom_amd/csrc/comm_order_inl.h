// comm_order_inl.h -- how the messages of one halo exchange pair up between ranks.  Plain C++, no HIP, no
// allocation: tools/comm_order_host_check.cpp checks both functions against brute force under AddressSanitizer and UBSan.
//
// RCCL's rule inside one ncclGroupStart / ncclGroupEnd: the i-th ncclSend a rank posts to peer P pairs with the i-th ncclRecv P posts
// from that rank.  Nothing else is compared -- no tag travels -- and the two counts must be equal.  comm_post_order is the order in
// which comm_exchange posts a message list to the library so that the rule delivers every halo to the right edge; comm_pair applies
// the rule to the posted lists of all ranks, which is how the in-process transport pairs its messages.
#ifndef MSOM_COMM_ORDER_INL_H
#define MSOM_COMM_ORDER_INL_H

#include <stddef.h>

// directions of the 8 neighbours (buffer slots)
enum { DIR_W = 0, DIR_E = 1, DIR_S = 2, DIR_N = 3, DIR_SW = 4, DIR_SE = 5, DIR_NW = 6, DIR_NE = 7 };

// directions W E S N SW SE NW NE and their opposites
static const int COMM_OPP[8] = {1, 0, 3, 2, 7, 6, 5, 4};
struct Xfer {
  int peer;        // rank of the neighbour
  int tag;         // direction (DIR_*) of this tile's edge = direction the sent message travels in
  double *send, *recv;
  size_t count;    // doubles (same in both directions)
};

enum { COMM_MAX_XFER = 16 };  // messages of one exchange

// Posting order of the nx <= COMM_MAX_XFER messages of one exchange: send k is x[so[k]], receive k is x[ro[k]].
// Within a group the sends of one rank to a peer pair up with that peer's receives in posting order.  When both neighbours
// of an axis are the same rank (periodic tiling, 1 or 2 tiles per side) two messages go to one peer: sends are posted in
// the order of their direction, receives in the order of the direction the incoming message travels in (the opposite).
static inline void comm_post_order(const Xfer *x, int nx, int *so, int *ro) {
  for (int k = 0; k < nx; k++) so[k] = ro[k] = k;
  for (int a = 1; a < nx; a++)
    for (int b = a; b > 0; b--) {
      if (x[so[b]].tag < x[so[b - 1]].tag) { const int t = so[b]; so[b] = so[b - 1]; so[b - 1] = t; }
      if (COMM_OPP[x[ro[b]].tag & 7] < COMM_OPP[x[ro[b - 1]].tag & 7]) { const int t = ro[b]; ro[b] = ro[b - 1]; ro[b - 1] = t; }
    }
}
typedef void (*comm_order_fn)(const Xfer *x, int nx, int *so, int *ro);

enum {
  COMM_PAIR_OK = 0,
  COMM_PAIR_NUMBER = 1,  // the peer posts another number of sends to this rank than this rank posts receives from it: RCCL would hang
  COMM_PAIR_COUNT = 2,   // the paired send has another count: RCCL would hang or overrun
  COMM_PAIR_TAG = 3,     // the paired send does not travel in direction COMM_OPP[tag]: a halo delivered to the wrong edge
  COMM_PAIR_ARG = 4      // rank, entry or peer out of range, or a list longer than COMM_MAX_XFER
};

// The send that entry k of rank R receives when every rank posts its list (lists[r], counts[r] entries, r < nranks) in the order
// `order` gives: entry k has peer P and is the i-th of R's receives from P in R's receive order; the source is the i-th of P's
// sends to R in P's send order, entry *src_index of lists[*src_rank].  On COMM_PAIR_COUNT and COMM_PAIR_TAG the paired entry is
// still named; nrecv / nsend, where given, take the number of receives R posts from P and of sends P posts to R.
static inline int comm_pair_by(comm_order_fn order, const Xfer *const *lists, const int *counts, int nranks, int R, int k,
                               int *src_rank, int *src_index, int *nrecv = nullptr, int *nsend = nullptr) {
  *src_rank = *src_index = -1;
  if (nrecv) *nrecv = 0;
  if (nsend) *nsend = 0;
  if (R < 0 || R >= nranks || k < 0 || k >= counts[R] || counts[R] > COMM_MAX_XFER) return COMM_PAIR_ARG;
  const Xfer *x = lists[R];
  const int P = x[k].peer;
  if (P < 0 || P >= nranks || counts[P] < 0 || counts[P] > COMM_MAX_XFER) return COMM_PAIR_ARG;
  *src_rank = P;
  int so[COMM_MAX_XFER], ro[COMM_MAX_XFER];
  order(x, counts[R], so, ro);
  int i = -1, nr = 0;  // position of entry k among R's receives from P
  for (int q = 0; q < counts[R]; q++)
    if (x[ro[q]].peer == P) {
      if (ro[q] == k) i = nr;
      nr++;
    }
  const Xfer *px = lists[P];
  order(px, counts[P], so, ro);
  int src = -1, ns = 0;  // the i-th of P's sends to R
  for (int q = 0; q < counts[P]; q++)
    if (px[so[q]].peer == R) {
      if (ns == i) src = so[q];
      ns++;
    }
  if (nrecv) *nrecv = nr;
  if (nsend) *nsend = ns;
  if (nr != ns || i < 0 || src < 0) return COMM_PAIR_NUMBER;
  *src_index = src;
  if (px[src].count != x[k].count) return COMM_PAIR_COUNT;
  if (px[src].tag != COMM_OPP[x[k].tag & 7]) return COMM_PAIR_TAG;
  return COMM_PAIR_OK;
}
static inline int comm_pair(const Xfer *const *lists, const int *counts, int nranks, int R, int k, int *src_rank, int *src_index,
                            int *nrecv = nullptr, int *nsend = nullptr) {
  return comm_pair_by(comm_post_order, lists, counts, nranks, R, k, src_rank, src_index, nrecv, nsend);
}

#endif
