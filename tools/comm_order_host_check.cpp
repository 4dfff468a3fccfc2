// comm_order_host_check.cpp -- stand-alone check of the order in which a halo exchange posts its messages and of the rule that pairs
// them (msom_amd/csrc/comm_order_inl.h), no GPU.
//
// For every px, py in {1, 2, 3, 4, 8}, walled and doubly periodic, every rank builds the message lists the callers of comm_exchange
// post -- {W, E}, {S, N}, {W, E, S, N} -- and the list of all eight directions, which no caller posts today but Xfer, the buffers
// and nb[8] provide for.  Neighbour ranks follow create_common (msom_api.hip), an entry is left out behind a wall; counts are 5 for
// W / E, 7 for S / N and 1 for a corner, so that a mix-up of edges of different length shows as a count error.  Tags are unique
// within a list, so the true source of rank R's entry with tag d is the entry with tag COMM_OPP[d] in the list of rank nb_R[d],
// found here by search: comm_pair must name exactly that entry, for every rank and entry.  One further list stands outside the
// enumerated set: one rank that is its own peer on all four faces, which is what msom_dbg_rccl_selftest posts.
//
// That the check can fail is shown with two wrong posting orders, which exist only in this file: receives posted in the order of the
// sends, and receives posted by descending tag.  Two broken sets of lists -- one message dropped, one count changed -- must be
// refused with the error that names the defect.  Build with -fsanitize=address,undefined (tests/test_comm_order_host.py does); exit
// status 0 = everything as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../msom_amd/csrc/comm_order_inl.h"

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (fails < 40) { printf("FAIL " __VA_ARGS__); printf("  [%s]\n", #cond); } \
      fails++;                                             \
    }                                                      \
  } while (0)

// ---- the two wrong rules
// receives in the order of the sends (by tag)
static void order_recv_as_sends(const Xfer *x, int nx, int *so, int *ro) {
  comm_post_order(x, nx, so, ro);
  for (int k = 0; k < nx; k++) ro[k] = so[k];
}
// receives by descending tag: right for two faces of one axis, wrong as soon as a peer gets faces of both axes or corners
static void order_recv_descending(const Xfer *x, int nx, int *so, int *ro) {
  comm_post_order(x, nx, so, ro);
  for (int k = 0; k < nx; k++) ro[k] = k;
  for (int a = 1; a < nx; a++)
    for (int b = a; b > 0 && x[ro[b]].tag > x[ro[b - 1]].tag; b--) { const int t = ro[b]; ro[b] = ro[b - 1]; ro[b - 1] = t; }
}

// ---- topologies and lists
struct Topo {
  int px, py;
  bool periodic;
};
// neighbour ranks of create_common: wrapped on a periodic tiling of more than one tile, -1 behind a wall
static void neighbours(const Topo &t, int rank, int nb[8]) {
  const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
  const int ix = rank % t.px, iy = rank / t.px;
  for (int d = 0; d < 8; d++) {
    nb[d] = -1;
    const int jx = ix + dx[d], jy = iy + dy[d];
    if (t.periodic && t.px * t.py > 1) nb[d] = ((jy + t.py) % t.py) * t.px + (jx + t.px) % t.px;
    else if (jx >= 0 && jx < t.px && jy >= 0 && jy < t.py) nb[d] = jy * t.px + jx;
  }
}
static size_t dir_count(int d) { return d == DIR_W || d == DIR_E ? 5 : d == DIR_S || d == DIR_N ? 7 : 1; }

struct DirSet {
  const char *name;
  int n, dirs[8];
};
static const DirSet SETS[4] = {{"WE", 2, {DIR_W, DIR_E}},
                               {"SN", 2, {DIR_S, DIR_N}},
                               {"WESN", 4, {DIR_W, DIR_E, DIR_S, DIR_N}},
                               {"all8", 8, {DIR_W, DIR_E, DIR_S, DIR_N, DIR_SW, DIR_SE, DIR_NW, DIR_NE}}};

struct Lists {
  std::vector<std::vector<Xfer>> x;   // per rank, in the caller's order
  std::vector<std::vector<int>> nb;   // per rank: nb[8]
  std::vector<const Xfer *> ptr;
  std::vector<int> cnt;
  void refresh() {
    ptr.clear(); cnt.clear();
    for (auto &v : x) { ptr.push_back(v.data()); cnt.push_back((int)v.size()); }
  }
};
static double g_slots[16];  // send / recv only have to be distinct addresses; nothing is read or written through them
static Lists build_lists(const Topo &t, const DirSet &s) {
  Lists L;
  const int P = t.px * t.py;
  L.x.resize(P); L.nb.resize(P);
  for (int r = 0; r < P; r++) {
    int nb[8];
    neighbours(t, r, nb);
    L.nb[r].assign(nb, nb + 8);
    for (int q = 0; q < s.n; q++) {
      const int d = s.dirs[q];
      if (nb[d] < 0) continue;
      L.x[r].push_back(Xfer{nb[d], d, &g_slots[d], &g_slots[8 + d], dir_count(d)});
    }
  }
  L.refresh();
  return L;
}
// one rank, its own peer on the four faces: the list of msom_dbg_rccl_selftest
static Lists build_self_lists(const DirSet &s) {
  Lists L;
  L.x.resize(1); L.nb.resize(1);
  L.nb[0].assign(8, 0);
  for (int q = 0; q < s.n; q++) L.x[0].push_back(Xfer{0, s.dirs[q], &g_slots[s.dirs[q]], &g_slots[8 + s.dirs[q]], dir_count(s.dirs[q])});
  L.refresh();
  return L;
}

// pairs every entry of every rank under `order`; counts the entries whose pairing is not the true one, by error code (index 0:
// no error reported, but another entry than the true one named)
struct Tally {
  int entries = 0, wrong = 0, by_code[5] = {0, 0, 0, 0, 0};
};
static Tally pair_all(const Lists &L, comm_order_fn order) {
  Tally T;
  const int P = (int)L.x.size();
  for (int r = 0; r < P; r++)
    for (int k = 0; k < (int)L.x[r].size(); k++) {
      const Xfer &e = L.x[r][k];
      // brute force: the entry with the opposite tag in the list of the neighbour in direction e.tag
      const int want_rank = L.nb[r][e.tag];
      int want_index = -1, matches = 0;
      if (want_rank >= 0)
        for (int q = 0; q < (int)L.x[want_rank].size(); q++)
          if (L.x[want_rank][q].tag == COMM_OPP[e.tag]) { want_index = q; matches++; }
      int sr = -2, si = -2;
      const int code = comm_pair_by(order, L.ptr.data(), L.cnt.data(), P, r, k, &sr, &si);
      T.entries++;
      const bool right = code == COMM_PAIR_OK && matches == 1 && sr == want_rank && si == want_index && L.x[sr][si].peer == r &&
                         L.x[sr][si].count == e.count;
      if (!right) { T.wrong++; T.by_code[code >= 0 && code <= 4 ? code : 4]++; }
    }
  return T;
}

static void topo_name(const Topo &t, char *buf, size_t n) { snprintf(buf, n, "%s %dx%d", t.periodic ? "periodic" : "walled", t.px, t.py); }

// the posting order of the loops that stood in comm_exchange before comm_post_order, kept here to show that the move changed nothing
static void order_before_the_move(const Xfer *x, int nx, int *so, int *ro) {
  for (int k = 0; k < nx; k++) so[k] = ro[k] = k;
  for (int a = 1; a < nx; a++)
    for (int b = a; b > 0; b--) {
      if (x[so[b]].tag < x[so[b - 1]].tag) std::swap(so[b], so[b - 1]);
      if (COMM_OPP[x[ro[b]].tag & 7] < COMM_OPP[x[ro[b - 1]].tag & 7]) std::swap(ro[b], ro[b - 1]);
    }
}

int main() {
  const int parts[] = {1, 2, 3, 4, 8};
  std::vector<Topo> topos;
  for (int per = 0; per < 2; per++)
    for (int px : parts)
      for (int py : parts) topos.push_back(Topo{px, py, per == 1});

  // ---- the project's rule on every topology and list; the wrong rules beside it
  int ntopo = 0, nlists = 0, nentries = 0;
  std::vector<std::string> caught_same, caught_desc;
  int desc_face_wrong = 0;
  for (const Topo &t : topos) {
    char name[64];
    topo_name(t, name, sizeof name);
    const int before = fails;
    int entries = 0;
    for (const DirSet &s : SETS) {
      const Lists L = build_lists(t, s);
      // every tag at most once in a list; walled ranks leave entries out, periodic ranks of a tiling never do
      for (int r = 0; r < t.px * t.py; r++) {
        int seen = 0;
        for (const Xfer &e : L.x[r]) { CHECK(!(seen & (1 << e.tag)), "%s %s rank %d: tag %d twice\n", name, s.name, r, e.tag); seen |= 1 << e.tag; }
        if (t.periodic && t.px * t.py > 1) CHECK((int)L.x[r].size() == s.n, "%s %s rank %d: %zu entries\n", name, s.name, r, L.x[r].size());
        // the new function gives the order of the loops it replaced
        int so[COMM_MAX_XFER], ro[COMM_MAX_XFER], so0[COMM_MAX_XFER], ro0[COMM_MAX_XFER];
        comm_post_order(L.ptr[r], L.cnt[r], so, ro);
        order_before_the_move(L.ptr[r], L.cnt[r], so0, ro0);
        CHECK(!memcmp(so, so0, L.cnt[r] * sizeof(int)) && !memcmp(ro, ro0, L.cnt[r] * sizeof(int)), "%s %s rank %d: posting order moved\n", name, s.name, r);
      }
      const Tally T = pair_all(L, comm_post_order);
      CHECK(T.wrong == 0, "%s %s: %d of %d entries paired wrongly (no error %d, number %d, count %d, tag %d, arg %d)\n", name, s.name, T.wrong,
            T.entries, T.by_code[0], T.by_code[1], T.by_code[2], T.by_code[3], T.by_code[4]);
      entries += T.entries;
      nlists++;
      const bool faces = s.n <= 4;
      const Tally A = pair_all(L, order_recv_as_sends);
      if (A.wrong) {
        char b[96];
        snprintf(b, sizeof b, "%s %s (%s)", name, s.name, A.by_code[3] == A.wrong ? "tag" : "mixed");
        caught_same.push_back(b);
      }
      const Tally D = pair_all(L, order_recv_descending);
      if (D.wrong) {
        char b[96];
        snprintf(b, sizeof b, "%s %s", name, s.name);
        caught_desc.push_back(b);
        if (faces) desc_face_wrong++;
      }
    }
    ntopo++;
    nentries += entries;
    printf("%s: %d messages: %s\n", name, entries, fails == before ? "ok" : "FAIL");
  }
  {  // outside the enumerated set: the list of the RCCL self-test
    const int before = fails;
    int entries = 0;
    for (const DirSet &s : SETS) {
      const Lists L = build_self_lists(s);
      const Tally T = pair_all(L, comm_post_order);
      CHECK(T.wrong == 0, "own peer %s: %d of %d entries paired wrongly\n", s.name, T.wrong, T.entries);
      entries += T.entries;
    }
    printf("one rank its own peer in every direction: %d messages: %s\n", entries, fails == before ? "ok" : "FAIL");
    const Lists L4 = build_self_lists(SETS[2]);
    CHECK(pair_all(L4, order_recv_as_sends).wrong > 0 && pair_all(L4, order_recv_descending).wrong > 0, "own peer WESN: a wrong rule passes\n");
  }

  // ---- posting order of the periodic 2 x 2 face list, from the function and from the loops it replaced
  {
    const Lists L = build_lists(Topo{2, 2, true}, SETS[2]);
    for (int r = 0; r < 4; r++) {
      int so[COMM_MAX_XFER], ro[COMM_MAX_XFER], so0[COMM_MAX_XFER], ro0[COMM_MAX_XFER];
      comm_post_order(L.ptr[r], L.cnt[r], so, ro);
      order_before_the_move(L.ptr[r], L.cnt[r], so0, ro0);
      printf("periodic 2x2 WESN rank %d: so %d %d %d %d ro %d %d %d %d | before the move: so %d %d %d %d ro %d %d %d %d\n", r, so[0], so[1], so[2], so[3],
             ro[0], ro[1], ro[2], ro[3], so0[0], so0[1], so0[2], so0[3], ro0[0], ro0[1], ro0[2], ro0[3]);
    }
  }

  // ---- the wrong rules
  printf("wrong rule 'receives in the order of the sends' caught on %zu lists:\n", caught_same.size());
  for (auto &s : caught_same) printf("  same-order caught: %s\n", s.c_str());
  printf("wrong rule 'receives by descending tag' caught on %zu lists, %d of them face-only:\n", caught_desc.size(), desc_face_wrong);
  for (auto &s : caught_desc) printf("  descending caught: %s\n", s.c_str());
  auto has = [](const std::vector<std::string> &v, const char *s) {
    for (auto &e : v)
      if (e == s) return true;
    return false;
  };
  for (const char *t : {"periodic 2x1", "periodic 1x2", "periodic 2x2"})
    for (const char *s : {"WE", "SN"}) {
      char b[96];
      snprintf(b, sizeof b, "%s %s (tag)", t, s);
      CHECK(has(caught_same, b), "same-order rule is not reported as a tag error on %s %s\n", t, s);
    }
  CHECK(desc_face_wrong == 0, "descending rule fails a face-only list: it is meant to be wrong only beyond the faces\n");
  CHECK(has(caught_desc, "periodic 2x1 all8"), "descending rule passes the eight-direction list of periodic 2x1\n");

  // ---- broken lists: periodic 2 x 2, the four faces
  {
    Lists L = build_lists(Topo{2, 2, true}, SETS[2]);
    L.x[1].erase(L.x[1].begin());   // rank 1 no longer posts its W message (peer 0)
    L.refresh();
    int sr, si, nr = -1, ns = -1;
    // rank 0 receives two messages from rank 1 (its W and E neighbour), which now sends one
    const int code = comm_pair(L.ptr.data(), L.cnt.data(), 4, 0, 0, &sr, &si, &nr, &ns);
    CHECK(code == COMM_PAIR_NUMBER && nr == 2 && ns == 1, "dropped message: code %d, %d receives, %d sends\n", code, nr, ns);
    // rank 1's remaining receive from rank 0 sees the same defect from the other side
    const int code1 = comm_pair(L.ptr.data(), L.cnt.data(), 4, 1, 0, &sr, &si, &nr, &ns);
    CHECK(code1 == COMM_PAIR_NUMBER && nr == 1 && ns == 2, "dropped message, other side: code %d, %d receives, %d sends\n", code1, nr, ns);
    printf("broken list 'one message dropped': %s\n", code == COMM_PAIR_NUMBER && code1 == COMM_PAIR_NUMBER ? "refused with the number error" : "NOT refused");
  }
  {
    Lists L = build_lists(Topo{2, 2, true}, SETS[2]);
    L.x[2][3].count += 1;   // rank 2's N message (peer 0)
    L.refresh();
    int sr, si;
    int n_count = 0, n_other = 0;
    for (int r = 0; r < 4; r++)
      for (int k = 0; k < L.cnt[r]; k++) {
        const int code = comm_pair(L.ptr.data(), L.cnt.data(), 4, r, k, &sr, &si);
        // exactly the two ends of that message see it: rank 2's N receive and rank 0's S receive
        const bool end = (r == 2 && L.x[r][k].tag == DIR_N) || (r == 0 && L.x[r][k].tag == DIR_S);
        if (code == COMM_PAIR_COUNT && end) n_count++;
        else if (code != COMM_PAIR_OK || end) n_other++;
      }
    CHECK(n_count == 2 && n_other == 0, "changed count: %d count errors, %d other\n", n_count, n_other);
    printf("broken list 'one count changed': %s\n", n_count == 2 && n_other == 0 ? "refused with the count error" : "NOT refused");
  }
  {  // arguments out of range are refused, not read
    const Lists L = build_lists(Topo{2, 1, true}, SETS[0]);
    int sr, si;
    CHECK(comm_pair(L.ptr.data(), L.cnt.data(), 2, 2, 0, &sr, &si) == COMM_PAIR_ARG && comm_pair(L.ptr.data(), L.cnt.data(), 2, 0, 2, &sr, &si) == COMM_PAIR_ARG &&
              comm_pair(L.ptr.data(), L.cnt.data(), 2, -1, 0, &sr, &si) == COMM_PAIR_ARG && comm_pair(L.ptr.data(), L.cnt.data(), 1, 0, 0, &sr, &si) == COMM_PAIR_ARG,
          "an argument out of range is accepted\n");
  }
  printf("%d topologies, %d lists, %d messages checked, %d failures\n", ntopo, nlists, nentries, fails);
  return fails ? 1 : 0;
}
