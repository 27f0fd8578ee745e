// csrc/ndt_target_state.cpp (host only) under AddressSanitizer + UBSan as a stand-alone program: every transition from
// every reachable state against the invariants written out in check(), a random walk of 10^5 transitions under the
// same invariants, and the call sequence that once made ndt_set_params re-voxelise a union's point count of a smaller
// kept cloud, replayed as state transitions.  Prints PASS.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "ndt_target_state.h"

using namespace ndt::engine;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

namespace {

enum Op { RETIRE, PUBLISH_SINGLE, PUBLISH_UNION, DROP, CLAIM };
struct Step {
  Op op;
  size_t a;       // retire: kept_cloud_n; publish: n_points
  int slots, valid;
  size_t cap;
};

// what the test itself remembers, independently of the state's fields
struct Shadow {
  IndexReuse stored;        // the pair the last publish stored, (0, 0) once handed out
  bool cloud = false;       // a retire kept a cloud and nothing has claimed it or published a union since
  bool pending = false;     // retired and not yet published: the engine publishes only then
};

auto key(const TargetState& s) {
  return std::make_tuple((int)s.kind(), s.n_points(), s.cloud_n(), s.prev_n_valid(), s.n_slots(), s.n_valid(), s.index_reuse().clean_cap,
                         s.index_reuse().dirty_slots);
}

void invariants(const TargetState& s) {
  CHECK(s.have_grid() == (s.kind() != TargetKind::NONE));
  CHECK(s.is_union() == (s.kind() == TargetKind::UNION));
  CHECK(s.has_cloud() == (s.cloud_n() > 0));
  if (s.kind() == TargetKind::NONE) CHECK(s.n_valid() == 0);
  if (s.kind() == TargetKind::UNION) {
    CHECK(s.cloud_n() == 0);
    CHECK(s.index_reuse().clean_cap == 0 && s.index_reuse().dirty_slots == 0);
    CHECK(s.n_slots() == s.n_valid());
  }
  CHECK(s.n_valid() >= 0 && s.n_slots() >= 0 && s.prev_n_valid() >= 0);
}

// one transition, checked against the state before it
void apply(TargetState& s, Shadow& sh, const Step& st) {
  const TargetState before = s;
  switch (st.op) {
    case RETIRE: {
      const IndexReuse got = s.retire(st.a);
      CHECK(s.gen() > before.gen());                                    // strictly increases
      CHECK(got.clean_cap == sh.stored.clean_cap && got.dirty_slots == sh.stored.dirty_slots);   // exactly what the last publish stored
      CHECK(s.index_reuse().clean_cap == 0 && s.index_reuse().dirty_slots == 0);
      CHECK(s.prev_n_valid() == (before.kind() == TargetKind::SINGLE ? before.n_valid() : 0));
      if (before.kind() != TargetKind::SINGLE) CHECK(s.prev_n_valid() == 0);
      CHECK(s.kind() == TargetKind::NONE && s.n_points() == 0 && s.n_slots() == 0 && s.n_valid() == 0);
      CHECK(s.cloud_n() == st.a);
      sh.stored = IndexReuse{};
      sh.cloud = st.a > 0;
      sh.pending = true;
      break;
    }
    case PUBLISH_SINGLE:
      s.publish_single(st.a, st.slots, st.valid, st.cap);
      CHECK(s.kind() == TargetKind::SINGLE && s.n_points() == st.a && s.n_slots() == st.slots && s.n_valid() == st.valid);
      CHECK(s.index_reuse().clean_cap == st.cap && s.index_reuse().dirty_slots == st.slots);
      CHECK(s.cloud_n() == before.cloud_n() && s.gen() == before.gen() && s.prev_n_valid() == before.prev_n_valid());
      sh.stored.clean_cap = st.cap;
      sh.stored.dirty_slots = st.slots;
      sh.pending = false;
      break;
    case PUBLISH_UNION:
      s.publish_union(st.a, st.slots);
      CHECK(s.kind() == TargetKind::UNION && s.n_points() == st.a && s.n_slots() == st.slots && s.n_valid() == st.slots);
      CHECK(s.gen() == before.gen() && s.prev_n_valid() == before.prev_n_valid());
      sh.stored = IndexReuse{};
      sh.cloud = false;
      sh.pending = false;
      break;
    case DROP:
      s.drop();
      CHECK(s.kind() == TargetKind::NONE && s.n_valid() == 0);
      CHECK(s.cloud_n() == before.cloud_n() && s.gen() == before.gen() && s.n_points() == before.n_points() &&
            s.n_slots() == before.n_slots() && s.prev_n_valid() == before.prev_n_valid());
      CHECK(s.index_reuse().clean_cap == before.index_reuse().clean_cap && s.index_reuse().dirty_slots == before.index_reuse().dirty_slots);
      break;
    case CLAIM:
      s.claim_cloud();
      CHECK(!s.has_cloud());
      CHECK(s.kind() == before.kind() && s.gen() == before.gen() && s.n_points() == before.n_points() && s.n_slots() == before.n_slots() &&
            s.n_valid() == before.n_valid() && s.prev_n_valid() == before.prev_n_valid());
      CHECK(s.index_reuse().clean_cap == before.index_reuse().clean_cap && s.index_reuse().dirty_slots == before.index_reuse().dirty_slots);
      sh.cloud = false;
      break;
  }
  invariants(s);
  CHECK(s.has_cloud() == sh.cloud);   // claim_cloud followed by no retire leaves has_cloud() false, whatever is published
  CHECK(s.index_reuse().clean_cap == sh.stored.clean_cap && s.index_reuse().dirty_slots == sh.stored.dirty_slots);
}

// the transitions a state admits: the engine publishes only what it has retired for (target_publish follows target_retire)
std::vector<Step> moves(const Shadow& sh) {
  std::vector<Step> m = {{RETIRE, 0, 0, 0, 0}, {RETIRE, 1334, 0, 0, 0}, {DROP, 0, 0, 0, 0}, {CLAIM, 0, 0, 0, 0}};
  if (sh.pending) {
    m.push_back({PUBLISH_SINGLE, 1334, 40, 31, 4096});
    m.push_back({PUBLISH_SINGLE, 9, 0, 0, 64});          // a grid without a leaf (a map whose box holds none)
    m.push_back({PUBLISH_UNION, 5808, 77, 77, 0});
  }
  return m;
}

// every transition from every reachable state (gen left out of a state's identity: it only counts)
size_t exhaustive() {
  struct Node { TargetState s; Shadow sh; };
  std::set<decltype(std::tuple_cat(key(TargetState{}), std::make_tuple(false)))> seen;
  std::vector<Node> frontier = {Node{}};
  invariants(frontier[0].s);
  CHECK(!frontier[0].s.have_grid() && !frontier[0].s.has_cloud() && frontier[0].s.gen() == 0);
  seen.insert(std::tuple_cat(key(frontier[0].s), std::make_tuple(false)));
  size_t edges = 0;
  while (!frontier.empty()) {
    std::vector<Node> next;
    for (const Node& n : frontier)
      for (const Step& st : moves(n.sh)) {
        Node c = n;
        apply(c.s, c.sh, st);
        ++edges;
        if (seen.insert(std::tuple_cat(key(c.s), std::make_tuple(c.sh.pending))).second) next.push_back(c);
      }
    frontier.swap(next);
  }
  CHECK(seen.size() > 20);
  return edges;
}

void random_walk(size_t steps) {
  std::mt19937_64 rng(20261019);
  TargetState s;
  Shadow sh;
  uint64_t gen = 0;
  for (size_t i = 0; i < steps; ++i) {
    Step st{};
    static const Op table[7] = {RETIRE, RETIRE, RETIRE, DROP, CLAIM, PUBLISH_SINGLE, PUBLISH_UNION};   // (publishes only while pending)
    st.op = table[rng() % (sh.pending ? 7 : 5)];
    st.a = st.op == RETIRE ? (rng() % 3 ? (size_t)(rng() % 100000) : 0) : (size_t)(rng() % 5000000);
    st.slots = (int)(rng() % 50000);
    st.valid = st.slots ? (int)(rng() % (uint64_t)(st.slots + 1)) : 0;
    st.cap = (size_t)(rng() % (1u << 30));
    apply(s, sh, st);
    if (st.op == RETIRE) ++gen;
    CHECK(s.gen() == gen);
  }
}

// addTarget x3, setInputTarget(small host cloud), createVoxelKdtree, setResolution -- as the engine's calls make them
void replay_reduced_fuzz_sequence() {
  TargetState s;
  Shadow sh;
  const size_t tiles[3] = {1936, 1936, 1936}, small = 1334;
  size_t total = 0;
  for (size_t n : tiles) {   // ndt_multigrid_add_target: a build from scratch arrays, then the table is only scratch
    apply(s, sh, {RETIRE, 0, 0, 0, 0});
    apply(s, sh, {PUBLISH_SINGLE, n, 60, 50, 1 << 20});
    apply(s, sh, {DROP, 0, 0, 0, 0});
    CHECK(!s.have_grid() && !s.has_cloud());
    total += n;
  }
  apply(s, sh, {CLAIM, 0, 0, 0, 0});   // ndt_set_target: the upload, then the build from the engine's own arrays
  apply(s, sh, {RETIRE, small, 0, 0, 0});
  apply(s, sh, {PUBLISH_SINGLE, small, 45, 40, 1 << 20});
  CHECK(s.kind() == TargetKind::SINGLE && s.cloud_n() == small && s.n_points() == small);
  apply(s, sh, {RETIRE, 0, 0, 0, 0});   // ndt_multigrid_create_kdtree
  apply(s, sh, {PUBLISH_UNION, total, 150, 150, 0});
  CHECK(s.is_union() && s.n_points() == total && total > small);
  CHECK(s.cloud_n() == 0);             // ndt_set_params: grid_changed && has_cloud() is false -> no rebuild from a cloud that is not the union's
  CHECK(!s.has_cloud());
  apply(s, sh, {DROP, 0, 0, 0, 0});    // ... the union is dropped instead
  CHECK(!s.have_grid() && s.n_valid() == 0);
}

// a producer that claimed the arrays and then failed: the surviving target has no cloud, whatever it was
void claim_without_publish() {
  for (int kind = 0; kind < 2; ++kind) {
    TargetState s;
    Shadow sh;
    apply(s, sh, {RETIRE, kind == 0 ? (size_t)500 : (size_t)0, 0, 0, 0});
    if (kind == 0) apply(s, sh, {PUBLISH_SINGLE, 500, 20, 10, 256});
    else apply(s, sh, {PUBLISH_UNION, 900, 30, 30, 0});
    apply(s, sh, {CLAIM, 0, 0, 0, 0});
    CHECK(s.have_grid() && !s.has_cloud() && s.cloud_n() == 0);
    apply(s, sh, {DROP, 0, 0, 0, 0});
    CHECK(!s.has_cloud());
  }
}

}  // namespace

int main() {
  const size_t edges = exhaustive();
  random_walk(100000);
  replay_reduced_fuzz_sequence();
  claim_without_publish();
  std::printf("%zu transitions from every reachable state, 100000 random ones\nPASS\n", edges);
  return 0;
}
