// ndt_target_state.h -- what the host knows about "the target right now", and the only ways it changes (host only, no
// HIP type: plain C++ like ndt_packets.cpp and ndt_scan_model.cpp; tests/cpp/sanitize_target_state.cpp walks every
// transition from every state).  The fields are private: whoever produces or invalidates a target goes through
// retire / publish_* / drop / claim_cloud, and in the engine only target_retire, target_publish and target_drop
// (ndt_handoff.hip) call those.  DESIGN.md has the table of which call does what.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ndt {
namespace engine {

enum class TargetKind { NONE, SINGLE, UNION };   // no grid | one voxelised cloud (or a map's moments) | a multi-grid union

// The dense index grid is filled with -1 once per allocation; afterwards a build resets only the cells the previous one
// published (a 33 MB fill per build otherwise).  (0, 0) = nothing known: fill everything.
struct IndexReuse {
  size_t clean_cap = 0;   // capacity that is -1 everywhere except the dirty leaves' cells
  int dirty_slots = 0;    // slots of `stats` whose cells may hold an index
};

class TargetState {
 public:
  // The published target makes way for the one being produced.  kept_cloud_n: points of tx/ty/tz the new grid is built
  // from (0: nothing is kept).  The index-grid reuse pair goes to the caller and stays pessimistic until a publish.
  IndexReuse retire(size_t kept_cloud_n);
  void publish_single(size_t n_points, int n_slots, int n_valid, size_t index_cap);
  void publish_union(size_t n_points, int n_leaves);
  // The published grid must not be evaluated any more (its parameters changed, its scratch was reused, a tile left the
  // union).  A kept cloud stays.
  void drop();
  // tx/ty/tz are about to be overwritten: whatever is published, they are not its cloud any more.
  void claim_cloud() { cloud_n_ = 0; }

  TargetKind kind() const { return kind_; }
  bool have_grid() const { return kind_ != TargetKind::NONE; }
  bool is_union() const { return kind_ == TargetKind::UNION; }
  bool has_cloud() const { return cloud_n_ > 0; }
  size_t n_points() const { return n_points_; }     // points the target stands for (ndt_grid_info::n_target_points)
  size_t cloud_n() const { return cloud_n_; }       // the first cloud_n points of tx/ty/tz are the grid's cloud
  uint64_t gen() const { return gen_; }             // counts retirements: what the fitness index was built for
  int prev_n_valid() const { return prev_n_valid_; }   // valid voxels of the SINGLE the last retire replaced, else 0
  int n_slots() const { return n_slots_; }
  int n_valid() const { return n_valid_; }
  IndexReuse index_reuse() const { return reuse_; }

 private:
  TargetKind kind_ = TargetKind::NONE;
  size_t n_points_ = 0, cloud_n_ = 0;
  uint64_t gen_ = 0;
  int prev_n_valid_ = 0, n_slots_ = 0, n_valid_ = 0;
  IndexReuse reuse_;
};

}  // namespace engine
}  // namespace ndt
