// ndt_target_state.cpp -- the target's transitions (see ndt_target_state.h).
#include "ndt_target_state.h"

namespace ndt {
namespace engine {

IndexReuse TargetState::retire(size_t kept_cloud_n) {
  prev_n_valid_ = kind_ == TargetKind::SINGLE ? n_valid_ : 0;   // (first_eval_behind_build's size guess)
  kind_ = TargetKind::NONE;
  n_points_ = 0;
  n_slots_ = n_valid_ = 0;
  ++gen_;   // (the fitness index, if any, is rebuilt by the next fitness call)
  cloud_n_ = kept_cloud_n;
  const IndexReuse was = reuse_;
  reuse_ = IndexReuse{};   // pessimistic until the new target has gone through
  return was;
}

void TargetState::publish_single(size_t n_points, int n_slots, int n_valid, size_t index_cap) {
  kind_ = TargetKind::SINGLE;
  n_points_ = n_points;
  n_slots_ = n_slots;
  n_valid_ = n_valid;
  reuse_.clean_cap = index_cap;
  reuse_.dirty_slots = n_slots;
}

void TargetState::publish_union(size_t n_points, int n_leaves) {
  kind_ = TargetKind::UNION;
  n_points_ = n_points;
  n_slots_ = n_valid_ = n_leaves;
  cloud_n_ = 0;            // a union keeps no cloud
  reuse_ = IndexReuse{};   // its index was filled whole: the next ordinary build starts from a cleared one
}

void TargetState::drop() {
  kind_ = TargetKind::NONE;
  n_valid_ = 0;
}

}  // namespace engine
}  // namespace ndt
