// ndt_tuning.h -- the engine's tuning / A-B switches (internal).  One process-wide ndt_tuning (include/ndt_hip.h);
// the production library changes it only through ndt_set_tuning(), the diagnostic variants (-DNDT_TUNING_ENV:
// make VARIANT=ab|seams|stamps) also seed it from the historical NDT_* environment variables at first use.
#pragma once

#include "../../include/ndt_hip.h"

namespace ndt {

// The one read of the process-wide struct, by value.  A build, an evaluation, an align and a handle creation each take
// ONE snapshot when they begin and pass it down: everything they size and launch follows that one configuration,
// whatever ndt_set_tuning() does on another thread meanwhile.
ndt_tuning tuning_snapshot();
void tuning_defaults(ndt_tuning* t);
int tuning_set(const ndt_tuning* t);  // NDT_OK | NDT_ERR_INVALID_ARG

}  // namespace ndt
