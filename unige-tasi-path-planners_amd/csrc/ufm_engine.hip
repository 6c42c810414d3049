// ufm_engine.hip -- MI355X (gfx950) cost-propagation engine behind include/ufm.h.
//
// What it replaces: the priority-queue driven G/RHS wavefront of the reference
// replanners -- ReplannerBase::step (ProjectToolkit/include/ReplannerBase.h:43-75)
// with FieldDPlanner / ShiftedGridPlanner / DFMPlanner init/update/plan
// (FieldDStar/FieldDPlanner_impl.h:15-163, ShiftedGridFastMarching/
// ShiftedGridPlanner_impl.h:9-231, DynamicFastMarching/DynamicFastMarching_impl.h:6-132).
//
// How: the serial D*-Lite expansion order is replaced by a block Fast Iterative Method ordered
// like fast marching at tile granularity.  The field G lives densely in HBM; the domain is cut
// into UFM_TILE x UFM_TILE-element tiles (16 by default); per-tile priorities (the smallest value
// that entered a tile since its last visit) drive launches of k_relax, which releases the tiles of
// the current band, stages each (+1 halo) in LDS, sweeps it to its local fixed point with
// asynchronous waves (one 4x4-node patch per wave, four lanes per node), writes it back and queues
// the neighbours whose halo changed.  The fixed point G = F(G) is unique (costs >= 1), so it equals
// the reference's consistent field.  Map patches (cost increases) are handled by an invalidation
// ("raise") phase -- an element whose value is no longer supported by its neighbours is reset to
// +inf, transitively -- followed by the usual lowering phase; both stop at the start's key like the
// reference's end_condition and keep the rest queued across steps.  DESIGN.md has the full story.
//
// Arithmetic contract (bit parity with oracle/ufm_oracle.c): IEEE fp32, one
// rounding per operation (-ffp-contract=off), correctly rounded sqrt.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <thread>
#include <vector>

#include "../../include/ufm.h"

namespace {

#include "ufm_diag.h"
#include "ufm_defs.h"
#include "ufm_ops.h"
#include "ufm_relax.h"
#include "ufm_control.h"

#include "ufm_region.h"
#include "ufm_cspace.h"
#include "ufm_cspace_graded.h"
#include "ufm_census.h"
#include "ufm_sensor.h"
#include "ufm_prepare.h"
#include "ufm_layers.h"

#include "ufm_host.h"
#include "ufm_map_host.h"
#include "ufm_delta.h"

}  // namespace

// ---- the readers of the diagnostic builds' records (libufm_timing.so, libufm_sstat.so) ----
#include "ufm_diag_host.h"

// ---- C ABI ---------------------------------------------------------------------------
#include "ufm_capi.h"
