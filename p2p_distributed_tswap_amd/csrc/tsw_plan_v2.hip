// tsw_plan_v2.hip — one instantiation of k_plan (tsw_plan_kernel.h), in a translation unit of its own so that the build
// compiles the seven in parallel. launch_plan (tsw_plan.hip) says which PlanArgs it serves.
#include "tsw_plan_kernel.h"

namespace tsw {
template hipError_t launch_plan_t<true, false, false, false>(const PlanArgs*, const WorkerArgs&, uint32_t, size_t, uint32_t, hipStream_t);
}  // namespace tsw
