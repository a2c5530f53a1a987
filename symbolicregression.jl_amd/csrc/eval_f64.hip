// eval_f64.hip — double variants of eval_kernel (see eval_kernel.h):
//   R = 4 rows per lane, kShallowSlots stack slots, basic or full operator set
//   R = 2 rows per lane, kMaxSlots stack slots (deep trees), full operator set
#include "eval_kernel.h"

namespace srhip {

template <>
hipError_t launch_eval<double>(const EvalPlan& plan, const EvalArgs<double>& a, int mode, hipStream_t stream) {
  if (plan.wide) return launch_eval_wide<double>(plan, a, mode, stream);  // eval_wide_f64.hip
  if (plan.D == kMaxSlots) {
    // deep trees; a list that holds expression operators runs the variant that
    // dispatches their micro-instructions
    if (plan.opset == OPSET_EXPR) return launch_rd<double, 2, kMaxSlots, OPSET_EXPR>(plan, a, mode, stream);
    return launch_rd<double, 2, kMaxSlots, OPSET_FULL>(plan, a, mode, stream);
  }
  if (plan.opset == OPSET_BASIC) return launch_rd<double, 4, kShallowSlots, OPSET_BASIC>(plan, a, mode, stream);
  return launch_rd<double, 4, kShallowSlots, OPSET_FULL>(plan, a, mode, stream);
}

}  // namespace srhip
