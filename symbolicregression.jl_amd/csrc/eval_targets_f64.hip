// eval_targets_f64.hip — double per-tree-targets variants of eval_kernel
// (eval_kernel.h kModeLossTargets): the row tile holds every target column of a
// multi-target dataset and each tree reads its own. Full operator set only:
//   R = 4, kShallowSlots; R = 2, kMaxSlots (with and without the expression
//   operators' micro-instructions); the wide variant (features from global memory)
#include "eval_kernel.h"

namespace srhip {

template <>
hipError_t launch_eval_targets<double>(const EvalPlan& plan, const EvalArgs<double>& a, hipStream_t stream) {
  if (plan.wide) return launch_targets_rd<double, 2, kMaxSlots, OPSET_EXPR, true>(plan, a, stream);
  if (plan.D == kMaxSlots) {
    if (plan.opset == OPSET_EXPR) return launch_targets_rd<double, 2, kMaxSlots, OPSET_EXPR>(plan, a, stream);
    return launch_targets_rd<double, 2, kMaxSlots, OPSET_FULL>(plan, a, stream);
  }
  return launch_targets_rd<double, 4, kShallowSlots, OPSET_FULL>(plan, a, stream);
}

}  // namespace srhip
