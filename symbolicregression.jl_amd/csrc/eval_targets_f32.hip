// eval_targets_f32.hip — float per-tree-targets variants of eval_kernel
// (eval_kernel.h kModeLossTargets): the row tile holds every target column of a
// multi-target dataset and each tree reads its own. Full operator set only:
//   R = 8, kShallowSlots; R = 4, kMaxSlots (with and without the expression
//   operators' micro-instructions); the wide variant (features from global memory)
#include "eval_kernel.h"

namespace srhip {

template <>
hipError_t launch_eval_targets<float>(const EvalPlan& plan, const EvalArgs<float>& a, hipStream_t stream) {
  if (plan.wide) return launch_targets_rd<float, 4, kMaxSlots, OPSET_EXPR, true>(plan, a, stream);
  if (plan.D == kMaxSlots) {
    if (plan.opset == OPSET_EXPR) return launch_targets_rd<float, 4, kMaxSlots, OPSET_EXPR>(plan, a, stream);
    return launch_targets_rd<float, 4, kMaxSlots, OPSET_FULL>(plan, a, stream);
  }
  return launch_targets_rd<float, SR_R32, kShallowSlots, OPSET_FULL>(plan, a, stream);
}

}  // namespace srhip
