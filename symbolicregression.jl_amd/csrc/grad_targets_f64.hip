// grad_targets_f64.hip — double per-tree-targets variants of grad_kernel (grad_kernel.h
// TG): the row tile holds every target column of a multi-target dataset and each
// work item reads its tree's own (srhip_eval_loss_grad_targets,
// srhip_optimize_constants_targets). Table losses only, weighted or not: the
// shallow variants at 1, 2 and kGradG tangents, the deep one, the wide one. Row-set
// calls need none of these: their gather picks each tree's column (grad_seg_*.hip).
#include "grad_kernel.h"

namespace srhip {

template <>
hipError_t launch_grad_targets<double>(const EvalPlan& plan, const GradArgs<double>& a, int mode, hipStream_t stream) {
  return launch_grad_targets_all<double>(plan, a, mode, stream);
}

}  // namespace srhip
