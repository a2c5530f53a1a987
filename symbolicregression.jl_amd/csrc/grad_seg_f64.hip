// grad_seg_f64.hip — double per-tree row-set variants of grad_kernel (grad_kernel.h
// SEG): one work item per workgroup, each staging its tree's own gathered sample
// (srhip_eval_loss_grad_rowsets, srhip_optimize_constants_rowsets). Every loss
// variant of grad_kernels.hip, the wide ones included; no per-row outputs.
#include "grad_kernel.h"

namespace srhip {

template <>
hipError_t launch_grad_seg<double>(const EvalPlan& plan, const GradArgs<double>& a, int mode, hipStream_t stream) {
  return launch_grad_all<double, true>(plan, a, mode, stream);
}

}  // namespace srhip
