// eval_wide_f64.hip — double wide variants of eval_kernel (eval_kernel.h XG; see
// eval_wide_f32.hip): R = 2 rows per lane, kMaxSlots stack slots, the full
// operator set with the expression operators' micro-instructions.
#include "eval_kernel.h"

namespace srhip {

template <>
hipError_t launch_eval_wide<double>(const EvalPlan& plan, const EvalArgs<double>& a, int mode, hipStream_t stream) {
  return launch_rd<double, 2, kMaxSlots, OPSET_EXPR, true>(plan, a, mode, stream);
}

}  // namespace srhip
