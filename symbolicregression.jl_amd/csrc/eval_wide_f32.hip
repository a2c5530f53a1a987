// eval_wide_f32.hip — float wide variants of eval_kernel (eval_kernel.h XG): the
// feature operands come from global memory, for datasets whose row tile does
// not fit in LDS. One configuration: R = 4 rows per lane, kMaxSlots stack
// slots, the full operator set with the expression operators' micro-
// instructions (a superset of every program the other variants run).
#include "eval_kernel.h"

namespace srhip {

template <>
hipError_t launch_eval_wide<float>(const EvalPlan& plan, const EvalArgs<float>& a, int mode, hipStream_t stream) {
  return launch_rd<float, 4, kMaxSlots, OPSET_EXPR, true>(plan, a, mode, stream);
}

}  // namespace srhip
