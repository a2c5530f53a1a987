// grad_deriv2_f64.hip — double variants of the second-order kernel (grad_deriv2.h):
// constant gradients of a derivative objective (srhip_eval_loss_grad_deriv) and the
// per-row mixed partials (srhip_eval_mixed_tree_array). Shallow and deep, weighted or
// not, the full operator set, and their finalisation.
#include "grad_deriv2.h"

namespace srhip {

template <>
hipError_t launch_grad_deriv2<double>(const EvalPlan& plan, const Deriv2Args<double>& a, int mode,
                                      hipStream_t stream) {
  return launch_grad_deriv2_all<double>(plan, a, mode, stream);
}

template <>
hipError_t launch_grad_deriv2_finalize<double>(const Deriv2Args<double>& a, double* out_loss, double* out_grad,
                                               uint8_t* out_ok, hipStream_t stream) {
  return launch_grad_deriv2_finalize_all<double>(a, out_loss, out_grad, out_ok, stream);
}

}  // namespace srhip
