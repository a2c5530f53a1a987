// grad_deriv_f64.hip — double derivative-objective variants of grad_kernel (grad_kernel.h
// kGradLossDeriv): tangents seeded at feature leaves, a table loss reduced on ŷ and on
// each ∂ŷ/∂x_dir in the same pass over a row tile that holds every column of the
// dataset (srhip_eval_loss_deriv). Weighted or not, the full operator set: the
// shallow variants at 1, 2 and kGradG tangents, the deep one, the wide one, and
// the finalisation of their partials.
#include "grad_kernel.h"

namespace srhip {

template <>
hipError_t launch_grad_deriv<double>(const EvalPlan& plan, const GradArgs<double>& a, hipStream_t stream) {
  return launch_grad_deriv_all<double>(plan, a, stream);
}

template <>
hipError_t launch_grad_deriv_finalize<double>(const GradArgs<double>& a, double* out_sum, uint8_t* out_ok,
                                       hipStream_t stream) {
  return launch_grad_deriv_finalize_all<double>(a, out_sum, out_ok, stream);
}

}  // namespace srhip
