// grad_deriv_f32.hip — float derivative-objective variants of grad_kernel (grad_kernel.h
// kGradLossDeriv): tangents seeded at feature leaves, a table loss reduced on ŷ and on
// each ∂ŷ/∂x_dir in the same pass over a row tile that holds every column of the
// dataset (srhip_eval_loss_deriv). Weighted or not, the full operator set: the
// shallow variants at 1, 2 and kGradG tangents, the deep one, the wide one, and
// the finalisation of their partials.
#include "grad_kernel.h"

namespace srhip {

template <>
hipError_t launch_grad_deriv<float>(const EvalPlan& plan, const GradArgs<float>& a, hipStream_t stream) {
  return launch_grad_deriv_all<float>(plan, a, stream);
}

template <>
hipError_t launch_grad_deriv_finalize<float>(const GradArgs<float>& a, double* out_sum, uint8_t* out_ok,
                                       hipStream_t stream) {
  return launch_grad_deriv_finalize_all<float>(a, out_sum, out_ok, stream);
}

}  // namespace srhip
