// grad_deriv2_f32.hip — float variants of the second-order kernel (grad_deriv2.h):
// constant gradients of a derivative objective (srhip_eval_loss_grad_deriv) and the
// per-row mixed partials (srhip_eval_mixed_tree_array). Shallow (R = 4 and R = 2) and
// deep, weighted or not, the full operator set; their finalisation; and the choice of
// variant and geometry for both element types.
#include "grad_deriv2.h"

namespace srhip {

void deriv2_variant(int dtype, bool deep, int ndir, int* R, int* GC) {
  // R: grad_kernel.h grad_R at the tangent count srhip_eval_loss_deriv carries
  *R = (dtype != SRHIP_F32 || deep) ? 1 : (ndir <= 2 ? 4 : 2);
  *GC = (dtype != SRHIP_F32 && deep) ? 1 : 2;
}

bool plan_grad_deriv2(int dtype, bool deep, int ndir, int mode, bool weighted, int nfeat, int64_t n, int nitems,
                      EvalPlan* p) {
  const size_t esz = dtype == SRHIP_F32 ? 4 : 8;
  int R, GC;
  deriv2_variant(dtype, deep, ndir, &R, &GC);
  const int narr = nfeat + (mode == DERIV2_LOSS ? (1 + ndir) * (weighted ? 2 : 1) : 0);
  return plan_geometry(esz, R, deep ? kMaxSlots : 4, narr, (3 + 2 * GC) * esz, n, nitems, p);
}

template <>
hipError_t launch_grad_deriv2<float>(const EvalPlan& plan, const Deriv2Args<float>& a, int mode, hipStream_t stream) {
  return launch_grad_deriv2_all<float>(plan, a, mode, stream);
}

template <>
hipError_t launch_grad_deriv2_finalize<float>(const Deriv2Args<float>& a, double* out_loss, double* out_grad,
                                              uint8_t* out_ok, hipStream_t stream) {
  return launch_grad_deriv2_finalize_all<float>(a, out_loss, out_grad, out_ok, stream);
}

}  // namespace srhip
