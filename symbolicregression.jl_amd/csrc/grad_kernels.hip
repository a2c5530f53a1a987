// grad_kernels.hip — constant-gradient kernels (forward mode, fused with the
// loss): the batched replacement for ConstantOptimization.jl's gradients
// (src/ConstantOptimization.jl:12-65 evaluates the loss by finite
// differences; eval_grad_tree_array(...; variable=false),
// src/InterfaceDynamicExpressions.jl:105-107, gives ∂ŷ/∂c per row).
//
// Same workgroup structure as eval_kernel (row group staged in LDS, waves take
// work items round-robin); a work item is (tree, tangent group of kGradG
// constants). GRAD_LOSS returns Σ w·ℓ and Σ w·ℓ'(r)·∂ŷ/∂c_k per constant;
// GRAD_OUT writes ŷ and ∂ŷ/∂c_k per row.
#include "grad_kernel.h"

namespace srhip {
namespace {

using namespace interp;

template <typename T, int G>
__global__ void __launch_bounds__(256) grad_finalize_kernel(GradArgs<T> a, double* __restrict__ out_sum,
                                                            uint8_t* __restrict__ out_ok,
                                                            double* __restrict__ out_dloss) {
  constexpr int S = 2 + G;
  __shared__ double sh[4][S][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int npos = a.ntg * a.tpb;
  const int pos = blockIdx.x * 64 + lane;
  double acc[S];
  for (int k = 0; k < S; ++k) acc[k] = 0.0;
  if (pos < npos) {
    for (int rg = w; rg < a.nrg; rg += 4) {
      const T* q = a.partial + ((size_t)rg * npos + pos) * S;
      for (int k = 0; k < S; ++k) acc[k] += (double)q[k];
    }
  }
  for (int k = 0; k < S; ++k) sh[w][k][lane] = acc[k];
  __syncthreads();
  if (w == 0 && pos < npos) {
    for (int k = 0; k < S; ++k) acc[k] = (sh[0][k][lane] + sh[1][k][lane]) + (sh[2][k][lane] + sh[3][k][lane]);
    const int g = pos / a.tpb;
    const int i = pos - g * a.tpb;
    const int sidx = i * a.ntg + ((i & 1) ? (a.ntg - 1 - g) : g);
    if (sidx < a.nitems) {
      const int item = a.items[sidx];
      const int t = item & 0xffffff;
      const int g0 = (item >> 24) * kGradG;
      const bool ok = !__builtin_isnan(acc[1]);
      if (g0 == 0) {
        out_sum[t] = ok ? acc[0] : __builtin_nan("");
        out_ok[t] = ok ? 1 : 0;
      }
      const int cb = a.const_off[t];
      const int nc = a.const_off[t + 1] - cb;
      for (int j = 0; j < G; ++j)
        if (g0 + j < nc) out_dloss[cb + g0 + j] = ok ? acc[2 + j] : __builtin_nan("");
    }
  }
}

}  // namespace

bool plan_grad(int dtype, bool deep, int G, int mode, bool weighted, int nfeat, int64_t n, int nitems,
               EvalPlan* p, int ntgt) {
  const size_t esz = dtype == SRHIP_F32 ? 4 : 8;
  const int ncol = ntgt > 0 ? ntgt : 1;  // columns of y (and of w) in the tile
  const int narr = nfeat + (mode == GRAD_LOSS ? ncol * (weighted ? 2 : 1) : 0);
  return plan_geometry(esz, grad_R(dtype, deep, G), deep ? kMaxSlots : 4, narr, (2 + G) * esz, n, nitems, p);
}

bool plan_grad_wide(int dtype, int mode, bool weighted, int64_t n, int nitems, EvalPlan* p, int ntgt) {
  const size_t esz = dtype == SRHIP_F32 ? 4 : 8;
  const int ncol = ntgt > 0 ? ntgt : 1;
  const int narr = mode == GRAD_LOSS ? ncol * (weighted ? 2 : 1) : 0;  // y, w: no feature array
  const bool ok = plan_geometry(esz, grad_R(dtype, true, kGradG), kMaxSlots, narr, (2 + kGradG) * esz, n, nitems, p);
  p->wide = true;
  return ok;
}

template <typename T>
hipError_t launch_grad(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream) {
  if (a.seg > 0) return launch_grad_seg<T>(plan, a, mode, stream);  // grad_seg_f32.hip / grad_seg_f64.hip
  if (a.tgt) return launch_grad_targets<T>(plan, a, mode, stream);  // grad_targets_f32.hip / grad_targets_f64.hip
  return launch_grad_all<T, false>(plan, a, mode, stream);
}

template <typename T>
hipError_t launch_grad_finalize(const GradArgs<T>& a, double* out_sum, uint8_t* out_ok, double* out_dloss,
                                hipStream_t stream) {
  const int npos = a.ntg * a.tpb;
  const unsigned grid = (unsigned)((npos + 63) / 64);
  if (a.G == 1)
    hipLaunchKernelGGL((grad_finalize_kernel<T, 1>), dim3(grid), dim3(256), 0, stream, a, out_sum, out_ok, out_dloss);
  else if (a.G == 2)
    hipLaunchKernelGGL((grad_finalize_kernel<T, 2>), dim3(grid), dim3(256), 0, stream, a, out_sum, out_ok, out_dloss);
  else
    hipLaunchKernelGGL((grad_finalize_kernel<T, kGradG>), dim3(grid), dim3(256), 0, stream, a, out_sum, out_ok,
                       out_dloss);
  return hipGetLastError();
}

template hipError_t launch_grad<float>(const EvalPlan&, const GradArgs<float>&, int, hipStream_t);
template hipError_t launch_grad<double>(const EvalPlan&, const GradArgs<double>&, int, hipStream_t);
template hipError_t launch_grad_finalize<float>(const GradArgs<float>&, double*, uint8_t*, double*, hipStream_t);
template hipError_t launch_grad_finalize<double>(const GradArgs<double>&, double*, uint8_t*, double*,
                                                 hipStream_t);

}  // namespace srhip
