// grad_kernel.h — the constant-gradient kernel (forward mode, fused with the
// loss) and its launch dispatch, shared by grad_kernels.hip (the variants over
// shared rows) and grad_seg_f32.hip / grad_seg_f64.hip (per-tree row sets).
//
// Same workgroup structure as eval_kernel (row group staged in LDS, waves take
// work items round-robin); a work item is (tree, tangent group of kGradG
// constants). GRAD_LOSS returns Σ w·ℓ and Σ w·ℓ'(r)·∂ŷ/∂c_k per constant;
// GRAD_OUT writes ŷ and ∂ŷ/∂c_k per row.
#pragma once
#include <hip/hip_runtime.h>

#include "grad_interp.h"
#include "kernels.h"

namespace srhip {
namespace {

using namespace interp;

// Kernel mode of a GRAD_LOSS launch whose loss is an expression loss (a.loss >=
// SRHIP_EXPR_LOSS_BEGIN): (ℓ, dℓ/dŷ) per row come from the loss program in dual
// numbers (grad_interp.h run_loss_dual) in place of elem_loss / elem_dloss, with
// no implicit weight. Instantiations of their own (full operator set; the weight
// column is the run-time a.w): the others keep their code.
constexpr int kGradLossExpr = 2;

// Kernel mode of a derivative objective (srhip_eval_loss_deriv): the tangents are
// those of G features, the directions a.dir[g0 .. g0+G-1] (grad_interp.h FEAT), and
// a table loss is reduced per channel in the same pass. The row tile stages the
// a.ntgt = 1 + ndir columns of y (and of w) as TG does: column 0 is y, column 1 + k
// the target of ∂ŷ/∂x_dir[k]. Per row, acc[0] += w₀·ℓ(ŷ, y) and acc[2 + j] +=
// w_c·ℓ(∂ŷ/∂x_dir[g0+j], Y[c]) with c = 1 + g0 + j: the derivative stands in the
// prediction's place. A slot past the last direction reads no column and stays 0.
//
// The engine's rule for the flag: acc[1] is the marker of the value evaluation
// only, as in GRAD_LOSS, so a tree's ok is its did_succeed (the rule
// eval_diff_tree_array follows here); a non-finite derivative gives a non-finite
// channel sum with ok = 1 (the expression losses' rule). Parity
// with DynamicExpressions' own completion flag for derivatives is unpinned.
// Instantiations of their own (grad_deriv_f32.hip / grad_deriv_f64.hip; the full
// operator set): the others keep their code.
constexpr int kGradLossDeriv = 3;

// XG: the wide variant (eval_kernel.h): y and w staged in LDS only, the programs'
// feature operands read from a.X in global memory.
//
// SEG: per-tree row sets (srhip_eval_loss_grad_rowsets; GRAD_LOSS and kGradLossExpr
// only). The launch has one work item per workgroup of one wave (a.tpb = 1, a.ntg =
// a.nitems, slot g is item g), and the workgroup stages its tree's own segment: rows
// [a.seg·t + row0, …) of the gathered X / y / w. a.ntiles and a.nrg are those of a
// dataset of a.n rows, so an item's tiles, lane sums, shuffle tree and row-group
// partials are the ones it has in a launch over such a dataset. A template
// parameter: the instantiations without it keep their code.
//
// TG: a target per tree (srhip_eval_loss_grad_targets; GRAD_LOSS only, never with
// SEG: a row-set launch gathers each tree's own column into its segment). a.y / a.w
// are a.ntgt columns, n_pad rows apart; the row tile stages all of them and a work
// item reads column a.tgt[t] of its tree. With one column an item's arithmetic is
// the plain kernel's. A template parameter, as SEG: the others keep their code.
template <typename T, int R, int D, int MODE, bool W, int G, int SET, bool XG = false, bool SEG = false,
          bool TG = false>
__global__ void __launch_bounds__(256) grad_kernel(GradArgs<T> a) {
  static_assert(!TG || (MODE == GRAD_LOSS && !SEG), "per-tree targets: table losses over shared rows");
  constexpr bool DV = MODE == kGradLossDeriv;
  static_assert(!DV || (!SEG && !TG), "derivative objectives: shared rows, their own columns");
  constexpr int S = 2 + G;
  constexpr int TILE = 64 * R;
  using V = typename V16<T>::type;
  constexpr int N = V16<T>::N;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int rows = a.ntiles * TILE;
  const int nx = XG ? 0 : a.nfeat;  // feature arrays staged in LDS
  const int ncol = (TG || DV) ? a.ntgt : 1;  // columns of y (and of w)
  const int narr = nx + ((MODE == GRAD_LOSS || DV) ? ncol * (W ? 2 : 1) : MODE == kGradLossExpr ? (a.w ? 2 : 1) : 0);
  T* sX = reinterpret_cast<T*>(smem);
  T* sY = sX + (size_t)nx * rows;
  T* sW = sY + (size_t)ncol * rows;
  T* sPart = sX + (size_t)narr * rows;

  const int rg = blockIdx.x / a.ntg;
  const int g = blockIdx.x - rg * a.ntg;
  const int64_t row0 = (int64_t)rg * rows;
  int64_t seg0 = 0;  // slot g's tree reads its own segment of X / y / w
  if constexpr (SEG) seg0 = a.seg * (int64_t)(a.items[g] & 0xffffff);
  {
    const int vper = rows / N;
    const int total = narr * vper;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int arr = idx / vper;
      const int v = idx - arr * vper;
      const T* src = arr < nx ? a.X + (size_t)arr * a.n_pad : (arr == nx ? a.y : a.w);
      if constexpr (TG || DV) {  // columns of y, then of w, n_pad rows apart
        if (arr >= nx) src = arr < nx + ncol ? a.y + (size_t)(arr - nx) * a.n_pad : a.w + (size_t)(arr - nx - ncol) * a.n_pad;
      }
      reinterpret_cast<V*>(sX + (size_t)arr * rows)[v] = reinterpret_cast<const V*>(src + seg0 + row0)[v];
    }
    for (int i = threadIdx.x; i < a.tpb * S; i += blockDim.x) sPart[i] = T(0);
    if (threadIdx.x == 0) *reinterpret_cast<uint32_t*>(sPart + a.tpb * S) = 0u;  // item counter (a.dyn)
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int64_t rem = a.n - row0;
  const int nt_valid = (int)min((int64_t)a.ntiles, (rem + TILE - 1) / TILE);
  const int last_valid = (int)(rem - (int64_t)(nt_valid - 1) * TILE);
  const double lp = a.lparam;

  // Waves take the group's (cost-sorted) items round-robin, or (a.dyn, the
  // default) from an LDS counter, so a wave that drew cheap items takes more.
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = (int)(blockDim.x >> 6);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(sPart + a.tpb * S);
  auto claim = [&]() {
    uint32_t v = 0;
    if (lane == 0) v = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane((int)v);
  };
  for (int i = a.dyn ? claim() : wave; i < a.tpb; i = a.dyn ? claim() : i + nwaves) {
    const int s = i * a.ntg + ((i & 1) ? (a.ntg - 1 - g) : g);
    if (s >= a.nitems) continue;
    const int item = __builtin_amdgcn_readfirstlane(a.items[s]);
    const int t = item & 0xffffff;
    const int g0 = (item >> 24) * kGradG;  // groups are kGradG constants; G of them carried
    CIns<T>* p = const_prog(a.prog + __builtin_amdgcn_readfirstlane(a.tree_off[t]));
    const int cbase = __builtin_amdgcn_readfirstlane(a.const_off[t]);
    const int nc = __builtin_amdgcn_readfirstlane(a.const_off[t + 1]) - cbase;
    int col = 0;  // this tree's column of the staged y (and w): wave-uniform, one scalar load per item
    if constexpr (TG) col = __builtin_amdgcn_readfirstlane(a.tgt[t]) * rows;
    int dir[G];  // DV: the feature of each tangent slot, wave-uniform, one scalar load each per item
    if constexpr (DV) {
#pragma unroll
      for (int j = 0; j < G; ++j) dir[j] = __builtin_amdgcn_readfirstlane(a.dir[g0 + j]);
    }
    T acc[S];
#pragma unroll
    for (int k = 0; k < S; ++k) acc[k] = T(0);  // [0] Σ w·ℓ, [1] marker, [2+j] Σ w·ℓ'·∂ŷ/∂c (DV: Σ w·ℓ(∂ŷ/∂x))
    for (int tl = 0; tl < nt_valid; ++tl) {
      Dual<T, R, G> d;
      if constexpr (XG) {
        if constexpr (DV) run_program_grad<T, R, D, G, SET, int64_t, true>(p, a.X + row0 + tl * TILE, a.n_pad, lane, g0, d, acc[1], dir);
        else run_program_grad<T, R, D, G, SET>(p, a.X + seg0 + row0 + tl * TILE, a.n_pad, lane, g0, d, acc[1]);
      } else {
        const T* sXt = sX + tl * TILE;
        if constexpr (DV) run_program_grad<T, R, D, G, SET, int, true>(p, sXt, rows, lane, g0, d, acc[1], dir);
        else run_program_grad<T, R, D, G, SET>(p, sXt, rows, lane, g0, d, acc[1]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) acc[1] = mark(d.v[r], acc[1]);
      if constexpr (MODE == GRAD_OUT) {
        const int64_t off = row0 + tl * TILE;
        if (g0 == 0) store_rows<T, R>(a.out_value + (size_t)t * a.out_stride + off, lane, d.v);
#pragma unroll
        for (int j = 0; j < G; ++j)
          if (g0 + j < nc)
            store_rows<T, R>(a.out_grad + (size_t)(cbase + g0 + j) * a.out_stride + off, lane, d.d[j]);
      } else {
        T yv[R], wv[R];
        lds_rows<T, R>(sY + col + tl * TILE, lane, yv);
        if constexpr (W) lds_rows<T, R>(sW + col + tl * TILE, lane, wv);
        const int valid = (tl < nt_valid - 1) ? TILE : last_valid;
        if constexpr (MODE == kGradLossExpr) {
          if (a.w) lds_rows<T, R>(sW + tl * TILE, lane, wv);
          else SR_UNROLL for (int e = 0; e < R; ++e) wv[e] = T(0);  // (a loss reading w is refused without weights)
          Dual<T, R, 1> ld;
          run_loss_dual<T, R>(const_prog(a.lprog), d.v, yv, wv, ld);
#pragma unroll
          for (int e = 0; e < R; ++e) {
            const bool in = row_of<T, R>(e, lane) < valid;
            acc[0] += in ? ld.v[e] : T(0);
#pragma unroll
            for (int j = 0; j < G; ++j) acc[2 + j] += in ? ld.d[0][e] * d.d[j][e] : T(0);
          }
        } else if constexpr (DV) {
#pragma unroll
          for (int e = 0; e < R; ++e) {
            T l = dev::elem_loss<T>(a.loss, lp, d.v[e], yv[e]);
            if constexpr (W) l = wv[e] * l;
            acc[0] += row_of<T, R>(e, lane) < valid ? l : T(0);
          }
#pragma unroll
          for (int j = 0; j < G; ++j) {
            const int c = 1 + g0 + j;  // the channel's column: wave-uniform
            if (c < ncol) {
              lds_rows<T, R>(sY + c * rows + tl * TILE, lane, yv);
              if constexpr (W) lds_rows<T, R>(sW + c * rows + tl * TILE, lane, wv);
#pragma unroll
              for (int e = 0; e < R; ++e) {
                T l = dev::elem_loss<T>(a.loss, lp, d.d[j][e], yv[e]);
                if constexpr (W) l = wv[e] * l;
                acc[2 + j] += row_of<T, R>(e, lane) < valid ? l : T(0);
              }
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < R; ++e) {
            T l = dev::elem_loss<T>(a.loss, lp, d.v[e], yv[e]);
            T dl = dev::elem_dloss<T>(a.loss, lp, d.v[e], yv[e]);
            if constexpr (W) { l = wv[e] * l; dl = wv[e] * dl; }
            const bool in = row_of<T, R>(e, lane) < valid;
            acc[0] += in ? l : T(0);
#pragma unroll
            for (int j = 0; j < G; ++j) acc[2 + j] += in ? dl * d.d[j][e] : T(0);
          }
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int k = 0; k < S; ++k) acc[k] += __shfl_xor(acc[k], off);
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < S; ++k) sPart[i * S + k] = acc[k];
  }
  __syncthreads();
  T* dst = a.partial + ((size_t)rg * ((size_t)a.ntg * a.tpb) + (size_t)g * a.tpb) * S;
  for (int i = threadIdx.x; i < a.tpb * S; i += blockDim.x) dst[i] = sPart[i];
}

template <typename T, int R, int D, int MODE, bool W, int G, int SET, bool XG = false, bool SEG = false,
          bool TG = false>
hipError_t launch_grad_one(const EvalPlan& plan, const GradArgs<T>& a, hipStream_t stream) {
  // raise the dynamic-LDS ceiling once per kernel instantiation: a function-
  // local static is initialised exactly once even with concurrent callers
  static const hipError_t attr_err = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&grad_kernel<T, R, D, MODE, W, G, SET, XG, SEG, TG>), hipFuncAttributeMaxDynamicSharedMemorySize,
      160 * 1024);
  if (attr_err != hipSuccess) return attr_err;
  const unsigned grid = (unsigned)a.nrg * (unsigned)a.ntg;
  hipLaunchKernelGGL((grad_kernel<T, R, D, MODE, W, G, SET, XG, SEG, TG>), dim3(grid), dim3(plan.threads), plan.lds_bytes,
                     stream, a);
  return hipGetLastError();
}

template <typename T, int R, int D, int G, int SET, bool XG = false, bool SEG = false>
hipError_t launch_grad_rd(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream) {
  if constexpr (SEG) {
    if (mode == GRAD_OUT) return hipErrorInvalidValue;  // row sets: losses only
  } else {
    if (mode == GRAD_OUT) return launch_grad_one<T, R, D, GRAD_OUT, false, G, SET, XG>(plan, a, stream);
  }
  constexpr int LSET = SET == OPSET_EXPR ? OPSET_EXPR : OPSET_FULL;  // (expression losses: no basic-set variant)
  if (a.loss >= SRHIP_EXPR_LOSS_BEGIN) return launch_grad_one<T, R, D, kGradLossExpr, false, G, LSET, XG, SEG>(plan, a, stream);
  if (a.w) return launch_grad_one<T, R, D, GRAD_LOSS, true, G, SET, XG, SEG>(plan, a, stream);
  return launch_grad_one<T, R, D, GRAD_LOSS, false, G, SET, XG, SEG>(plan, a, stream);
}

// gradient variants: rows per lane R (fewer tangents leave room for more
// rows) and stack slots D
inline int grad_R(int dtype, bool deep, int G) {
  if (dtype != SRHIP_F32 || deep) return 1;
  return G <= 2 ? 4 : 2;
}

template <typename T, int G, bool SEG = false>
hipError_t launch_grad_g(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream) {
  constexpr int RS = sizeof(T) == 4 ? (G <= 2 ? 4 : 2) : 1;  // grad_R, shallow
  if (plan.D == 4) {
    if (a.opset == OPSET_BASIC) return launch_grad_rd<T, RS, 4, G, OPSET_BASIC, false, SEG>(plan, a, mode, stream);
    return launch_grad_rd<T, RS, 4, G, OPSET_FULL, false, SEG>(plan, a, mode, stream);
  }
  // deep programs; with expression operators among them, the variant that
  // dispatches their micro-instructions
  if (a.opset == OPSET_EXPR) return launch_grad_rd<T, 1, kMaxSlots, G, OPSET_EXPR, false, SEG>(plan, a, mode, stream);
  return launch_grad_rd<T, 1, kMaxSlots, G, OPSET_FULL, false, SEG>(plan, a, mode, stream);
}

// every variant of one element type; SEG: the per-tree row-set instantiations
template <typename T, bool SEG>
hipError_t launch_grad_all(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream) {
  if (plan.wide) {
    // the wide variants: the deep configuration, a.G = kGradG. Both operator sets: a gradient
    // program's feature index has 16 bits without expression operators, 15 with them
    if (a.opset == OPSET_EXPR) return launch_grad_rd<T, 1, kMaxSlots, kGradG, OPSET_EXPR, true, SEG>(plan, a, mode, stream);
    return launch_grad_rd<T, 1, kMaxSlots, kGradG, OPSET_FULL, true, SEG>(plan, a, mode, stream);
  }
  if (plan.D != 4) return launch_grad_g<T, kGradG, SEG>(plan, a, mode, stream);  // deep programs: one variant
  if (a.G == 1) return launch_grad_g<T, 1, SEG>(plan, a, mode, stream);
  if (a.G == 2) return launch_grad_g<T, 2, SEG>(plan, a, mode, stream);
  return launch_grad_g<T, kGradG, SEG>(plan, a, mode, stream);
}

// ---- a target per tree (grad_targets_f32.hip / grad_targets_f64.hip) ------------
// GRAD_LOSS with a table loss only; weighted or not.
template <typename T, int R, int D, int G, int SET, bool XG = false>
hipError_t launch_grad_targets_rd(const EvalPlan& plan, const GradArgs<T>& a, hipStream_t stream) {
  if (a.w) return launch_grad_one<T, R, D, GRAD_LOSS, true, G, SET, XG, false, true>(plan, a, stream);
  return launch_grad_one<T, R, D, GRAD_LOSS, false, G, SET, XG, false, true>(plan, a, stream);
}

template <typename T, int G>
hipError_t launch_grad_targets_g(const EvalPlan& plan, const GradArgs<T>& a, hipStream_t stream) {
  constexpr int RS = sizeof(T) == 4 ? (G <= 2 ? 4 : 2) : 1;  // grad_R, shallow
  if (plan.D == 4) {
    if (a.opset == OPSET_BASIC) return launch_grad_targets_rd<T, RS, 4, G, OPSET_BASIC>(plan, a, stream);
    return launch_grad_targets_rd<T, RS, 4, G, OPSET_FULL>(plan, a, stream);
  }
  if (a.opset == OPSET_EXPR) return launch_grad_targets_rd<T, 1, kMaxSlots, G, OPSET_EXPR>(plan, a, stream);
  return launch_grad_targets_rd<T, 1, kMaxSlots, G, OPSET_FULL>(plan, a, stream);
}

// the variants of launch_grad_all that a per-tree-targets call reaches
template <typename T>
hipError_t launch_grad_targets_all(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream) {
  if (mode != GRAD_LOSS || a.loss >= SRHIP_EXPR_LOSS_BEGIN || a.seg > 0 || !a.tgt || a.ntgt < 1)
    return hipErrorInvalidValue;
  if (plan.wide) {
    if (a.opset == OPSET_EXPR) return launch_grad_targets_rd<T, 1, kMaxSlots, kGradG, OPSET_EXPR, true>(plan, a, stream);
    return launch_grad_targets_rd<T, 1, kMaxSlots, kGradG, OPSET_FULL, true>(plan, a, stream);
  }
  if (plan.D != 4) return launch_grad_targets_g<T, kGradG>(plan, a, stream);  // deep programs: one variant
  if (a.G == 1) return launch_grad_targets_g<T, 1>(plan, a, stream);
  if (a.G == 2) return launch_grad_targets_g<T, 2>(plan, a, stream);
  return launch_grad_targets_g<T, kGradG>(plan, a, stream);
}

// ---- derivative objectives (grad_deriv_f32.hip / grad_deriv_f64.hip) ---------------
// kGradLossDeriv with a table loss, weighted or not, the full operator set: the shallow
// variants at 1, 2 and kGradG tangents, the deep one, the wide one.
template <typename T, int R, int D, int G, bool XG = false>
hipError_t launch_grad_deriv_rd(const EvalPlan& plan, const GradArgs<T>& a, hipStream_t stream) {
  if (a.w) return launch_grad_one<T, R, D, kGradLossDeriv, true, G, OPSET_FULL, XG>(plan, a, stream);
  return launch_grad_one<T, R, D, kGradLossDeriv, false, G, OPSET_FULL, XG>(plan, a, stream);
}

template <typename T>
hipError_t launch_grad_deriv_all(const EvalPlan& plan, const GradArgs<T>& a, hipStream_t stream) {
  if (a.loss >= SRHIP_MARGIN_LOSS_BEGIN || a.opset == OPSET_EXPR || a.seg > 0 || a.tgt || !a.dir || a.ntgt < 2)
    return hipErrorInvalidValue;
  if (plan.wide) return launch_grad_deriv_rd<T, 1, kMaxSlots, kGradG, true>(plan, a, stream);
  if (plan.D != 4) return launch_grad_deriv_rd<T, 1, kMaxSlots, kGradG>(plan, a, stream);  // deep programs: one variant
  constexpr int R12 = sizeof(T) == 4 ? 4 : 1, R4 = sizeof(T) == 4 ? 2 : 1;  // grad_R, shallow
  if (a.G == 1) return launch_grad_deriv_rd<T, R12, 4, 1>(plan, a, stream);
  if (a.G == 2) return launch_grad_deriv_rd<T, R12, 4, 2>(plan, a, stream);
  return launch_grad_deriv_rd<T, R4, 4, kGradG>(plan, a, stream);
}

// Σ over row groups of a derivative launch's partials in fp64, in grad_finalize_kernel's
// fixed order, into out_sum [ntrees][1 + ndir]: group 0 writes channel 0 and the flag,
// every group the channels of its own directions. Each group evaluated the value, so
// each holds the tree's marker: a failed tree's whole row is NaN.
template <typename T, int G>
__global__ void __launch_bounds__(256) deriv_finalize_kernel(GradArgs<T> a, double* __restrict__ out_sum,
                                                             uint8_t* __restrict__ out_ok) {
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
      double* row = out_sum + (size_t)t * a.ntgt;
      if (g0 == 0) {
        row[0] = ok ? acc[0] : __builtin_nan("");
        out_ok[t] = ok ? 1 : 0;
      }
      for (int j = 0; j < G; ++j)
        if (1 + g0 + j < a.ntgt) row[1 + g0 + j] = ok ? acc[2 + j] : __builtin_nan("");
    }
  }
}

template <typename T>
hipError_t launch_grad_deriv_finalize_all(const GradArgs<T>& a, double* out_sum, uint8_t* out_ok, hipStream_t stream) {
  const int npos = a.ntg * a.tpb;
  const unsigned grid = (unsigned)((npos + 63) / 64);
  if (a.G == 1)
    hipLaunchKernelGGL((deriv_finalize_kernel<T, 1>), dim3(grid), dim3(256), 0, stream, a, out_sum, out_ok);
  else if (a.G == 2)
    hipLaunchKernelGGL((deriv_finalize_kernel<T, 2>), dim3(grid), dim3(256), 0, stream, a, out_sum, out_ok);
  else
    hipLaunchKernelGGL((deriv_finalize_kernel<T, kGradG>), dim3(grid), dim3(256), 0, stream, a, out_sum, out_ok);
  return hipGetLastError();
}

}  // namespace
}  // namespace srhip
