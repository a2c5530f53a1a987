// grad_deriv2.h — constant gradients of a derivative objective: the kernel of
// srhip_eval_loss_grad_deriv and srhip_eval_mixed_tree_array (second-order forward
// mode, grad2_interp.h), its launch dispatch and its finalisation. Included by
// grad_deriv2_f32.hip / grad_deriv2_f64.hip only: grad_kernel.h and its
// instantiations are untouched.
//
// Same workgroup structure as grad_kernel (row group staged in LDS, waves take work
// items from an LDS counter or round-robin). A work item is (tree, direction k,
// group of GC constants); the layout of items and partials is in kernels.h
// (Deriv2Args). The row tile stages every column of Y and W, as kGradLossDeriv does.
//
// The flag rule is that of the derivative objectives: only the
// value evaluation is marked, so ok is did_succeed; a non-finite derivative or
// mixed partial gives non-finite sums with ok = 1; a failed tree's rows are NaN.
#pragma once
#include <hip/hip_runtime.h>

#include "grad2_interp.h"
#include "kernels.h"

namespace srhip {
namespace {

using namespace interp;

template <typename T, int R, int D, int MODE, bool W, int GC>
__global__ void __launch_bounds__(256) grad_deriv2_kernel(Deriv2Args<T> a) {
  constexpr int S = 3 + 2 * GC;
  constexpr int TILE = 64 * R;
  using V = typename V16<T>::type;
  constexpr int N = V16<T>::N;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int rows = a.ntiles * TILE;
  const int nx = a.nfeat;
  const int ncol = 1 + a.ndir;  // columns of y (and of w)
  const int narr = nx + (MODE == DERIV2_LOSS ? ncol * (W ? 2 : 1) : 0);
  T* sX = reinterpret_cast<T*>(smem);
  T* sY = sX + (size_t)nx * rows;
  T* sW = sY + (size_t)ncol * rows;
  T* sPart = sX + (size_t)narr * rows;

  const int rg = blockIdx.x / a.ntg;
  const int g = blockIdx.x - rg * a.ntg;
  const int64_t row0 = (int64_t)rg * rows;
  {
    const int vper = rows / N;
    const int total = narr * vper;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int arr = idx / vper;
      const int v = idx - arr * vper;
      const T* src = arr < nx ? a.X + (size_t)arr * a.n_pad
                   : arr < nx + ncol ? a.y + (size_t)(arr - nx) * a.n_pad
                                     : a.w + (size_t)(arr - nx - ncol) * a.n_pad;
      reinterpret_cast<V*>(sX + (size_t)arr * rows)[v] = reinterpret_cast<const V*>(src + row0)[v];
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
    const int item = __builtin_amdgcn_readfirstlane(a.items[2 * s]);
    const int k = __builtin_amdgcn_readfirstlane(a.items[2 * s + 1]);  // the direction: wave-uniform
    const int t = item & 0xffffff;
    const int g0 = ((item >> 24) & 0xff) * GC;
    const int fd = __builtin_amdgcn_readfirstlane(a.dir[k]);
    CIns<T>* p = const_prog(a.prog + __builtin_amdgcn_readfirstlane(a.tree_off[t]));
    const int cbase = __builtin_amdgcn_readfirstlane(a.const_off[t]);
    const int nc = __builtin_amdgcn_readfirstlane(a.const_off[t + 1]) - cbase;
    T acc[S];
#pragma unroll
    for (int q = 0; q < S; ++q) acc[q] = T(0);
    for (int tl = 0; tl < nt_valid; ++tl) {
      Dual2<T, R, GC> d;
      run_program_grad2<T, R, D, GC>(p, sX + tl * TILE, rows, lane, g0, fd, d, acc[1]);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[1] = mark(d.v[r], acc[1]);
      if constexpr (MODE == DERIV2_OUT) {
        const int64_t off = row0 + tl * TILE;
        if (g0 == 0) store_rows<T, R>(a.out_deriv + ((size_t)t * a.ndir + k) * a.out_stride + off, lane, d.dx);
#pragma unroll
        for (int j = 0; j < GC; ++j)
          if (g0 + j < nc)
            store_rows<T, R>(a.out_mixed + ((size_t)(cbase + g0 + j) * a.ndir + k) * a.out_stride + off, lane,
                             d.dxc[j]);
      } else {
        const int valid = (tl < nt_valid - 1) ? TILE : last_valid;
        T yv[R], wv[R];
        // the direction's channel: dx stands in the prediction's place
        lds_rows<T, R>(sY + (1 + k) * rows + tl * TILE, lane, yv);
        if constexpr (W) lds_rows<T, R>(sW + (1 + k) * rows + tl * TILE, lane, wv);
#pragma unroll
        for (int e = 0; e < R; ++e) {
          T l = dev::elem_loss<T>(a.loss, lp, d.dx[e], yv[e]);
          T dl = dev::elem_dloss<T>(a.loss, lp, d.dx[e], yv[e]);
          if constexpr (W) { l = wv[e] * l; dl = wv[e] * dl; }
          const bool in = row_of<T, R>(e, lane) < valid;
          acc[2] += in ? l : T(0);
#pragma unroll
          for (int j = 0; j < GC; ++j) acc[3 + j] += in ? dl * d.dxc[j][e] : T(0);
        }
        if (k == 0) {  // channel 0, once per (tree, constant group)
          lds_rows<T, R>(sY + tl * TILE, lane, yv);
          if constexpr (W) lds_rows<T, R>(sW + tl * TILE, lane, wv);
#pragma unroll
          for (int e = 0; e < R; ++e) {
            T l = dev::elem_loss<T>(a.loss, lp, d.v[e], yv[e]);
            T dl = dev::elem_dloss<T>(a.loss, lp, d.v[e], yv[e]);
            if constexpr (W) { l = wv[e] * l; dl = wv[e] * dl; }
            const bool in = row_of<T, R>(e, lane) < valid;
            acc[0] += in ? l : T(0);
#pragma unroll
            for (int j = 0; j < GC; ++j) acc[3 + GC + j] += in ? dl * d.dc[j][e] : T(0);
          }
        }
      }
    }
    if constexpr (MODE == DERIV2_LOSS) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < S; ++q) acc[q] += __shfl_xor(acc[q], off);
      if (lane == 0)
#pragma unroll
        for (int q = 0; q < S; ++q) sPart[i * S + q] = acc[q];
    }
  }
  if constexpr (MODE == DERIV2_LOSS) {
    __syncthreads();
    T* dst = a.partial + ((size_t)rg * ((size_t)a.ntg * a.tpb) + (size_t)g * a.tpb) * S;
    for (int i = threadIdx.x; i < a.tpb * S; i += blockDim.x) dst[i] = sPart[i];
  }
}

template <typename T, int R, int D, int MODE, bool W, int GC>
hipError_t launch_deriv2_one(const EvalPlan& plan, const Deriv2Args<T>& a, hipStream_t stream) {
  static const hipError_t attr_err =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&grad_deriv2_kernel<T, R, D, MODE, W, GC>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr_err != hipSuccess) return attr_err;
  const unsigned grid = (unsigned)a.nrg * (unsigned)a.ntg;
  hipLaunchKernelGGL((grad_deriv2_kernel<T, R, D, MODE, W, GC>), dim3(grid), dim3(plan.threads), plan.lds_bytes, stream,
                     a);
  return hipGetLastError();
}

template <typename T, int R, int D, int GC>
hipError_t launch_deriv2_rd(const EvalPlan& plan, const Deriv2Args<T>& a, int mode, hipStream_t stream) {
  if (plan.R != R || plan.D != D || a.GC != GC || plan.wide) return hipErrorInvalidValue;
  if (mode == DERIV2_OUT) return launch_deriv2_one<T, R, D, DERIV2_OUT, false, GC>(plan, a, stream);
  if (a.w) return launch_deriv2_one<T, R, D, DERIV2_LOSS, true, GC>(plan, a, stream);
  return launch_deriv2_one<T, R, D, DERIV2_LOSS, false, GC>(plan, a, stream);
}

// Σ over row groups of the partials in fp64, in grad_finalize_kernel's fixed order.
// The item of constant group 0 writes its direction's loss sum (and, for k = 0, channel
// 0's and the flag); every item the gradient sums of its own constants: column 1 + k,
// and column 0 from the items of k = 0. Each item evaluated the value, so each holds
// the tree's marker.
template <typename T, int GC>
__global__ void __launch_bounds__(256) deriv2_finalize_kernel(Deriv2Args<T> a, double* __restrict__ out_loss,
                                                              double* __restrict__ out_grad,
                                                              uint8_t* __restrict__ out_ok) {
  constexpr int S = 3 + 2 * GC;
  __shared__ double sh[4][S][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int npos = a.ntg * a.tpb;
  const int pos = blockIdx.x * 64 + lane;
  double acc[S];
  for (int q = 0; q < S; ++q) acc[q] = 0.0;
  if (pos < npos) {
    for (int rg = w; rg < a.nrg; rg += 4) {
      const T* q = a.partial + ((size_t)rg * npos + pos) * S;
      for (int e = 0; e < S; ++e) acc[e] += (double)q[e];
    }
  }
  for (int q = 0; q < S; ++q) sh[w][q][lane] = acc[q];
  __syncthreads();
  if (w == 0 && pos < npos) {
    for (int q = 0; q < S; ++q) acc[q] = (sh[0][q][lane] + sh[1][q][lane]) + (sh[2][q][lane] + sh[3][q][lane]);
    const int g = pos / a.tpb;
    const int i = pos - g * a.tpb;
    const int sidx = i * a.ntg + ((i & 1) ? (a.ntg - 1 - g) : g);
    if (sidx < a.nitems) {
      const int item = a.items[2 * sidx];
      const int k = a.items[2 * sidx + 1];
      const int t = item & 0xffffff;
      const int g0 = ((item >> 24) & 0xff) * GC;
      const int ncol = 1 + a.ndir;
      const bool ok = !__builtin_isnan(acc[1]);
      const double nan = __builtin_nan("");
      if (g0 == 0) {
        out_loss[(size_t)t * ncol + 1 + k] = ok ? acc[2] : nan;
        if (k == 0) {
          out_loss[(size_t)t * ncol] = ok ? acc[0] : nan;
          out_ok[t] = ok ? 1 : 0;
        }
      }
      const int cb = a.const_off[t];
      const int nc = a.const_off[t + 1] - cb;
      for (int j = 0; j < GC; ++j)
        if (g0 + j < nc) {
          double* row = out_grad + (size_t)(cb + g0 + j) * ncol;
          row[1 + k] = ok ? acc[3 + j] : nan;
          if (k == 0) row[0] = ok ? acc[3 + GC + j] : nan;
        }
    }
  }
}

// R and GC per variant (kernels.hip deriv2_variant): no instantiation spills a VGPR
// (DESIGN.md §3.19's resource table)
template <typename T>
hipError_t launch_grad_deriv2_all(const EvalPlan& plan, const Deriv2Args<T>& a, int mode, hipStream_t stream) {
  if (a.ndir < 1 || !a.dir) return hipErrorInvalidValue;
  if constexpr (sizeof(T) == 4) {
    if (plan.D != 4) return launch_deriv2_rd<T, 1, kMaxSlots, 2>(plan, a, mode, stream);
    if (plan.R == 4) return launch_deriv2_rd<T, 4, 4, 2>(plan, a, mode, stream);
    return launch_deriv2_rd<T, 2, 4, 2>(plan, a, mode, stream);
  } else {
    if (plan.D != 4) return launch_deriv2_rd<T, 1, kMaxSlots, 1>(plan, a, mode, stream);
    return launch_deriv2_rd<T, 1, 4, 2>(plan, a, mode, stream);
  }
}

template <typename T>
hipError_t launch_grad_deriv2_finalize_all(const Deriv2Args<T>& a, double* out_loss, double* out_grad, uint8_t* out_ok,
                                           hipStream_t stream) {
  const int npos = a.ntg * a.tpb;
  const unsigned grid = (unsigned)((npos + 63) / 64);
  if (a.GC == 1)
    hipLaunchKernelGGL((deriv2_finalize_kernel<T, 1>), dim3(grid), dim3(256), 0, stream, a, out_loss, out_grad, out_ok);
  else
    hipLaunchKernelGGL((deriv2_finalize_kernel<T, 2>), dim3(grid), dim3(256), 0, stream, a, out_loss, out_grad, out_ok);
  return hipGetLastError();
}

}  // namespace
}  // namespace srhip
