// kernels.h — launch interface of the HIP kernels (kernels.hip) for the
// host runtime (api.cpp). No torch, no HIP types beyond the stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srhip_internal.h"

namespace srhip {

enum EvalMode : int { MODE_LOSS = 0, MODE_OUT = 1 };

// Per-(tree, row-group) partial result: Σ w·ℓ over the group's rows and the
// non-finite marker (0, or NaN when some checked value was non-finite).
template <typename T>
struct alignas(2 * sizeof(T)) Part {
  T sum;
  T chk;
};

template <typename T>
struct EvalArgs {
  const Ins<T>* prog;      // all programs
  const int32_t* tree_off; // [ntrees] program start per tree
  const int32_t* list;     // tree ids handled by this launch, cost-descending
  const int32_t* list_off; // [nlist] program start of list[s] (= tree_off[list[s]])
  uint32_t* fail;          // [nlist] MODE_LOSS: set once slot s is known to fail (early exit)
  const uint4* ti_rec;     // [nlist][64] threaded-interpreter records (nullptr: C++ dispatch)
  int nlist;
  const T* X;              // [nfeat][n_pad] feature-major, rows padded
  const T* y;              // [n_pad]
  const T* w;              // [n_pad] or nullptr
  int64_t n;               // valid rows
  int64_t n_pad;
  int nfeat;
  int ntiles;              // row tiles per workgroup
  int ntg;                 // tree groups
  int tpb;                 // trees per group
  int nrg;                 // row groups
  int loss;
  int rotate;              // MODE_LOSS: start each wave's tree sequence at row-group-dependent offsets
  int contig;              // tree group g holds list slots [g*tpb, (g+1)*tpb) (tree code: a group's
                           // code is one contiguous range); 0: slots dealt in snake order
  double lparam;           // the loss parameter (LossFunctions' Float64 field, not rounded to T)
  Part<T>* partial;        // [nrg][ntg*tpb]
  T* out;                  // MODE_OUT: [ntrees][out_stride]
  int64_t out_stride;
  // per-tree row sets (srhip_eval_loss_rowsets; interpreter, one tree per
  // group): tree t reads rows [t·seg, t·seg + n) of X / y / w; 0 = shared rows
  int64_t seg = 0;
  // finalize only: the launch wrote 4-byte partials (Σ; float at partial + rg·npos + pos) and a
  // failed tree is the one whose slot failure flag is set (the hand-written loss tree loops)
  int part4 = 0;
  // the loss program of an expression loss (loss >= SRHIP_EXPR_LOSS_BEGIN), device memory
  const Ins<T>* lprog = nullptr;
  // per-tree targets (srhip_eval_loss_targets; the kModeLossTargets variants of
  // eval_targets_*.hip): tree id t is scored against column tgt[t] of y / w, which
  // are then [ntgt][n_pad] (target-major); nullptr / 0: one y, one w
  const int32_t* tgt = nullptr;
  int ntgt = 0;
};

// Geometry of one evaluation launch, chosen by plan_eval().
struct EvalPlan {
  int R;          // rows per lane per instruction
  int D;          // stack slots of the kernel variant (kShallowSlots or kMaxSlots)
  int opset;      // OpSet the kernel variant is compiled for
  int tile;       // rows per tile = 64 * R
  int ntiles;
  int rows_wg;    // rows per workgroup
  int nrg, ntg, tpb;
  size_t lds_bytes;
  int threads;    // workgroup size
  // tree code only: row groups [0, nbig) of ntiles tiles, then row groups of
  // ts tiles (the last round of workgroups in smaller pieces); nbig < 0: all full
  int nbig = -1, ts = 0;
  // loss tree code only (tail_map.h): each tree group of the row groups
  // [tbig, nrg) is run by tsub workgroups, launched after all the others;
  // tsub = 1: every tree group is one workgroup
  int tbig = -1, tsub = 1;
  // the wide kernel variant (eval_kernel.h / grad_kernels.hip XG): X is read from
  // global memory, LDS holds y, w and the partial slots only
  bool wide = false;
};

// Choose the geometry for `nlist` trees over `n` rows; returns false when the
// row tile of this feature count does not fit in LDS (the caller then plans
// the wide variant, plan_eval_wide).
// Threaded-interpreter instruction records of every list slot (f32 shallow
// programs; eval_kernel.h / gen_asm_interp.py): [nlist][64] uint4.
bool ti_compiled();  // eval kernels built with the threaded interpreter (SR_TI)
hipError_t launch_ti_records(const Ins<float>* prog, const int32_t* list_off, int nlist,
                             uint32_t rs_bytes, uint4* rec, hipStream_t stream);

// ntgt > 0 (a per-tree-targets launch): the tile holds ntgt columns of y (and of w).
bool plan_eval(int dtype, bool deep, int opset, int mode, bool weighted, int nfeat,
               int64_t n, int nlist, EvalPlan* plan, int ntgt = 0);
// The wide plan of the same launch: the deep configuration with no feature
// array in LDS. False only when y, w and the partial slots do not fit.
bool plan_eval_wide(int dtype, int mode, bool weighted, int64_t n, int nlist, EvalPlan* plan, int ntgt = 0);
// Same, for explicit R / D / LDS arrays / partial bytes per tree slot.
// target_wg: workgroups the tree groups aim at; min_per_group: trees a group
// keeps at least (the loss tree code: 16384 / 64, measured on config #2)
bool plan_geometry(size_t esz, int R, int D, int narr, size_t part_bytes, int64_t n,
                   int nlist, EvalPlan* plan, size_t tile_budget = 40 * 1024, size_t two_tile_cap = 0,
                   int target_wg = 8192, int min_per_group = 4);

// ---- constant gradients (grad_kernels.hip) -----------------------------------
constexpr int kGradG = 4;  // tangents per pass (constants per "tangent group")
enum GradMode : int { GRAD_LOSS = 0, GRAD_OUT = 1 };

template <typename T>
struct GradArgs {
  const Ins<T>* prog;       // programs compiled for gradients (no folding)
  const int32_t* tree_off;
  const int32_t* items;     // work items: tree | (tangent group << 24)
  int nitems;
  const int32_t* const_off; // [ntrees+1]
  const T* X;
  const T* y;
  const T* w;
  int64_t n, n_pad;
  int nfeat;
  int ntiles, ntg, tpb, nrg;
  int loss;
  double lparam;
  int G;                    // tangents carried by this launch (1, 2 or kGradG)
  int opset;                // OPSET_BASIC: the programs use only the basic operators
  T* partial;               // [nrg][ntg*tpb][2 + G]
  T* out_value;             // GRAD_OUT: [ntrees][out_stride]
  T* out_grad;              // GRAD_OUT: [total consts][out_stride]
  int64_t out_stride;
  int dyn = 0;              // waves take their items from an LDS counter (SRHIP_INTERP_DYN)
  const Ins<T>* lprog = nullptr;  // the loss program of an expression loss (loss >= SRHIP_EXPR_LOSS_BEGIN)
  // per-tree row sets (srhip_eval_loss_grad_rowsets; GRAD_LOSS, one item per workgroup: tpb = 1,
  // ntg = nitems): tree t reads rows [t·seg, t·seg + n) of X / y / w; 0 = shared rows
  int64_t seg = 0;
  // per-tree targets (srhip_eval_loss_grad_targets; the TG variants of
  // grad_targets_*.hip): tree id t is scored against column tgt[t] of y / w, which
  // are then [ntgt][n_pad] (target-major); nullptr / 0: one y, one w
  const int32_t* tgt = nullptr;
  int ntgt = 0;
  // derivative objectives (srhip_eval_loss_deriv; the kGradLossDeriv variants of
  // grad_deriv_*.hip): the feature of each tangent, [groups · kGradG] with a negative
  // sentinel past the last direction; y / w are then ntgt = 1 + ndir columns
  // (y, then one per direction) and tgt is null
  const int32_t* dir = nullptr;
};

// ntgt > 0 (a per-tree-targets launch): the tile holds ntgt columns of y (and of w).
bool plan_grad(int dtype, bool deep, int G, int mode, bool weighted, int nfeat, int64_t n,
               int nitems, EvalPlan* plan, int ntgt = 0);
// The wide plan: the deep configuration, kGradG tangents, no feature array in LDS.
bool plan_grad_wide(int dtype, int mode, bool weighted, int64_t n, int nitems, EvalPlan* plan, int ntgt = 0);
template <typename T>
hipError_t launch_grad(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream);
// the per-tree row-set variants (a.seg > 0, GRAD_LOSS; launch_grad forwards to them)
template <typename T>
hipError_t launch_grad_seg(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream);
// the per-tree-targets variants (a.tgt set, GRAD_LOSS, shared rows; launch_grad forwards to them)
template <typename T>
hipError_t launch_grad_targets(const EvalPlan& plan, const GradArgs<T>& a, int mode, hipStream_t stream);
// the derivative-objective variants (a.dir set; grad_deriv_f32.hip / grad_deriv_f64.hip) and
// their finalisation into out_sum [ntrees][a.ntgt], out_ok [ntrees]
template <typename T>
hipError_t launch_grad_deriv(const EvalPlan& plan, const GradArgs<T>& a, hipStream_t stream);
template <typename T>
hipError_t launch_grad_deriv_finalize(const GradArgs<T>& a, double* out_sum, uint8_t* out_ok, hipStream_t stream);
template <typename T>
hipError_t launch_grad_finalize(const GradArgs<T>& a, double* out_sum, uint8_t* out_ok,
                                double* out_dloss, hipStream_t stream);

// ---- constant gradients of a derivative objective (grad_deriv2_f32.hip / _f64.hip) ----
// Second-order forward mode (grad2_interp.h). A work item is two words:
//   items[2s]     tree (24 bits) | constant group << 24
//   items[2s + 1] direction index k (0 .. ndir-1)
// so a call holds up to 2^24 trees, 256 constant groups per tree (256·GC constants:
// more than the 254 a gradient program can index) and any int32 count of directions.
// DERIV2_LOSS partial per item, 3 + 2·GC values:
//   [0] Σ w₀·ℓ(ŷ, y) (items of k = 0)   [1] marker of the value evaluation
//   [2] Σ w_{1+k}·ℓ(dx, Y[1+k])          [3 + j] Σ w_{1+k}·ℓ'(dx, Y[1+k])·dxc[j]
//   [3 + GC + j] Σ w₀·ℓ'(ŷ, y)·dc[j] (items of k = 0)
// DERIV2_OUT writes dx and dxc per row.
enum Deriv2Mode : int { DERIV2_LOSS = 0, DERIV2_OUT = 1 };

template <typename T>
struct Deriv2Args {
  const Ins<T>* prog;       // gradient programs (no folding)
  const int32_t* tree_off;
  const int32_t* items;     // [nitems][2]
  int nitems;
  const int32_t* const_off; // [ntrees+1]
  const int32_t* dir;       // [ndir] feature of each direction
  int ndir;
  const T* X;
  const T* y;               // [1 + ndir][n_pad]
  const T* w;               // [1 + ndir][n_pad] or nullptr
  int64_t n, n_pad;
  int nfeat;
  int ntiles, ntg, tpb, nrg;
  int loss;
  double lparam;
  int GC;                   // constant tangents carried by this launch (1 or 2)
  T* partial;               // [nrg][ntg*tpb][3 + 2·GC]
  T* out_deriv;             // DERIV2_OUT: [ntrees][ndir][out_stride]
  T* out_mixed;             // DERIV2_OUT: [total consts][ndir][out_stride]
  int64_t out_stride;
  int dyn = 0;
};

// GC and R of the variant that runs (dtype, deep, ndir): R is the one
// srhip_eval_loss_deriv's variant has for the same call, so both reduce a row
// group's rows in the same order.
void deriv2_variant(int dtype, bool deep, int ndir, int* R, int* GC);
// false: the row tile of every feature and column does not fit in LDS (no wide variant)
bool plan_grad_deriv2(int dtype, bool deep, int ndir, int mode, bool weighted, int nfeat, int64_t n, int nitems,
                      EvalPlan* plan);
template <typename T>
hipError_t launch_grad_deriv2(const EvalPlan& plan, const Deriv2Args<T>& a, int mode, hipStream_t stream);
// out_loss [ntrees][1 + ndir], out_grad [total consts][1 + ndir], out_ok [ntrees]
template <typename T>
hipError_t launch_grad_deriv2_finalize(const Deriv2Args<T>& a, double* out_loss, double* out_grad, uint8_t* out_ok,
                                       hipStream_t stream);

// Σ over row groups of the gradient tree code's per-constant partials:
// out[cidx[k]] = Σ_rg gpart[rg][cidx[k]] in fp64 (jit_grad.cpp).
// zero a[0..na) and b[0..nb) (uint32 words) in one launch
hipError_t launch_zero_words(uint32_t* a, int64_t na, uint32_t* b, int64_t nb, hipStream_t stream);
// [Σ w·ℓ, failed] per tree + Σ w into device memory (srhip_eval_loss_packed)
hipError_t launch_pack_partials(const double* sum, const uint8_t* ok, const uint8_t* verdict, int nt, int64_t rows,
                                double wsum, double* out, hipStream_t stream);
// the gradient's partials: [Σ w·ℓ, failed] per tree, Σ w·∂ℓ/∂c per constant, Σ w
// (2·nt + nconst + 1 doubles; have: sum / ok / dloss hold this call's results)
hipError_t launch_pack_grad_partials(const double* sum, const uint8_t* ok, const double* dloss,
                                     const uint8_t* static_fail, const int32_t* const_off, int nt, int nconst,
                                     bool have, double wsum, double* out, hipStream_t stream);
// device groups: ndev packed partials (stride doubles apart) added in member
// order and finished (NaN / ok = 0 for a tree that failed on any shard);
// out_dloss null: the loss layout (nconst = 0)
hipError_t launch_combine_partials(const double* slots, size_t stride, int ndev, int nt, int nconst,
                                   const int32_t* const_off, double* out_sum, uint8_t* out_ok, double* out_dloss,
                                   double* out_wsum, hipStream_t stream);
hipError_t launch_gconst_finalize(const float* gpart, int nrg, int nconst, const int32_t* cidx, int ncidx,
                                  double* out, hipStream_t stream);
// the same over Float64 partials (jit64.cpp's gradient tree code)
hipError_t launch_gconst_finalize(const double* gpart, int nrg, int nconst, const int32_t* cidx, int ncidx,
                                  double* out, hipStream_t stream);

template <typename T>
hipError_t launch_eval(const EvalPlan& plan, const EvalArgs<T>& a, int mode,
                       hipStream_t stream);
// the wide variants (plan.wide; launch_eval forwards to them)
template <typename T>
hipError_t launch_eval_wide(const EvalPlan& plan, const EvalArgs<T>& a, int mode, hipStream_t stream);
// the per-tree-targets variants (a.tgt set, MODE_LOSS; eval_targets_*.hip): LDS or wide by plan.wide
template <typename T>
hipError_t launch_eval_targets(const EvalPlan& plan, const EvalArgs<T>& a, hipStream_t stream);

// Σ over row groups of the partials → per-tree fp64 sum and ok flag; clears
// the failure flags it read (a.fail) and, given cnt, copies the two tree-code
// counters to cnt_host and clears them.
template <typename T>
hipError_t launch_finalize(const EvalArgs<T>& a, double* out_sum,
                           uint8_t* out_ok, hipStream_t stream, uint32_t* cnt = nullptr,
                           uint32_t* cnt_host = nullptr);

// Dataset packing: src rows [0, rows) in Julia (nfeat, n) column-major layout
// (layout 0) or feature-major with row stride src_stride (layout 1) →
// dst [nfeat][n_pad], padding rows replicate the last row. Sets *bad if a
// non-finite value is seen.
template <typename T>
hipError_t launch_pack_x(const T* src, int layout, int64_t src_stride,
                         int64_t rows, int nfeat, int64_t n_pad, T* dst,
                         int* bad, hipStream_t stream);
template <typename T>
hipError_t launch_pack_vec(const T* src, int64_t rows, int64_t n_pad, T* dst,
                           hipStream_t stream);
// Shared-subtree columns (jit.h Columns): every row of column g = list[k],
// k < ncol, of cols ([.][n_pad]) set to NaN when ok[g] == 0 (device memory).
hipError_t launch_poison_columns(const uint8_t* ok, const int32_t* list, int ncol, float* cols, int64_t n_pad,
                                 hipStream_t stream);
// Row gather for score_func_batch: dst[f][k] = src[f][idx[k]] (+ y, w);
// seg > 0: one sample of nidx rows per segment of seg rows (per-tree samples,
// srhip_eval_loss_rowsets), idx = [dst_pad / seg][nidx].
template <typename T>
hipError_t launch_gather_rows(const T* X, const T* y, const T* w, int nfeat,
                              int64_t src_pad, const int64_t* idx, int64_t nidx, int64_t seg,
                              int64_t dst_pad, T* Xd, T* yd, T* wd,
                              hipStream_t stream);
// The per-tree samples of a multi-target dataset (srhip_eval_loss_rowsets_targets):
// Y / W are [ntargets][src_pad]; segment t takes its y (and w) rows from column
// tgt[t]. seg > 0, idx = [dst_pad / seg][nidx], tgt = [dst_pad / seg].
template <typename T>
hipError_t launch_gather_rows_targets(const T* X, const T* Y, const T* W, const int32_t* tgt, int nfeat,
                                      int64_t src_pad, const int64_t* idx, int64_t nidx, int64_t seg,
                                      int64_t dst_pad, T* Xd, T* yd, T* wd, hipStream_t stream);

}  // namespace srhip
