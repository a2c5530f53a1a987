// api.cpp — the C ABI of libsrhip.so (include/srhip.h).
//
// Host runtime: contexts (device + stream + workspace, one mutex), device
// datasets (uploaded once, feature-major, rows padded), compiled programs
// (device resident), evaluation planning and launches, results back to the
// caller's buffers. No C++ exception crosses the boundary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits>
#include <condition_variable>
#include <functional>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <type_traits>
#include <numeric>
#include <thread>
#include <string>
#include <vector>

#include "../../include/srhip.h"
#include "compile.h"
#include "host_ops.h"
#include "constopt.h"
#include "env.h"
#include "jit.h"
#include "kernels.h"

namespace srhip {
namespace {
thread_local const char* t_last_kernel = "";
}
void note_kernel(const char* name) { t_last_kernel = name ? name : ""; }
const char* last_kernel() { return t_last_kernel; }
static thread_local int t_loss_launch[6] = {0, 0, 0, 0, 0, 0};
void note_loss_launch(int nrg, int ntg, int tpb, unsigned grid, int tbig, int tsub) {
  const int v[6] = {nrg, ntg, tpb, (int)grid, tbig, tsub};
  std::copy(v, v + 6, t_loss_launch);
}
const int* last_loss_launch() { return t_loss_launch; }
int& host_thread_cap() {
  thread_local int cap = 0;
  return cap;
}
}  // namespace srhip

using namespace srhip;

namespace {

thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIP_CHECK(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess)                                                            \
      throw Error(SRHIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const Error& e) {
    return set_error(e.code, e.what());
  } catch (const std::bad_alloc&) {
    return set_error(SRHIP_ERR_NOMEM, "host allocation failed");
  } catch (const std::exception& e) {
    return set_error(SRHIP_ERR_INVALID, e.what());
  } catch (...) {
    return set_error(SRHIP_ERR_INVALID, "unknown error");
  }
}

// grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void ensure(size_t n) {
    if (n <= bytes) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) throw Error(SRHIP_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    bytes = n;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// scoped device buffer: freed when it goes out of scope (hipFree waits for
// the device, so an in-flight copy never reads freed memory)
struct ScopedBuf : DevBuf {
  ScopedBuf() = default;
  ScopedBuf(const ScopedBuf&) = delete;
  ScopedBuf& operator=(const ScopedBuf&) = delete;
  ~ScopedBuf() { release(); }
};

constexpr int64_t kRowPad = 8192;  // dataset rows are padded to a multiple of this

int64_t pad_rows(int64_t rows) { return ((std::max<int64_t>(rows, 1) + kRowPad - 1) / kRowPad) * kRowPad; }

size_t dtype_size(int dtype) { return dtype == SRHIP_F32 ? 4 : 8; }

// f(T()) with T the element type of dtype (checked by the caller): float or double
template <typename F>
auto by_dtype(int dtype, F&& f) -> decltype(f(float())) {
  return dtype == SRHIP_F32 ? f(float()) : f(double());
}

// Persistent host-copy workers of one context (copy_rows_to_host): created
// at the first large per-row output, joined when the context closes. A job is
// one function run by every worker with its index; the caller keeps issuing
// the DMA chunks meanwhile and waits for the job at the end.
class CopyPool {
 public:
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  unsigned size() const { return (unsigned)th_.size(); }
  void start(unsigned n, int device) {
    if (!th_.empty()) return;
    for (unsigned j = 0; j < n; ++j)
      th_.emplace_back([this, j, device] {
        const bool dev_ok = hipSetDevice(device) == hipSuccess;
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
          cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
          if (stop_) return;
          seen = gen_;
          std::function<void(unsigned, bool)> f = job_;
          lk.unlock();
          f(j, dev_ok);
          lk.lock();
          if (--busy_ == 0) cv_done_.notify_all();
        }
      });
  }
  void submit(std::function<void(unsigned, bool)> f) {
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = std::move(f);
      busy_ = (unsigned)th_.size();
      ++gen_;
    }
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return busy_ == 0; });
  }

 private:
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, cv_done_;
  std::function<void(unsigned, bool)> job_;
  uint64_t gen_ = 0;
  unsigned busy_ = 0;
  bool stop_ = false;
};

}  // namespace

struct srhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // kernel timing of the current call: event pairs recorded around each launch
  // and read after the call's one stream synchronisation (timing_finish)
  std::vector<hipEvent_t> tev;
  int tpairs = 0;
  bool timing_pending = false;
  bool cnt_pending = false;    // tree-code bail / PRECISE-redo counters copied to pin_cnt
  // pinned host copies of the per-tree results 
  double* pin_sum = nullptr;
  uint8_t* pin_ok = nullptr;
  size_t pin_cap = 0;
  // where the finalize of the current evaluation writes the per-tree results:
  // the pinned host buffers themselves (zero copy) or sums / oks on the device
  double* res_sum = nullptr;
  uint8_t* res_ok = nullptr;
  bool res_host = false;
  bool want_device_results = false;  // srhip_eval_loss_packed: per-tree results stay in device buffers
  uint32_t* pin_cnt = nullptr;  // [2]
  // pinned staging of large per-row outputs (srhip_eval_tree_array): two
  // halves, DMA into one while the other is copied to the caller's memory
  unsigned char* pin_stage = nullptr;
  size_t stage_cap = 0;
  std::vector<hipEvent_t> stage_evs;  // one per chunk of a staged copy
  std::unique_ptr<CopyPool> copy_pool;  // its host-copy workers (persistent)
  double last_ms = 0.0;
  int last_launches = 0;
  int last_bailed = 0;  // trees re-evaluated after their tree code handed a tile back
  int last_jit_trees = 0;  // trees the last evaluation ran as tree code
  int64_t last_redone = 0;  // tiles tree code redid with the PRECISE routines
  DevBuf partial, sums, oks, dloss, scratch_idx, gather, derived;
  DevBuf gderived;  // [gspan][n_pad] shared-subtree columns of a call that cannot use a dataset's pool (jit.h Columns)
  DevBuf gpartial, gsum, gok, gti;  // their derive pass's partials, per-column results, threaded records
  // the stable column numbers of this context's shared subtrees (slots.h; SRHIP_COLUMN_SLOTS,
  // default 64), the datasets holding a column pool under them, and what the derive passes did:
  // columns derived, columns a call found in a pool, derive programs built
  SlotRegistry slots{std::max(0, env_int("SRHIP_COLUMN_SLOTS", 64))};
  std::vector<srhip_dataset*> pooled;
  int64_t cols_derived = 0, cols_reused = 0, derive_programs = 0;
  DevBuf tgt;  // [ntrees] the target of each tree (srhip_eval_loss_targets, _rowsets_targets)
  DevBuf fail;  // [list slots] early-exit flags of the eval kernel (MODE_LOSS)
  bool fail_clean = false;  // all of `fail` is zero: the finalize kernels clear the flags they read
  DevBuf ti_rec;  // threaded-interpreter records of the shallow f32 list
  DevBuf bail_list, bail_fail;  // trees whose tree code handed a tile back, and their flags
  DevBuf gpart;  // [nrg][nconst] per-row-group ∂L/∂c of the gradient tree code
  std::vector<double> h_sum;
  std::vector<uint8_t> h_ok;
  // device copies of the expression-loss programs this context has run, by
  // (handle, dtype): uploaded at first use, freed when the context closes
  // (handles are never reused, so an entry cannot go stale)
  struct LossProg { int kind, dtype; void* d; };
  std::vector<LossProg> lprogs;
};

// Device memory of a multi-target dataset (srhip_dataset_create_multi): one X,
// the target columns Y and weight columns W ([ntargets][n_pad] each), owned
// jointly by the parent and its views and freed with the last of them.
struct MultiMem {
  int device = 0;
  void* X = nullptr;
  void* Y = nullptr;
  void* W = nullptr;
  ~MultiMem() {
    (void)hipSetDevice(device);
    if (X) (void)hipFree(X);
    if (Y) (void)hipFree(Y);
    if (W) (void)hipFree(W);
  }
};

struct srhip_dataset {
  srhip_ctx* ctx = nullptr;
  int dtype = SRHIP_F32;
  int64_t rows = 0;
  int nfeat = 0;
  int64_t n_pad = 0;
  void* X = nullptr;
  void* y = nullptr;
  void* w = nullptr;
  double sum_w = 0.0, sum_yw = 0.0;
  bool x_finite = true;
  std::vector<double> h_w;  // host copy of the shard weights (Σw of row samples)
  // multi-target datasets and their views: X / y / w point into mem and are not
  // freed by the dataset. ntargets > 1 (the parent): y / w are the first of
  // ntargets columns n_pad rows apart, t_* the per-target Σw, Σy·w and weights.
  int ntargets = 1;
  std::shared_ptr<MultiMem> mem;
  std::vector<double> t_sum_w, t_sum_yw;
  std::vector<std::vector<double>> t_h_w;
  // column pool: the shared-subtree columns of loss tree code over this dataset's own X
  // ([pool_cols][n_pad] Float32, column = the subtree's slot in the context's registry) and the
  // canonical text each column holds ("": none). Kept from call to call: run_eval derives only
  // the columns whose key differs from the calling program's (shared_columns).
  DevBuf pool;
  int pool_cols = 0;
  std::vector<std::string> pool_key;
};

struct srhip_program {
  srhip_ctx* ctx = nullptr;
  int dtype = SRHIP_F32;
  int ntrees = 0;
  // host copy of the postfix streams (for set_constants → recompile)
  std::vector<int32_t> node_off, const_off;
  std::vector<uint8_t> kind;
  std::vector<uint16_t> arg;
  std::vector<unsigned char> consts;
  // compiled metadata
  std::vector<int32_t> nodes;
  std::vector<uint8_t> static_fail, fail_if_rows;
  // the static verdicts on the device (srhip_eval_loss_packed), uploaded when stale
  uint8_t* d_verdict = nullptr;
  bool verdict_stale = true;
  int max_feature = -1;
  int64_t total_nodes = 0;
  // device
  void* d_code = nullptr;
  int32_t* d_tree_off = nullptr;
  int32_t* d_list = nullptr;  // [nlist_a + nlist_b]: shallow trees then deep trees
  int nlist_a = 0, nlist_b = 0;
  // tree code (jit.cpp) of the first nlist_j shallow slots, Float32 programs
  jit::Module* jit = nullptr;
  jit::Module64* jit64 = nullptr;  // Float64 programs: the same slots as Float64 tree code (jit64.cpp)
  int nlist_j = 0;
  std::vector<int32_t> h_jit_list;  // the trees of those slots, in slot order
  // the same trees' tree code for other elementwise losses (jit::Options::loss),
  // built at a loss's first evaluation; null m: that loss runs interpreted
  struct LossJit { int kind; uint64_t bits; jit::Module* m; };
  mutable std::vector<LossJit> jit_loss;
  // Float64 programs: the same trees' tree code for the other losses and for
  // per-row outputs (kind -2), built at first use (module64)
  struct LossJit64 { int kind; uint64_t bits; jit::Module64* m; };
  mutable std::vector<LossJit64> jit64_loss;
  // the constants the tree code was built with: the trees of a later loss or
  // output build are compiled with them, so that every tree folds and fails
  // statically as in that build (the slot layouts match); memory-constant code
  // reads the current constants from the programs either way
  std::vector<unsigned char> jit_consts, gjit_consts;
  jit::Stats jit_stats;
  // tree code is compiled for one constant set: a program whose constants are
  // set again (srhip_program_set_constants) runs on the interpreter
  bool jit_allowed = true;
  // tree code whatever the tree count (the shared-subtree derive program: a few dozen subtrees
  // over every row of the call; jit_wanted's 256-tree bar is for the cost of loading a code object
  // per program, which this program pays once and keeps)
  bool jit_forced = false;
  // SRHIP_PROGRAM_WIDE_TREE_CODE: literal loss tree code may be built wide (jit::Options::xg) and
  // stays in use on a dataset whose interpreter passes run wide (run_eval)
  bool wide_tc = false;
  // gradient tree code allowed (the rerun of Periodic's handed-back trees: none)
  bool gjit_allowed = true;
  // the gradient programs were built by a call on per-tree row sets, without tree code
  bool gjit_skipped = false;
  // tree code reads its constants from the device programs (jit::Options::memc):
  // built at the first new constant set, after which set_constants only
  // updates the programs in place
  bool jit_memc = false;
  // host image of the uploaded programs: set_constants patches the device
  // copies in place when only instruction immediates change
  std::vector<unsigned char> h_code, h_gcode;
  std::vector<int32_t> h_toff, h_gtoff, h_len, h_glen;
  // their constant maps (CompiledBatch::cmap / direct): new constants of a
  // tree whose immediates are its constants are written without a recompile
  std::vector<int32_t> h_cmap, h_gcmap;
  std::vector<uint8_t> h_direct, h_gdirect;
  std::vector<FoldRec> h_folds, h_gfolds;
  // the constants each image was last compiled / patched with: a tree that
  // is recompiled at every set (a failing one) is skipped while they stand
  std::vector<unsigned char> h_cprev, h_gcprev;
  int64_t n_inplace = 0, n_rebuild = 0;
  int opset = OPSET_FULL;      // smallest operator set covering the compiled programs
  // expression operators (srhip.h): the definitions this program's trees use, held
  // so that a destroyed handle does not disturb it; whether the deep list of
  // the loss / gradient programs holds their code (it then runs OPSET_EXPR)
  std::vector<std::shared_ptr<const ExprOp>> xops;
  bool has_expr = false, g_has_expr = false;
  // gradient programs (compiled on first use)
  bool grad_built = false;
  bool grad_stale = false;  // constants changed since the gradient programs were patched
  std::vector<uint8_t> g_static_fail;
  // per tree, for the calls that deal their own work items (srhip_eval_loss_deriv): the
  // cost of its gradient program, and 0 shallow / 1 deep / 2 never run (a static verdict)
  std::vector<int32_t> g_cost;
  std::vector<uint8_t> g_class;
  void* d_gcode = nullptr;
  int32_t* d_gtree_off = nullptr;
  int32_t* d_gitems = nullptr;  // work items (tree | group << 24): shallow then deep
  int32_t* d_const_off = nullptr;
  // work items by pass: shallow items carrying 1, 2 or kGradG tangents, then deep ones
  int ngitems[4] = {0, 0, 0, 0};
  int g_opset = OPSET_FULL;
  // gradient tree code (jit_grad.cpp) of the Float32 trees it can compile;
  // with it, the interpreter runs the remaining trees' items (ngitems_rest,
  // stored after the ngitems[] items in d_gitems)
  jit::GradModule* gjit = nullptr;
  jit::GradStats gjit_stats;
  // its candidate trees (cost order) and compiled slot list: the gradient tree
  // code of another elementwise loss is built from the same candidates at that
  // loss's first gradient and used only with the same slots (null m: that
  // loss's gradients run interpreted)
  std::vector<int32_t> h_gcand, h_gjl;
  struct GradLossJit { int kind; uint64_t bits; jit::GradModule* m; };
  std::vector<GradLossJit> gjit_loss;
  int ngitems_rest[4] = {0, 0, 0, 0};
  int32_t* d_gjit_list = nullptr;   // [nslots] tree of each gradient-code slot
  int32_t* d_gjit_cidx = nullptr;   // constants of those trees
  int ngjit_cidx = 0;
  float* d_gconsts = nullptr;       // the constants as Float32 (+16 padding)
  // Float64 programs: the gradient tree code of jit64.cpp (L2), its constants (+16 padding)
  jit::GradModule64* gjit64 = nullptr;
  struct GradLossJit64 { int kind; uint64_t bits; jit::GradModule64* m; };
  std::vector<GradLossJit64> gjit64_loss;  // other losses' Float64 gradient tree code (same slots)
  double* d_gconsts64 = nullptr;
  size_t gcs64_cap = 0;
  size_t gjl_cap = 0, gjc_cap = 0, gcs_cap = 0;
  // byte capacities of the device buffers above (kept across rebuilds)
  size_t code_cap = 0, toff_cap = 0, list_cap = 0;
  size_t gcode_cap = 0, gtoff_cap = 0, gitems_cap = 0, gconst_cap = 0;
  // the shared subtrees of the tree code (jit.h Columns) as a program of their
  // own, run by the interpreter's per-row output mode once per call
  // (derive_shared); built at the first call that needs it
  mutable srhip_program* shared = nullptr;
  mutable std::vector<std::string> shared_keys;
  // the same for the gradient tree code's columns (jit::grad_columns)
  mutable srhip_program* gshared = nullptr;
  mutable std::vector<std::string> gshared_keys;
  // a derive program: the column of each list slot's subtree ([nlist_a + nlist_b], device; in place
  // of d_list, so per-row outputs and per-column results land in the subtree's column) and the
  // column of each subtree (host)
  int32_t* d_col_list = nullptr;
  std::vector<int32_t> h_cols;
};

namespace {

// The scope of a call on a context: its mutex held, its device current.
struct CallScope {
  std::lock_guard<std::mutex> lk;
  CallScope(srhip_ctx* c, const char* what) : lk(c->mu) {
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) throw Error(SRHIP_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
  }
};
// (a failing hipSetDevice is reported with the caller's expression, as HIP_CHECK words it)
#define CALL_SCOPE(ctx) CallScope scope((ctx), "hipSetDevice(" #ctx "->device)")

// the program's own trees as the tree compilers take them, with the given constants
srhip_trees trees_of(const srhip_program* p, const void* consts) {
  srhip_trees tr;
  tr.ntrees = p->ntrees;
  tr.node_off = p->node_off.data();
  tr.kind = p->kind.data();
  tr.arg = p->arg.data();
  tr.const_off = p->const_off.data();
  tr.consts = consts;
  return tr;
}

// ---- expression losses (srhip.h "expression losses") ----------------------------
// A registered loss tree: its postfix stream (the host statement of the
// semantics, srhip_loss_expr_eval) and its loss program for both element types
// (srhip_internal.h "expression-loss programs"). Entries are immutable; the
// registry is process-wide and hands out kinds from SRHIP_EXPR_LOSS_BEGIN on,
// never twice.
struct ExprLoss {
  std::vector<uint8_t> kind;
  std::vector<uint16_t> arg;
  std::vector<double> consts;
  bool uses_w = false;
  std::vector<Ins<float>> p32;
  std::vector<Ins<double>> p64;
};
std::mutex g_expr_mu;
std::vector<std::pair<int32_t, std::shared_ptr<const ExprLoss>>> g_expr;
int32_t g_expr_next = SRHIP_EXPR_LOSS_BEGIN;

std::shared_ptr<const ExprLoss> expr_loss_lookup(int32_t kind) {
  std::lock_guard<std::mutex> lk(g_expr_mu);
  for (const auto& e : g_expr)
    if (e.first == kind) return e.second;
  throw Error(SRHIP_ERR_INVALID, "loss kind " + std::to_string(kind) + " is not a registered expression loss");
}

// an expression loss that reads the weight needs a weighted dataset
void check_expr_loss_weights(int32_t kind, bool weighted) {
  if (kind < SRHIP_EXPR_LOSS_BEGIN) return;
  if (expr_loss_lookup(kind)->uses_w && !weighted)
    throw Error(SRHIP_ERR_INVALID, "the expression loss reads the weight (feature 2) but the dataset has no weights");
}

// Validate a postfix loss stream and compile it. Malformed: INVALID; well formed
// but beyond the limits (nodes, stack depth, operator tables): UNSUPPORTED.
std::shared_ptr<const ExprLoss> expr_loss_compile(const uint8_t* kind, const uint16_t* arg, int32_t nnodes,
                                                  const double* consts, int32_t nconsts) {
  if (!kind || !arg || nnodes <= 0 || nconsts < 0 || (nconsts > 0 && !consts))
    throw Error(SRHIP_ERR_INVALID, "expression loss: null or empty node stream");
  struct N { int l = -1, r = -1; };
  std::vector<N> nd((size_t)nnodes);
  std::vector<int> st;
  int nc = 0, maxdepth = 0;
  bool beyond_ops = false, uses_w = false;
  for (int i = 0; i < nnodes; ++i) {
    switch (kind[i]) {
      case SRHIP_NODE_CONST:
        if (nc >= nconsts) throw Error(SRHIP_ERR_INVALID, "expression loss: more constant leaves than constants");
        if (!std::isfinite(consts[nc])) throw Error(SRHIP_ERR_INVALID, "expression loss: non-finite constant");
        ++nc;
        break;
      case SRHIP_NODE_FEATURE:
        if (arg[i] > 2) throw Error(SRHIP_ERR_INVALID, "expression loss: feature index beyond 2 (0: prediction, 1: target, 2: weight)");
        uses_w = uses_w || arg[i] == 2;
        break;
      case SRHIP_NODE_UNARY:
        if (st.empty()) throw Error(SRHIP_ERR_INVALID, "expression loss: stack underflow");
        beyond_ops = beyond_ops || arg[i] >= SRHIP_NUM_UOPS;
        nd[i].l = st.back();
        st.pop_back();
        break;
      case SRHIP_NODE_BINARY:
        if (st.size() < 2) throw Error(SRHIP_ERR_INVALID, "expression loss: stack underflow");
        beyond_ops = beyond_ops || arg[i] >= SRHIP_NUM_BOPS;
        nd[i].r = st.back();
        st.pop_back();
        nd[i].l = st.back();
        st.pop_back();
        break;
      default: throw Error(SRHIP_ERR_INVALID, "expression loss: unknown node kind");
    }
    st.push_back(i);
    maxdepth = std::max(maxdepth, (int)st.size());
  }
  if (st.size() != 1) throw Error(SRHIP_ERR_INVALID, "expression loss: the stream leaves " + std::to_string(st.size()) + " values");
  if (nc != nconsts) throw Error(SRHIP_ERR_INVALID, "expression loss: constant count mismatch");
  if (beyond_ops) throw Error(SRHIP_ERR_UNSUPPORTED, "expression loss: operator id beyond the engine's table");
  if (nnodes > kLossMaxNodes) throw Error(SRHIP_ERR_UNSUPPORTED, "expression loss: more than 64 nodes");
  if (maxdepth > kLossMaxDepth) throw Error(SRHIP_ERR_UNSUPPORTED, "expression loss: more than 4 values live on the stack");

  auto e = std::make_shared<ExprLoss>();
  e->kind.assign(kind, kind + nnodes);
  e->arg.assign(arg, arg + nnodes);
  e->consts.assign(consts, consts + nconsts);
  e->uses_w = uses_w;
  // constant index of each constant leaf
  std::vector<int> cidx((size_t)nnodes, -1);
  for (int i = 0, c = 0; i < nnodes; ++i)
    if (kind[i] == SRHIP_NODE_CONST) cidx[i] = c++;
  struct I { uint32_t code; double imm; };
  std::vector<I> prog;
  auto is_leaf = [&](int i) { return kind[i] == SRHIP_NODE_CONST || kind[i] == SRHIP_NODE_FEATURE; };
  auto leaf_of = [&](int i) { return kind[i] == SRHIP_NODE_CONST ? (int)LEAF_IMM : (int)arg[i]; };
  auto imm_of = [&](int i) { return kind[i] == SRHIP_NODE_CONST ? consts[cidx[i]] : 0.0; };
  std::function<void(int, int)> emit = [&](int i, int k) {  // k: slots in use
    if (is_leaf(i)) {
      prog.push_back({make_loss_code(LOP_LD, leaf_of(i)), imm_of(i)});
    } else if (kind[i] == SRHIP_NODE_UNARY) {
      emit(nd[i].l, k);
      prog.push_back({make_loss_code(LOP_UN0 + arg[i], 0), 0.0});
    } else {
      const int l = nd[i].l, r = nd[i].r, b = arg[i];
      if (is_leaf(r)) {
        emit(l, k);
        prog.push_back({make_loss_code(LOP_AX0 + b, leaf_of(r)), imm_of(r)});
      } else if (is_leaf(l)) {
        emit(r, k);
        prog.push_back({make_loss_code(LOP_XA0 + b, leaf_of(l)), imm_of(l)});
      } else {
        if (k >= kLossSlots) throw Error(SRHIP_ERR_UNSUPPORTED, "expression loss: needs more than 3 stack slots");
        emit(l, k);
        prog.push_back({make_loss_code(LOP_PUSH0 + k, 0), 0.0});
        emit(r, k + 1);
        prog.push_back({make_loss_code(LOP_POP0 + k, 0), 0.0});
        prog.push_back({make_loss_code(LOP_TA0 + b, 0), 0.0});
      }
    }
  };
  emit(nnodes - 1, 0);
  for (int k = 0; k < 3; ++k) prog.push_back({make_loss_code(LOP_END, 0), 0.0});  // END + the prefetch's slack
  for (const I& in : prog) {
    Ins<float> a;
    a.code = in.code;
    a.imm = (float)in.imm;
    e->p32.push_back(a);
    Ins<double> d;
    d.code = in.code;
    d.pad = 0u;
    d.imm = in.imm;
    e->p64.push_back(d);
  }
  return e;
}

// ℓ(ŷ, y, w) per row on the host, in T, with the routines constant folding uses
template <typename T>
void expr_loss_eval_host(const ExprLoss& e, const T* yhat, const T* y, const T* w, int64_t n, T* out) {
  const int nn = (int)e.kind.size();
  for (int64_t i = 0; i < n; ++i) {
    T st[kLossMaxDepth];
    int sp = 0, c = 0;
    for (int k = 0; k < nn; ++k) {
      switch (e.kind[k]) {
        case SRHIP_NODE_CONST: st[sp++] = (T)e.consts[c++]; break;
        case SRHIP_NODE_FEATURE: st[sp++] = e.arg[k] == 0 ? yhat[i] : e.arg[k] == 1 ? y[i] : w[i]; break;
        case SRHIP_NODE_UNARY: st[sp - 1] = host::unop<T>(e.arg[k], st[sp - 1]); break;
        default:
          st[sp - 2] = host::binop<T>(e.arg[k], st[sp - 2], st[sp - 1]);
          --sp;
      }
    }
    out[i] = st[0];
  }
}

// The loss program of an expression loss in the context's device memory
// (uploaded once per context, handle and element type; the context's mutex is held).
template <typename T>
const Ins<T>* expr_loss_device(srhip_ctx* c, int32_t kind) {
  const int dtype = sizeof(T) == 4 ? SRHIP_F32 : SRHIP_F64;
  for (const auto& lp : c->lprogs)
    if (lp.kind == kind && lp.dtype == dtype) return static_cast<const Ins<T>*>(lp.d);
  const std::shared_ptr<const ExprLoss> e = expr_loss_lookup(kind);
  const void* src;
  size_t bytes;
  if constexpr (sizeof(T) == 4) { src = e->p32.data(); bytes = e->p32.size() * sizeof(Ins<float>); }
  else { src = e->p64.data(); bytes = e->p64.size() * sizeof(Ins<double>); }
  void* d = nullptr;
  hipError_t err = hipMalloc(&d, bytes);
  if (err != hipSuccess) throw Error(SRHIP_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(err));
  err = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);  // synchronous: in place before any launch reads it
  if (err != hipSuccess) {
    (void)hipFree(d);
    throw Error(SRHIP_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(err));
  }
  c->lprogs.push_back({kind, dtype, d});
  return static_cast<const Ins<T>*>(d);
}

// Programs are rebuilt by every srhip_program_set_constants (the batched
// constant optimiser does so once per line-search round) and hipFree
// synchronises the device, so rebuilds reuse buffers that are large enough.
void ensure_dev(void** ptr, size_t* cap, size_t bytes) {
  if (*ptr && *cap >= bytes) return;
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  HIP_CHECK(hipMalloc(ptr, bytes));
  *cap = bytes;
}

// ---- per-call kernel timing (no synchronisation per launch) -----------------------
void timing_reset(srhip_ctx* c) {
  c->last_ms = 0.0;
  c->last_launches = 0;
  c->last_bailed = 0;
  c->last_redone = 0;
  c->tpairs = 0;
  c->timing_pending = false;
  c->cnt_pending = false;
}
int timed_begin(srhip_ctx* c, hipStream_t s) {
  while (c->tev.size() < 2 * (size_t)(c->tpairs + 1)) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    c->tev.push_back(e);
  }
  HIP_CHECK(hipEventRecord(c->tev[2 * (size_t)c->tpairs], s));
  return c->tpairs++;
}
void timed_end(srhip_ctx* c, hipStream_t s, int k) {
  HIP_CHECK(hipEventRecord(c->tev[2 * (size_t)k + 1], s));
  c->timing_pending = true;
  c->last_launches += 1;
}
// after the stream is synchronised: kernel times and the copied-back counters
void timing_finish(srhip_ctx* c) {
  if (c->timing_pending) {
    double tot = 0.0;
    for (int k = 0; k < c->tpairs; ++k) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, c->tev[2 * (size_t)k], c->tev[2 * (size_t)k + 1]));
      tot += ms;
    }
    c->last_ms = tot;
    c->timing_pending = false;
  }
  if (c->cnt_pending) {
    c->last_redone = c->pin_cnt[1];
    c->cnt_pending = false;
  }
}
// the timing and counters of a call that returned before its results were read
// (srhip_eval_loss_packed): wait for it, under the context's lock, and read them
void flush_pending(srhip_ctx* c) {
  if (!c->timing_pending && !c->cnt_pending) return;
  CALL_SCOPE(c);
  HIP_CHECK(hipStreamSynchronize(c->stream));
  timing_finish(c);
}

void free_grad_device(srhip_program* p) {
  for (void* q : {p->d_gcode, (void*)p->d_gtree_off, (void*)p->d_gitems, (void*)p->d_const_off,
                  (void*)p->d_gjit_list, (void*)p->d_gjit_cidx, (void*)p->d_gconsts})
    if (q) (void)hipFree(q);
  p->d_gcode = nullptr;
  p->d_gtree_off = p->d_gitems = p->d_const_off = nullptr;
  p->d_gjit_list = p->d_gjit_cidx = nullptr;
  p->d_gconsts = nullptr;
  p->gcode_cap = p->gtoff_cap = p->gitems_cap = p->gconst_cap = 0;
  p->gjl_cap = p->gjc_cap = p->gcs_cap = 0;
  jit::destroy_grad(p->gjit);
  p->gjit = nullptr;
  for (auto& l : p->gjit_loss) jit::destroy_grad(l.m);
  p->gjit_loss.clear();
  jit::destroy_grad64(p->gjit64);
  p->gjit64 = nullptr;
  for (auto& l : p->gjit64_loss) jit::destroy_grad64(l.m);
  p->gjit64_loss.clear();
  if (p->d_gconsts64) (void)hipFree(p->d_gconsts64);
  p->d_gconsts64 = nullptr;
  p->gcs64_cap = 0;
  p->grad_built = false;
}

// Gradient tree code on/off: SRHIP_GJIT=0 never, =1 for every Float32
// program, default for programs of at least 256 trees (loading a code object
// costs about a millisecond).
bool gjit_wanted(int ntrees) {
  if (!jit::available() || ntrees == 0) return false;
  const int k = env_01("SRHIP_GJIT");
  return k >= 0 ? k == 1 : ntrees >= 256;
}

// LDS for the row tiles of a gradient tree-code workgroup; more tiles per
// workgroup amortise each tree's call over more rows
size_t gjit_tile_budget() { return (size_t)52 * 1024; }

// the constants the gradient tree code reads (s_load), 16 of padding: Float32
// (jit_grad.cpp) or Float64 (jit64.cpp) as the program's
void upload_gconsts(srhip_program* p) {
  const size_t nconst = p->const_off.back();
  if (p->dtype == SRHIP_F64) {
    std::vector<double> h(nconst + 16, 0.0);
    if (nconst) std::memcpy(h.data(), p->consts.data(), nconst * sizeof(double));
    ensure_dev((void**)&p->d_gconsts64, &p->gcs64_cap, h.size() * sizeof(double));
    HIP_CHECK(hipMemcpyAsync(p->d_gconsts64, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->ctx->stream));
  } else {
    std::vector<float> h(nconst + 16, 0.0f);
    if (nconst) std::memcpy(h.data(), p->consts.data(), nconst * sizeof(float));
    ensure_dev((void**)&p->d_gconsts, &p->gcs_cap, h.size() * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(p->d_gconsts, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, p->ctx->stream));
  }
  HIP_CHECK(hipStreamSynchronize(p->ctx->stream));
}

void free_loss_jits(const srhip_program* p) {
  for (auto& l : p->jit_loss) jit::destroy(l.m);
  p->jit_loss.clear();
  for (auto& l : p->jit64_loss) jit::destroy64(l.m);
  p->jit64_loss.clear();
}

void free_program_device(srhip_program* p) {
  for (srhip_program** q : {&p->shared, &p->gshared})
    if (*q) {
      free_program_device(*q);
      delete *q;
      *q = nullptr;
    }
  p->shared_keys.clear();
  p->gshared_keys.clear();
  jit::destroy(p->jit);
  p->jit = nullptr;
  jit::destroy64(p->jit64);
  p->jit64 = nullptr;
  free_loss_jits(p);
  p->nlist_j = 0;
  if (p->d_code) (void)hipFree(p->d_code);
  if (p->d_verdict) (void)hipFree(p->d_verdict);
  p->d_verdict = nullptr;
  p->verdict_stale = true;
  if (p->d_tree_off) (void)hipFree(p->d_tree_off);
  if (p->d_list) (void)hipFree(p->d_list);
  if (p->d_col_list) (void)hipFree(p->d_col_list);
  p->d_col_list = nullptr;
  p->d_code = nullptr;
  p->d_tree_off = nullptr;
  p->d_list = nullptr;
  p->code_cap = p->toff_cap = p->list_cap = 0;
  free_grad_device(p);
}

// New constants (p->consts) into a built program image, compiling only the
// trees that need it: a tree whose constant-derived immediates are all in the
// constant map (direct) gets the new values written through it — a constant
// as given, a folded subtree evaluated again (eval_fold) — as long as every
// new constant and folded value is finite (the static verdicts then stay
// clear); the others (static failures, non-finite values) are compiled again
// as one small batch and must keep their instruction stream (a tree that
// newly fails statically keeps its old code; its verdict decides its result).
// Returns false when the layout must change (the caller rebuilds: the image
// may then be half patched). *verdicts_changed is set when a static verdict
// moved.
template <typename T>
bool patch_image(srhip_program* p, std::vector<unsigned char>& code, const std::vector<int32_t>& toff,
                 const std::vector<int32_t>& len, std::vector<int32_t>& cmap, std::vector<uint8_t>& direct,
                 std::vector<FoldRec>& folds, std::vector<uint8_t>& sfail, std::vector<uint8_t>* fir, bool grad,
                 bool* verdicts_changed, std::vector<unsigned char>& cprev, int64_t* n_recompiled = nullptr) {
  const int nt = p->ntrees;
  if (cmap.size() * sizeof(Ins<T>) != code.size() || (int)direct.size() != nt || (int)toff.size() != nt ||
      (int)len.size() != nt || (int)sfail.size() != nt)
    return false;
  Ins<T>* ins = reinterpret_cast<Ins<T>*>(code.data());
  const T* c = reinterpret_cast<const T*>(p->consts.data());
  const int32_t* co = p->const_off.data();
  const srhip_trees tr = trees_of(p, c);  // the program's own trees with the new constants (eval_fold)
  std::vector<int32_t> redo;
  const bool keep = p->jit_memc;  // compiled with keep_layout: every tree has its code
  const T* cp = cprev.size() == p->consts.size() ? reinterpret_cast<const T*>(cprev.data()) : nullptr;
  for (int t = 0; t < nt; ++t) {
    if (!direct[t] && cp && std::memcmp(cp + co[t], c + co[t], (size_t)(co[t + 1] - co[t]) * sizeof(T)) == 0)
      continue;  // compiled with these very constants: same code, same verdict
    if (direct[t] && keep) {
      // keep_layout: the code stays, the verdict follows from the patched
      // immediates as compile_batch decides it — a folded subtree that is no
      // longer finite fails the tree statically; else a non-finite constant
      // operand does (fail_if_rows for a tree that is one constant)
      bool fold_bad = false, const_bad = false, unsure = false;
      for (int i = toff[t], e = toff[t] + len[t]; i < e; ++i) {
        const int32_t m = cmap[i];
        if (m >= 0) {
          ins[i].imm = c[m];
          const_bad |= !std::isfinite(c[m]);
        } else if (m <= -2) {
          const FoldRec& f = folds[-2 - m];
          if (!eval_fold<T>(f, tr, &ins[i].imm)) {
            ins[i].imm = std::numeric_limits<T>::quiet_NaN();
            if (f.node_e - f.node_b >= kMaxFoldDepth) unsure = true;  // eval_fold's stack, not the value
            else fold_bad = true;
          }
        }
      }
      if (!unsure) {
        const int nb = p->node_off[t], ne = p->node_off[t + 1];
        const bool one_const = ne - nb == 1 && p->kind[nb] == SRHIP_NODE_CONST;
        const uint8_t nsf = (uint8_t)(grad ? const_bad : (fold_bad || (const_bad && !one_const)));
        const uint8_t nfir = (uint8_t)(!grad && !fold_bad && const_bad && one_const);
        if (sfail[t] != nsf || (fir && (*fir)[t] != nfir)) *verdicts_changed = true;
        sfail[t] = nsf;
        if (fir) (*fir)[t] = nfir;
        continue;
      }
    } else if (direct[t]) {
      bool finite = true;
      for (int k = co[t]; k < co[t + 1]; ++k) finite &= std::isfinite(c[k]);
      for (int i = toff[t], e = toff[t] + len[t]; i < e && finite; ++i) {
        const int32_t m = cmap[i];
        if (m >= 0) ins[i].imm = c[m];
        else if (m <= -2) finite = eval_fold<T>(folds[-2 - m], tr, &ins[i].imm);
      }
      if (finite) continue;
    }
    redo.push_back(t);
  }
  if (n_recompiled) *n_recompiled = (int64_t)redo.size();
  if (env_set("SRHIP_DEBUG_SETC")) std::fprintf(stderr, "srhip set_constants: %d of %d trees recompiled\n", (int)redo.size(), nt);
  if (redo.empty()) {
    cprev = p->consts;
    return true;
  }
  const int nr = (int)redo.size();
  std::vector<int32_t> s_noff(1, 0), s_coff(1, 0);
  std::vector<uint8_t> s_kind;
  std::vector<uint16_t> s_arg;
  std::vector<T> s_c;
  for (int32_t t : redo) {
    const int b = p->node_off[t], e = p->node_off[t + 1];
    s_kind.insert(s_kind.end(), p->kind.begin() + b, p->kind.begin() + e);
    s_arg.insert(s_arg.end(), p->arg.begin() + b, p->arg.begin() + e);
    s_c.insert(s_c.end(), c + co[t], c + co[t + 1]);
    s_noff.push_back((int32_t)s_kind.size());
    s_coff.push_back((int32_t)s_c.size());
  }
  srhip_trees sub;
  sub.ntrees = nr;
  sub.node_off = s_noff.data();
  sub.kind = s_kind.data();
  sub.arg = s_arg.data();
  sub.const_off = s_coff.data();
  sub.consts = s_c.data();
  CompiledBatch<T> rb = compile_batch_par<T>(sub, grad, p->jit_memc);
  for (int r = 0; r < nr; ++r) {
    const int t = redo[r];
    if (rb.tree_off[r] >= 0) {
      if (toff[t] < 0 || rb.len[r] != len[t]) return false;
      const Ins<T>* src = &rb.code[rb.tree_off[r]];
      for (int j = 0; j < len[t]; ++j)
        if (src[j].code != ins[toff[t] + j].code) return false;
      for (int j = 0; j < len[t]; ++j) {
        ins[toff[t] + j] = src[j];
        const int32_t m = rb.cmap[rb.tree_off[r] + j];
        int32_t& dst = cmap[toff[t] + j];
        if (m >= 0) {
          dst = co[t] + (m - s_coff[r]);
        } else if (m <= -2) {  // the fold, in the program's numbering (reusing the slot it had)
          const FoldRec& f = rb.folds[-2 - m];
          const FoldRec g{p->node_off[t] + (f.node_b - s_noff[r]), p->node_off[t] + (f.node_e - s_noff[r]),
                          co[t] + (f.const_b - s_coff[r])};
          if (dst <= -2) {
            folds[-2 - dst] = g;
          } else {
            folds.push_back(g);
            dst = -2 - ((int32_t)folds.size() - 1);
          }
        } else {
          dst = -1;
        }
      }
      direct[t] = rb.direct[r];
    } else {
      direct[t] = 0;  // keeps its old code: the static verdict decides its result
    }
    if (sfail[t] != rb.static_fail[r] || (fir && (*fir)[t] != rb.fail_if_rows[r])) *verdicts_changed = true;
    sfail[t] = rb.static_fail[r];
    if (fir) (*fir)[t] = rb.fail_if_rows[r];
  }
  cprev = p->consts;
  return true;
}

// New constants for built gradient programs: immediates patched in place when
// the programs keep their shape, else a rebuild. Deferred from set_constants
// to the next gradient call (a line search sets constants many times between
// two gradient calls).
template <typename T>
void patch_grad_constants(srhip_program* p) {
  p->grad_stale = false;
  bool vchg = false;  // the gradient kernels read the verdicts from the programs themselves
  if (patch_image<T>(p, p->h_gcode, p->h_gtoff, p->h_glen, p->h_gcmap, p->h_gdirect, p->h_gfolds, p->g_static_fail,
                     nullptr, /*grad=*/true, &vchg, p->h_gcprev)) {
    hipStream_t s = p->ctx->stream;
    HIP_CHECK(hipMemcpyAsync(p->d_gcode, p->h_gcode.data(), p->h_gcode.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (p->gjit || p->gjit64) upload_gconsts(p);
  } else {
    p->grad_built = false;  // rebuilt below
  }
}

// Gradient programs: compiled without folding, one work item per (tree,
// tangent group of kGradG constants), cost-sorted.
// tree_code false (a call on per-tree row sets, which never runs it): no gradient
// tree code is built; the first later call that could run it builds the programs
// again with it.
template <typename T>
void build_grad_program(srhip_program* p, bool tree_code = true) {
  if (p->grad_built && tree_code && p->gjit_skipped) p->grad_built = false;
  if (p->grad_built && p->grad_stale) patch_grad_constants<T>(p);
  if (p->grad_built) return;
  p->gjit_skipped = !tree_code && p->gjit_allowed && gjit_wanted(p->ntrees);
  CompiledBatch<T> cb = compile_batch_par<T>(trees_of(p, p->consts.data()), /*grad=*/true, p->jit_memc);
  if (p->ntrees >= (1 << 24)) throw Error(SRHIP_ERR_UNSUPPORTED, "too many trees for gradient work items");
  p->g_static_fail = cb.static_fail;
  p->g_has_expr = std::find(cb.expr.begin(), cb.expr.end(), (uint8_t)1) != cb.expr.end();
  p->g_opset = OPSET_BASIC;
  for (const Ins<T>& ins : cb.code) {
    const int opc = (int)(ins.code & 0xffu);
    if (opc >= kNumOpcodes) continue;  // an expression operator's micro-instruction (deep list only)
    if (opc >= OP_BIN0 ? !opset_has_bop(OPSET_BASIC, (opc - OP_BIN0) % SRHIP_NUM_BOPS)
                       : opc >= OP_UN0 && !opset_has_uop(OPSET_BASIC, opc - OP_UN0))
      p->g_opset = OPSET_FULL;
  }
  // gradient tree code for the Float32 trees it can compile (cost-sorted slots)
  jit::destroy_grad(p->gjit);
  p->gjit = nullptr;
  for (auto& l : p->gjit_loss) jit::destroy_grad(l.m);
  p->gjit_loss.clear();
  jit::destroy_grad64(p->gjit64);
  p->gjit64 = nullptr;
  for (auto& l : p->gjit64_loss) jit::destroy_grad64(l.m);
  p->gjit64_loss.clear();
  p->h_gcand.clear();
  p->h_gjl.clear();
  p->gjit_stats = jit::GradStats();
  std::vector<uint8_t> in_jit(p->ntrees, 0);
  std::vector<int32_t> gjl, gcidx;
  if constexpr (std::is_same<T, float>::value) {
    std::vector<int32_t> cand;
    for (int t = 0; t < p->ntrees; ++t)
      if (cb.tree_off[t] >= 0 && !cb.expr[t]) cand.push_back(t);
    if (tree_code && p->gjit_allowed && gjit_wanted((int)cand.size())) {
      std::stable_sort(cand.begin(), cand.end(), [&](int32_t x, int32_t y) {
        return cb.cost[x] != cb.cost[y] ? cb.cost[x] > cb.cost[y] : x < y;
      });
      std::vector<int32_t> rest;
      p->gjit = jit::build_grad(cb, p->const_off, cand, gjl, rest, &p->gjit_stats);
      if (p->gjit) {
        p->h_gcand = cand;
        p->h_gjl = gjl;
        p->gjit_consts = p->consts;
      }
      if (p->gjit)
        for (int32_t t : gjl) {
          in_jit[t] = 1;
          for (int k = p->const_off[t]; k < p->const_off[t + 1]; ++k) gcidx.push_back(k);
        }
      else
        gjl.clear();
    }
  } else {  // Float64: the gradient tree code of jit64.cpp (L2)
    std::vector<int32_t> cand;
    for (int t = 0; t < p->ntrees; ++t)
      if (cb.tree_off[t] >= 0 && !cb.expr[t]) cand.push_back(t);
    if (tree_code && p->gjit_allowed && gjit_wanted((int)cand.size()) && jit::available64()) {
      std::stable_sort(cand.begin(), cand.end(), [&](int32_t x, int32_t y) {
        return cb.cost[x] != cb.cost[y] ? cb.cost[x] > cb.cost[y] : x < y;
      });
      std::vector<int32_t> rest;
      p->gjit64 = jit::build_grad64(cb, p->const_off, cand, gjl, rest, &p->gjit_stats);
      if (p->gjit64) {
        p->h_gcand = cand;
        p->h_gjl = gjl;
        p->gjit_consts = p->consts;
        for (int32_t t : gjl) {
          in_jit[t] = 1;
          for (int k = p->const_off[t]; k < p->const_off[t + 1]; ++k) gcidx.push_back(k);
        }
      } else {
        gjl.clear();
      }
    }
  }
  // a work item carries the tangents of its group only: groups of 1 and 2
  // constants run in kernels with fewer tangents (and more rows per lane)
  auto by_cost = [](const std::pair<int, int32_t>& x, const std::pair<int, int32_t>& y) {
    return x.first != y.first ? x.first > y.first : x.second < y.second;
  };
  p->g_cost.assign(p->ntrees, 0);
  p->g_class.assign(p->ntrees, 2);
  for (int t = 0; t < p->ntrees; ++t) {
    if (cb.tree_off[t] < 0) continue;
    p->g_cost[t] = cb.cost[t];
    p->g_class[t] = (cb.need[t] > 4 || cb.expr[t]) ? 1 : 0;
  }
  std::vector<int32_t> items;
  for (int rest_only = 0; rest_only < 2; ++rest_only) {
    std::vector<std::pair<int, int32_t>> cls[4];  // (cost, item)
    for (int t = 0; t < p->ntrees; ++t) {
      if (cb.tree_off[t] < 0 || (rest_only && in_jit[t])) continue;
      const int nc = p->const_off[t + 1] - p->const_off[t];
      const int ngroups = std::max(1, (nc + kGradG - 1) / kGradG);
      for (int gi = 0; gi < ngroups; ++gi) {
        const int ntan = std::min(kGradG, nc - gi * kGradG);
        const int k = (cb.need[t] > 4 || cb.expr[t]) ? 3 : ntan <= 1 ? 0 : ntan <= 2 ? 1 : 2;
        cls[k].push_back({cb.cost[t], (int32_t)(t | (gi << 24))});
      }
    }
    for (int k = 0; k < 4; ++k) {
      std::stable_sort(cls[k].begin(), cls[k].end(), by_cost);
      for (auto& q : cls[k]) items.push_back(q.second);
      (rest_only ? p->ngitems_rest : p->ngitems)[k] = (int)cls[k].size();
    }
  }
  std::vector<int32_t> toff(cb.tree_off);
  for (auto& v : toff) v = std::max(v, 0);
  hipStream_t s = p->ctx->stream;
  ensure_dev(&p->d_gcode, &p->gcode_cap, std::max<size_t>(cb.code.size(), 1) * sizeof(Ins<T>));
  ensure_dev((void**)&p->d_gtree_off, &p->gtoff_cap, std::max<size_t>(toff.size(), 1) * sizeof(int32_t));
  ensure_dev((void**)&p->d_gitems, &p->gitems_cap, std::max<size_t>(items.size(), 1) * sizeof(int32_t));
  ensure_dev((void**)&p->d_const_off, &p->gconst_cap, p->const_off.size() * sizeof(int32_t));
  HIP_CHECK(hipMemcpyAsync(p->d_gcode, cb.code.data(), cb.code.size() * sizeof(Ins<T>), hipMemcpyHostToDevice, s));
  if (!toff.empty())
    HIP_CHECK(hipMemcpyAsync(p->d_gtree_off, toff.data(), toff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (!items.empty())
    HIP_CHECK(hipMemcpyAsync(p->d_gitems, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(p->d_const_off, p->const_off.data(), p->const_off.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
  p->ngjit_cidx = (int)gcidx.size();
  if (p->gjit || p->gjit64) {
    ensure_dev((void**)&p->d_gjit_list, &p->gjl_cap, gjl.size() * sizeof(int32_t));
    HIP_CHECK(hipMemcpyAsync(p->d_gjit_list, gjl.data(), gjl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ensure_dev((void**)&p->d_gjit_cidx, &p->gjc_cap, std::max<size_t>(gcidx.size(), 1) * sizeof(int32_t));
    if (!gcidx.empty())
      HIP_CHECK(hipMemcpyAsync(p->d_gjit_cidx, gcidx.data(), gcidx.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (p->gjit || p->gjit64) upload_gconsts(p);
  p->h_gcode.assign(reinterpret_cast<const unsigned char*>(cb.code.data()),
                    reinterpret_cast<const unsigned char*>(cb.code.data() + cb.code.size()));
  p->h_gtoff = cb.tree_off;
  p->h_glen = cb.len;
  p->h_gcmap = cb.cmap;
  p->h_gdirect = cb.direct;
  p->h_gfolds = cb.folds;
  p->h_gcprev = p->consts;
  p->grad_built = true;
  p->grad_stale = false;
}

// Tree code (jit.cpp, jit64.cpp) on/off: SRHIP_JIT=0 never, =1 for every
// program, default for programs of at least 256 shallow trees (code generation
// ~5 µs per tree, loading a code object about a millisecond). The bar was 512
// until round 4: a 512-tree shard of config #2 (bench.py --shard trees, N = 8)
// has 509-512 shallow trees — a tree folds to a constant or fails statically —
// so three of the eight shards ran interpreted at 0.84-0.89 ms against
// 0.55-0.64 ms for the others (profiles/r04_shard_fast.jsonl).
// SRHIP_JIT_FAST=0 keeps the FAST path out.
bool jit_wanted(int nshallow) {
  if (!jit::available() || nshallow == 0) return false;
  const int k = env_01("SRHIP_JIT");
  return k >= 0 ? k == 1 : nshallow >= 256;
}
// Tree code: SRHIP_JIT_CONTIG=1 gives tree group g the contiguous slots
// [g*tpb, (g+1)*tpb) of the cost-sorted list (its code one contiguous range).
// Measured slower than the snake deal (config #2 3.39 -> 3.63 ms, config #5
// gradient 49.6 -> 60.9 ms: the expensive trees end up in a few groups;
// profiles/r02i_evalknobs.txt), so off by default.
bool jit_contig() { return env_is1("SRHIP_JIT_CONTIG"); }  // read per launch: A/B measurements

// Tree code: every tree group of a row group on one XCD, so that the row
// group's X tile comes from HBM once and from that XCD's L2 for the other tree
// groups (config #2: 110 -> 32 MB fetched per launch, 3.006 -> 2.982 ms);
// SRHIP_RG_XCD=0: blocks in launch order
bool rg_xcd() { return env_on("SRHIP_RG_XCD"); }  // read per launch: A/B measurements
// SRHIP_TG_MAJOR=1 (experiment, read per launch): within an XCD the blocks
// run tree group by tree group (jit_template.hip block_of, rotate 3), so the
// workgroups resident on a CU share their tree code in the instruction cache
int rotate_mode() {
  if (!rg_xcd()) return 0;
  return env_is1("SRHIP_TG_MAJOR") ? 3 : 2;
}

bool zero_copy_enabled() { return env_on("SRHIP_ZERO_COPY"); }  // read per call: A/B measurements
void ensure_pinned(srhip_ctx* c, size_t nt);

// Wait for a call's last launch by polling the stream instead of the runtime's
// blocking wait: hipStreamSynchronize sleeps on a completion interrupt, whose
// wake-up costs tens of microseconds per call on an idle host (more when the
// cores sit in deep C-states), on every synchronous eval_loss. The spin is
// bounded (SRHIP_SPIN_US, default 200 µs: a loss call of a search-sized batch
// ends well within it) and then falls back to the blocking wait, so a long
// kernel (config #5's 48 ms gradients) does not hold a host core that the
// caller's other threads need. SRHIP_SPIN=0: the blocking wait (A/B).
void wait_stream(hipStream_t s) {
  if (!env_on("SRHIP_SPIN")) {  // read per call: A/B measurements
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  static const double budget_us = [] {
    return std::max(0.0, env_double("SRHIP_SPIN_US", 200.0));
  }();
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t r;
  int k = 0;
  while ((r = hipStreamQuery(s)) == hipErrorNotReady) {
    __builtin_ia32_pause();
    if ((++k & 63) == 0 &&
        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > budget_us) {
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
  }
  HIP_CHECK(r);
}

// LDS for the row tiles of a tree-code workgroup (SRHIP_EVAL_LDS, KiB)
size_t jit_tile_budget() {
  static const size_t b = (size_t)env_int("SRHIP_EVAL_LDS", 40) * 1024;
  return b;
}
bool jit_fast_enabled() { return env_on("SRHIP_JIT_FAST"); }
// SRHIP_COLUMN_CACHE=0 (read per build and per call: tests): shared-subtree columns numbered per
// program and derived at every call, as before the datasets' column pools
bool column_cache_enabled() { return env_on("SRHIP_COLUMN_CACHE"); }
// the registry that numbers a program's shared-subtree columns, or null: the program's own numbering
// (a derive program's subtrees are not shared further)
SlotRegistry* column_slots(const srhip_program* p) {
  return column_cache_enabled() && !p->jit_forced ? &p->ctx->slots : nullptr;
}

template <typename T>
void build_program(srhip_program* p) {
  CompiledBatch<T> cb = compile_batch_par<T>(trees_of(p, p->consts.data()), /*grad=*/false, p->jit_memc);
  p->nodes = cb.nodes;
  p->static_fail = cb.static_fail;
  p->fail_if_rows = cb.fail_if_rows;
  p->verdict_stale = true;
  p->max_feature = cb.max_feature;
  p->total_nodes = cb.total_nodes;
  // operator set: every opcode left after folding must be in it
  p->opset = OPSET_BASIC;
  for (const Ins<T>& ins : cb.code) {
    const int opc = (int)(ins.code & 0xffu);
    if (opc >= kNumOpcodes) continue;  // an expression operator's micro-instruction (deep list only)
    if (opc >= OP_BIN0 ? !opset_has_bop(OPSET_BASIC, (opc - OP_BIN0) % SRHIP_NUM_BOPS)
                       : opc >= OP_UN0 && !opset_has_uop(OPSET_BASIC, opc - OP_UN0))
      p->opset = OPSET_FULL;
  }
  // trees to run, cost-descending; shallow (<= kShallowSlots) and deep lists
  std::vector<int32_t> a, b;
  for (int t = 0; t < p->ntrees; ++t) {
    if (cb.tree_off[t] < 0) continue;
    // (a tree with expression-operator code: the deep list whatever its need)
    (cb.need[t] <= kShallowSlots && cb.len[t] <= kVProgMax && !cb.expr[t] ? a : b).push_back(t);
  }
  p->has_expr = std::find(cb.expr.begin(), cb.expr.end(), (uint8_t)1) != cb.expr.end();
  auto by_cost = [&](int32_t x, int32_t y) {
    return cb.cost[x] != cb.cost[y] ? cb.cost[x] > cb.cost[y] : x < y;
  };
  std::stable_sort(a.begin(), a.end(), by_cost);
  std::stable_sort(b.begin(), b.end(), by_cost);
  // tree code for the shallow Float32 trees of large batches: the compiled
  // trees lead the shallow list, the others follow (interpreter)
  jit::destroy(p->jit);
  p->jit = nullptr;
  jit::destroy64(p->jit64);
  p->jit64 = nullptr;
  free_loss_jits(p);
  p->h_jit_list.clear();
  p->nlist_j = 0;
  p->jit_stats = jit::Stats();
  if constexpr (std::is_same<T, float>::value) {
    if (p->jit_allowed && (jit_wanted((int)a.size()) || (p->jit_forced && jit::available() && !a.empty()))) {
      std::vector<int32_t> jl, rest;
      jit::Options jo;
      jo.fast = jit_fast_enabled();
      jo.memc = p->jit_memc || env_is1("SRHIP_JIT_MEMC");  // read per build: tests
      // wide code when a candidate reads a feature past the LDS tile's reach (features 0 .. 62)
      jo.xg = p->wide_tc && !jo.memc && jit::max_feature_read(cb, a) >= 63;
      jo.slots = column_slots(p);
      p->jit = jit::build(cb, a, jl, rest, jo, &p->jit_stats);
      if (p->jit) {
        p->nlist_j = (int)jl.size();
        p->h_jit_list = jl;
        p->jit_consts = p->consts;
        a = jl;
        a.insert(a.end(), rest.begin(), rest.end());
      }
    }
  } else {
    // Float64 tree code (jit64.cpp) for the shallow trees of large batches;
    // SRHIP_JIT64=0: interpreted
    static const bool on64 = env_on("SRHIP_JIT64");
    // Float64 tree code holds its constants as literals: a VARYING_CONSTANTS program (the
    // optimiser's candidates) would rebuild it interpreted at its first set_constants
    if (on64 && p->jit_allowed && !p->jit_memc && jit_wanted((int)a.size()) && jit::available64()) {
      std::vector<int32_t> jl, rest;
      p->jit64 = jit::build64(cb, a, jl, rest, &p->jit_stats);
      if (p->jit64) {
        p->nlist_j = (int)jl.size();
        p->h_jit_list = jl;
        p->jit_consts = p->consts;
        a = jl;
        a.insert(a.end(), rest.begin(), rest.end());
      }
    }
  }
  p->nlist_a = (int)a.size();
  p->nlist_b = (int)b.size();
  std::vector<int32_t> list(a);
  list.insert(list.end(), b.begin(), b.end());
  std::vector<int32_t> toff(cb.tree_off);
  for (auto& v : toff) v = std::max(v, 0);
  // second half of d_list: program offset of every list slot (one load
  // instead of list -> tree_off when the kernel prefetches the next program)
  const size_t nl = list.size();
  list.resize(2 * nl);
  for (size_t k = 0; k < nl; ++k) list[nl + k] = toff[list[k]];

  p->grad_built = false;  // the gradient programs embed the constants too
  hipStream_t s = p->ctx->stream;
  HIP_CHECK(hipStreamSynchronize(s));  // no launch may still read the old buffers
  // +64 instructions of OP_END padding: the VGPR-resident program load reads
  // 64 instructions from the start of every program
  const size_t ncode_alloc = cb.code.size() + 64;
  ensure_dev(&p->d_code, &p->code_cap, ncode_alloc * sizeof(Ins<T>));
  HIP_CHECK(hipMemsetAsync(p->d_code, 0, ncode_alloc * sizeof(Ins<T>), p->ctx->stream));
  ensure_dev((void**)&p->d_tree_off, &p->toff_cap, std::max<size_t>(toff.size(), 1) * sizeof(int32_t));
  ensure_dev((void**)&p->d_list, &p->list_cap, std::max<size_t>(list.size(), 1) * sizeof(int32_t));
  HIP_CHECK(hipMemcpyAsync(p->d_code, cb.code.data(), cb.code.size() * sizeof(Ins<T>), hipMemcpyHostToDevice, s));
  if (!toff.empty())
    HIP_CHECK(hipMemcpyAsync(p->d_tree_off, toff.data(), toff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (!list.empty())
    HIP_CHECK(hipMemcpyAsync(p->d_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
  p->h_code.assign(reinterpret_cast<const unsigned char*>(cb.code.data()),
                   reinterpret_cast<const unsigned char*>(cb.code.data() + cb.code.size()));
  p->h_toff = cb.tree_off;
  p->h_len = cb.len;
  p->h_cmap = cb.cmap;
  p->h_direct = cb.direct;
  p->h_folds = cb.folds;
  p->h_cprev = p->consts;
}

void build_program_f32(srhip_program* p) { build_program<float>(p); }

// srhip_program_set_constants: new immediates written into the host image
// through its constant map (patch_image) and the device programs overwritten
// in place (no reallocation, no list rebuild; the gradient programs are
// patched at the next gradient call); a changed layout rebuilds.
template <typename T>
void update_constants(srhip_program* p) {
  // (wide Float32 code likewise: memory-constant code keeps its constants where wide code's column base lives)
  if (p->jit64 || jit::xg(p->jit)) {  // Float64 tree code holds its constants as literals: interpreted from now on
    p->jit_allowed = false;
    ++p->n_rebuild;
    const bool had_grad = p->grad_built;
    build_program<T>(p);
    if (had_grad) {
      p->grad_built = true;
      p->grad_stale = true;
    }
    return;
  }
  if (p->jit && !p->jit_memc && !jit::memc(p->jit)) {
    // first new constant set of a tree-code program with constants in its
    // code: rebuilt once as memory-constant tree code (jit.cpp Gen::memc),
    // which later constant sets reach through the in-place program update
    p->jit_memc = true;
    ++p->n_rebuild;
    const bool had_grad = p->grad_built;
    build_program<T>(p);
    if (had_grad) {  // same trees: the gradient programs (and their tree code) only need the constants
      p->grad_built = true;
      p->grad_stale = true;
    }
    return;
  }
  if (!p->jit) p->jit_allowed = false;
  // same layout: the immediates and the host-side static verdicts change in
  // place (the host image is idle: every upload of it ends in a synchronisation,
  // and the copy is ordered after the launches that read the old programs)
  bool vchg = false;
  const auto t0 = std::chrono::steady_clock::now();
  if (!patch_image<T>(p, p->h_code, p->h_toff, p->h_len, p->h_cmap, p->h_direct, p->h_folds, p->static_fail,
                      &p->fail_if_rows, /*grad=*/false, &vchg, p->h_cprev)) {
    ++p->n_rebuild;
    build_program<T>(p);
    if (env_set("SRHIP_DEBUG_SETC"))
      std::fprintf(stderr, "srhip set_constants: full rebuild of %d trees %.1f us\n", p->ntrees,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    return;
  }
  if (vchg) p->verdict_stale = true;
  const auto t1 = std::chrono::steady_clock::now();
  hipStream_t s = p->ctx->stream;
  HIP_CHECK(hipMemcpyAsync(p->d_code, p->h_code.data(), p->h_code.size(), hipMemcpyHostToDevice, s));
  if (p->grad_built) p->grad_stale = true;  // patched by the next gradient call (patch_grad_constants)
  HIP_CHECK(hipStreamSynchronize(s));
  if (env_set("SRHIP_DEBUG_SETC"))
    std::fprintf(stderr, "srhip set_constants: patch %.1f us, upload of %zu bytes %.1f us\n",
                 std::chrono::duration<double, std::micro>(t1 - t0).count(), p->h_code.size(),
                 std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count());
  ++p->n_inplace;
}

void check_program_vs_dataset(const srhip_dataset* ds, const srhip_program* p, bool multi_ok = false) {
  if (!ds || !p) throw Error(SRHIP_ERR_INVALID, "null dataset or program");
  if (ds->ntargets > 1 && !multi_ok)
    throw Error(SRHIP_ERR_INVALID, "dataset has " + std::to_string(ds->ntargets) +
                                       " targets: take a view of one (srhip_dataset_view) or use srhip_eval_loss_targets");
  // a dataset is read-only device memory once created: any context of its
  // device may evaluate a program on it (the program's context runs the call)
  if (ds->ctx->device != p->ctx->device)
    throw Error(SRHIP_ERR_INVALID, "dataset is on device " + std::to_string(ds->ctx->device) + " but the program on device " +
                                       std::to_string(p->ctx->device) +
                                       ": create the program with a context of the dataset's device");
  if (ds->dtype != p->dtype) throw Error(SRHIP_ERR_INVALID, "dataset and program dtypes differ");
  if (p->max_feature >= ds->nfeat)
    throw Error(SRHIP_ERR_INVALID, "tree references feature " + std::to_string(p->max_feature + 1) +
                                       " but the dataset has " + std::to_string(ds->nfeat));
  if (!ds->x_finite)
    throw Error(SRHIP_ERR_UNSUPPORTED,
                "X contains non-finite values: did_succeed of fused leaves differs from the reference; use the CPU path");
}

// Threaded interpreter on/off (SRHIP_TI=0 disables it; built only when the
// kernels were compiled with SR_TI).
static bool ti_enabled() { return ti_compiled() && env_on("SRHIP_TI"); }  // read per launch: tests compare both paths

// Wide datasets: an interpreter pass whose row tile of all
// nfeat features does not fit in LDS runs the wide kernel variant, which reads
// its feature operands from global memory. SRHIP_WIDE (read per call): unset:
// wide only where the LDS plan fails; 1: every interpreter pass wide and no
// tree code (tests, A/B runs); 0: no wide kernels, UNSUPPORTED as before them.
static int wide_mode() {
  const char* e = env_str("SRHIP_WIDE");
  return (!e || !e[0]) ? -1 : (e[0] == '0' ? 0 : 1);
}
[[noreturn]] static void throw_lds(int nfeat) {
  throw Error(SRHIP_ERR_UNSUPPORTED, "row tile of " + std::to_string(nfeat) + " features does not fit in LDS");
}
// The plan of an interpreter evaluation pass: the LDS plan where it fits, else the wide one.
static void plan_interp(int dtype, bool deep, int opset, int mode, bool weighted, int nfeat, int64_t rows, int nlist,
                        EvalPlan* plan, int ntgt = 0) {
  const int wm = wide_mode();
  if (wm != 1 && plan_eval(dtype, deep, opset, mode, weighted, nfeat, rows, nlist, plan, ntgt)) return;
  if (wm != 0 && plan_eval_wide(dtype, mode, weighted, rows, nlist, plan, ntgt)) return;
  throw_lds(nfeat);
}
static const char* interp_name(size_t esz, bool wide) {
  return wide ? (esz == 4 ? "eval_kernel_wide<float>" : "eval_kernel_wide<double>")
              : (esz == 4 ? "eval_kernel<float>" : "eval_kernel<double>");
}

// Row-group rotation of the tree order, off by default (SRHIP_ROT=1 enables
// it): measured 4.09 -> 4.15 ms on config #2.
// The interpreter kernels' waves take their trees from an LDS counter
// (eval_kernel.h, a.rotate & 4): interleaved A/B (tools/interp_dyn_ab.py,
// profiles/r04_interp_dyn_ab.jsonl) config #3 interpreted 0.511 → 0.469 ms,
// a 300-tree batch 0.117 → 0.112, config #2 interpreted 5.95 → 5.90; sums bit
// for bit. SRHIP_INTERP_DYN=0 (read per launch): round-robin.
static bool interp_dyn() { return env_on("SRHIP_INTERP_DYN"); }
static bool rotate_enabled() { return env_is1("SRHIP_ROT"); }  // read per launch: A/B measurements

// Trees whose tree code handed a tile back (a sin/cos argument beyond the
// fast reduction, jit_template.hip) are evaluated again, whole, by the
// shallow interpreter kernel; finalize overwrites their results.
template <typename T>
void rerun_bailed(srhip_ctx* c, const srhip_program* p, jit::Module* jm, const EvalArgs<T>& ja, const EvalPlan& jplan,
                  int nfeat, int64_t rows, int loss, double lparam) {
  (void)jplan;
  if constexpr (std::is_same<T, float>::value) {
    hipStream_t s = c->stream;
    const int nj = p->nlist_j;
    if (!jit::module_bails(jm)) return;  // no routine hands a tile back: the finalize copied the counters
    std::vector<uint32_t> flags((size_t)nj + 2);
    HIP_CHECK(hipMemcpyAsync(flags.data(), jit::bail_flags(jm), flags.size() * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    c->last_redone = flags[nj + 1];
    if (flags[nj] == 0) return;
    std::vector<int32_t> slots;
    for (int k = 0; k < nj; ++k)
      if (flags[k]) slots.push_back(k);
    if (slots.empty()) return;
    // list = tree ids, list_off = program offsets (copied from the program's list)
    std::vector<int32_t> all((size_t)2 * (p->nlist_a + p->nlist_b));
    HIP_CHECK(hipMemcpyAsync(all.data(), p->d_list, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t nl = (size_t)p->nlist_a + p->nlist_b;
    const int nb = (int)slots.size();
    std::vector<int32_t> bl(2 * (size_t)nb);
    for (int k = 0; k < nb; ++k) {
      bl[k] = all[slots[k]];
      bl[nb + k] = all[nl + slots[k]];
    }
    c->bail_list.ensure(bl.size() * sizeof(int32_t));
    c->bail_fail.ensure((size_t)nb * sizeof(uint32_t));
    HIP_CHECK(hipMemcpyAsync(c->bail_list.p, bl.data(), bl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(c->bail_fail.p, 0, (size_t)nb * sizeof(uint32_t), s));
    EvalPlan plan;
    plan_interp(p->dtype, false, OPSET_FULL, MODE_LOSS, ja.w != nullptr, nfeat, rows, nb, &plan);
    EvalArgs<T> a = ja;
    a.contig = 0;  // the interpreter kernel deals its slots in snake order
    a.rotate = 0;
    a.list = static_cast<const int32_t*>(c->bail_list.p);
    a.list_off = a.list + nb;
    a.fail = static_cast<uint32_t*>(c->bail_fail.p);
    a.nlist = nb;
    a.ti_rec = nullptr;
    if (ti_enabled() && !plan.wide) {
      c->ti_rec.ensure((size_t)nb * 64 * sizeof(uint4));
      HIP_CHECK(launch_ti_records(reinterpret_cast<const Ins<float>*>(a.prog), a.list_off, nb,
                                  (uint32_t)(plan.ntiles * plan.tile * sizeof(T)), static_cast<uint4*>(c->ti_rec.p), s));
      a.ti_rec = static_cast<const uint4*>(c->ti_rec.p);
    }
    a.ntiles = plan.ntiles;
    a.ntg = plan.ntg;
    a.tpb = plan.tpb;
    a.nrg = plan.nrg;
    a.loss = loss;
    a.lparam = lparam;
    c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * sizeof(Part<T>));
    a.partial = static_cast<Part<T>*>(c->partial.p);
    const int tk = timed_begin(c, s);
    note_kernel(interp_name(sizeof(T), plan.wide));
    HIP_CHECK(launch_eval<T>(plan, a, MODE_LOSS, s));
    timed_end(c, s, tk);
    HIP_CHECK(launch_finalize<T>(a, c->res_sum, c->res_ok, s));
    c->last_bailed = nb;
    if (env_set("SRHIP_DEBUG_PASSES")) std::fprintf(stderr, "srhip pass bail-rerun: %d trees\n", nb);
  }
}

// Compute units of the context's device (queried once).
int device_cus(const srhip_ctx* c) {
  // contexts on several threads may ask at once: each entry is written with
  // the same value by whichever thread gets there first
  static std::atomic<int> cus[64];
  const int d = c->device;
  if (d < 0 || d >= 64) return 256;
  int v = cus[d].load(std::memory_order_relaxed);
  if (!v) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) v = 256;
    cus[d].store(v, std::memory_order_relaxed);
  }
  return v;
}

// Tree-code grids whose workgroups fill a whole number of rounds of the
// device's resident workgroups plus a fraction f of one: the last round
// would run with most of the device idle. The row groups past the whole
// rounds are cut into single tiles instead (a quarter of the work each),
// when their rounds, ceil(f·ntiles)/ntiles, come to less than a full one.
// Rounds are counted at 5 waves per SIMD (the tree code's 94 VGPRs, LDS per
// workgroup sized to match: jit::lds_per_workgroup). SRHIP_JIT_TAIL=0 keeps
// every row group whole.
void tail_split(const srhip_ctx* c, EvalPlan* plan, int64_t rows, int jw) {
  static const bool on = env_on("SRHIP_JIT_TAIL");
  if (!on || plan->ntiles < 2 || rows <= 0) return;
  const int64_t conc = (int64_t)device_cus(c) * std::max(1, 20 / jw);
  const int64_t W = (int64_t)plan->nrg * plan->ntg;
  const int64_t full = W / conc;
  const int64_t rest = W - full * conc;  // workgroups of the last, partial round
  if (full < 1 || rest == 0) return;
  // row groups in the whole rounds (the remaining ones become single tiles)
  const int64_t nbig = full * conc / plan->ntg;
  const int64_t left_rows = rows - nbig * (int64_t)plan->rows_wg;
  if (nbig < 1 || left_rows <= 0) return;
  const int64_t nsmall = (left_rows + plan->tile - 1) / plan->tile;
  const int64_t small_rounds_x = (nsmall * plan->ntg + conc - 1) / conc;  // rounds of single-tile groups
  if (small_rounds_x >= plan->ntiles) return;  // no shorter than one more round of whole groups
  plan->nbig = (int)nbig;
  plan->ts = 1;
  plan->nrg = (int)(nbig + nsmall);
}

// The tail split along trees (tail_map.h; loss tree code under its
// hand-written loops). A launch of many rounds ends on whole workgroups: with
// config #2's 241 trees per group one lasts ≈ 0.18 ms, and every compute unit
// waits on units of that size while the launch drains. The row-wise split
// above does not apply there (the last round is nearly full) and cuts the
// wrong way for this kernel: a quarter of the rows per call multiplies the
// per-call costs by 4. Here the last row groups keep their tiles per call and
// each of their tree groups is run by S workgroups, launched last: the same
// calls, in units a S-th the size.
//   SRHIP_JIT_TAIL_TREES   S: 2, 4 or 8; 1 none; 0 the largest of them that
//                          leaves every wave at least 4 trees; unset: 4, or
//                          fewer by that rule
//   SRHIP_JIT_TAIL_ROUNDS  the split workgroups come to this many rounds of
//                          the resident workgroups (rounds as tail_split
//                          counts them; a fraction is fine)
//   SRHIP_JIT_TAIL_RG      n >= 0: the last n row groups are split whatever
//                          the rounds (tests: a small grid never fills one)
// All read per launch. SRHIP_JIT_TAIL=0 turns this split off as well. The
// split workgroups are launched last and walk unrotated (jit_template.hip);
// by rounds they never reach into the first round, whose simultaneous start
// the rotation is there for (forced by SRHIP_JIT_TAIL_RG they may: that costs
// speed, never a result). Defaults from the sweep S ∈ {2, 4, 8} × rounds ∈ {1, 1.5, 2}
// (profiles/tail_trees_sweep.json, one process, settings alternating): config
// #2 at 1M rows 2.299 ms unsplit, 2.281 / 2.280 / 2.281 (S = 2), 2.264 / 2.265
// / 2.268 (S = 4), 2.284 / 2.270 / 2.265 (S = 8); its 125k-row shard and the
// 512-tree shard unchanged within their spread. DESIGN.md §3.1.
constexpr int kTailTreesDefault = 4;
constexpr double kTailRoundsDefault = 1.5;
void tail_trees(const srhip_ctx* c, EvalPlan* plan, int jw) {
  plan->tbig = -1;
  plan->tsub = 1;
  if (!env_on("SRHIP_JIT_TAIL") || plan->nbig >= 0 || plan->nrg < 1) return;
  // unset: the default, or fewer where it would leave a wave under 4 trees; 0: the same rule from 8
  const char* es = env_str("SRHIP_JIT_TAIL_TREES");
  int S = es ? std::atoi(es) : kTailTreesDefault;
  if (!es || S == 0)
    for (S = S == 0 ? 8 : S; S > 1 && plan->tpb / (S * std::max(1, jw)) < 4;) S >>= 1;
  if (S != 2 && S != 4 && S != 8) return;
  const int forced = env_int("SRHIP_JIT_TAIL_RG", -1);
  int64_t ntail;
  if (forced >= 0) {
    ntail = std::min<int64_t>(forced, plan->nrg);
  } else {
    const double rounds = env_double("SRHIP_JIT_TAIL_ROUNDS", kTailRoundsDefault);
    const int64_t conc = (int64_t)device_cus(c) * std::max(1, 20 / jw);
    const int64_t first = (conc + plan->ntg - 1) / plan->ntg;  // row groups of the first round
    if (!(rounds > 0.0)) return;
    ntail = std::min<int64_t>((int64_t)(rounds * (double)conc / ((double)plan->ntg * S) + 0.5), plan->nrg - first);
  }
  if (ntail < 1) return;
  int64_t tbig = plan->nrg - ntail;
  if (forced < 0 && rg_xcd()) {
    // the XCD-dealt block order runs the head in whole octets of row groups (no padding blocks
    // there): tbig down to a multiple of 8, but not into the first round
    const int64_t first = ((int64_t)device_cus(c) * std::max(1, 20 / jw) + plan->ntg - 1) / plan->ntg;
    tbig &= ~(int64_t)7;
    if (tbig < first) tbig = (first + 7) & ~(int64_t)7;
    if (tbig >= plan->nrg) return;
  }
  plan->tbig = (int)tbig;
  plan->tsub = S;
}

// The skeleton of the tree-code modules built at first use: the module cached
// under (kind, bits), else the program's trees compiled again with the
// constants of the first build (`consts`), `build` run on them, a module whose
// slot layout is not that build's (`same_layout` false) destroyed, and the
// result, null included, cached with the program.
template <typename T, typename M, typename Cache, typename Build, typename Same, typename Destroy>
M* lazy_module(const srhip_program* p, Cache& cache, int kind, uint64_t bits, const std::vector<unsigned char>& consts,
               bool grad, Build build, Same same_layout, Destroy destroy) {
  for (const auto& l : cache)
    if (l.kind == kind && l.bits == bits) return l.m;
  const CompiledBatch<T> cb = compile_batch_par<T>(trees_of(p, consts.data()), grad);
  std::vector<int32_t> jl, rest;
  M* m = build(cb, jl, rest);
  if (m && !same_layout(jl, rest)) {
    destroy(m);  // a different slot layout: interpreted
    m = nullptr;
  }
  cache.push_back({kind, bits, m});
  return m;
}

uint64_t bits_of(double lparam) {
  uint64_t bits;
  std::memcpy(&bits, &lparam, 8);
  return bits;
}

// The tree code of a Float32 program for an elementwise loss: the L2 build
// itself, or (other losses) the same trees compiled with that loss's tile
// tail, built at the loss's first evaluation and kept with the program
// (SRHIP_JIT_LOSSES=0: other losses interpreted). Null: no tree code.
jit::Module* loss_module(const srhip_program* p, int loss, double lparam) {
  if (!p->jit || p->nlist_j == 0) return nullptr;
  if (loss == SRHIP_LOSS_L2) return p->jit;
  static const bool on = env_on("SRHIP_JIT_LOSSES");
  if (!on || loss < 0 || loss >= SRHIP_NUM_LOSSES || !jit::has_loss_routine(loss)) return nullptr;
  jit::Options jo;
  jo.fast = jit_fast_enabled();
  jo.memc = jit::memc(p->jit);
  jo.xg = jit::xg(p->jit);
  jo.loss = loss;
  jo.lparam = bits_of(lparam);
  jo.slots = column_slots(p);
  return lazy_module<float, jit::Module>(
      p, p->jit_loss, loss, jo.lparam, p->jit_consts, false,
      [&](const CompiledBatch<float>& cb, std::vector<int32_t>& jl, std::vector<int32_t>& rest) {
        jit::Stats st;
        return jit::build(cb, p->h_jit_list, jl, rest, jo, &st);
      },
      [&](const std::vector<int32_t>& jl, const std::vector<int32_t>& rest) { return jl == p->h_jit_list && rest.empty(); },
      jit::destroy);
}

// The Float64 tree code of a program for an elementwise loss (L2: the build
// itself; the others: the same trees with that loss's routine in the tile
// tail, jit64.cpp emit_tail_loss) or for per-row outputs (kind -2:
// srhip_eval_tree_array, jit64.cpp emit_store_out), built at its first use
// and kept with the program; null (SRHIP_JIT64_EXTRA=0, a different slot
// layout): interpreted. The constants are literals of the code: new constants
// destroy it with the L2 build (update_constants).
jit::Module64* module64(const srhip_program* p, int kind, double lparam) {
  if (!p->jit64 || p->nlist_j == 0) return nullptr;
  if (kind == SRHIP_LOSS_L2) return p->jit64;
  static const bool on = env_on("SRHIP_JIT64_EXTRA");
  if (!on || kind < -2 || kind >= SRHIP_NUM_LOSSES || (kind >= 0 && !jit::has_loss_routine64(kind))) return nullptr;
  jit::Opts64 o;
  o.out = kind == -2;
  o.loss = kind == -2 ? SRHIP_LOSS_L2 : kind;
  o.lparam = kind == -2 ? 0 : bits_of(lparam);
  return lazy_module<double, jit::Module64>(
      p, p->jit64_loss, kind, o.lparam, p->jit_consts, false,
      [&](const CompiledBatch<double>& cb, std::vector<int32_t>& jl, std::vector<int32_t>& rest) {
        jit::Stats st;
        return jit::build64(cb, p->h_jit_list, jl, rest, &st, o);
      },
      [&](const std::vector<int32_t>& jl, const std::vector<int32_t>& rest) { return jl == p->h_jit_list && rest.empty(); },
      jit::destroy64);
}

// The per-row output tree code of a Float32 program (srhip_eval_tree_array):
// the same trees compiled with jit::Options::out, PRECISE routines only, built
// at the first per-row evaluation and kept with the program (kind -2 in
// jit_loss); null (SRHIP_JIT_OUT=0, a different slot layout): interpreted.
jit::Module* out_module(const srhip_program* p) {
  if (!p->jit || p->nlist_j == 0) return nullptr;
  static const bool on = env_on("SRHIP_JIT_OUT");
  if (!on || jit::xg(p->jit)) return nullptr;  // (no wide per-row output code)
  jit::Options jo;
  jo.fast = false;
  jo.memc = jit::memc(p->jit);
  jo.out = true;
  return lazy_module<float, jit::Module>(
      p, p->jit_loss, -2, 0, p->jit_consts, false,
      [&](const CompiledBatch<float>& cb, std::vector<int32_t>& jl, std::vector<int32_t>& rest) {
        jit::Stats st;
        return jit::build(cb, p->h_jit_list, jl, rest, jo, &st);
      },
      [&](const std::vector<int32_t>& jl, const std::vector<int32_t>& rest) { return jl == p->h_jit_list && rest.empty(); },
      jit::destroy);
}

// The gradient tree code of a Float32 program for an elementwise loss: the
// L2 build, or the same candidates compiled with that loss's seed (jit_grad.cpp
// emit_loss_seed), built at the loss's first gradient and kept with the
// program; null: that loss's gradients run interpreted (SRHIP_JIT_LOSSES=0,
// no dℓ/dr routine, or a different slot layout).
jit::GradModule* grad_module(srhip_program* p, int loss, double lparam) {
  if (!p->gjit) return nullptr;
  if (loss == SRHIP_LOSS_L2) return p->gjit;
  static const bool on = env_on("SRHIP_JIT_LOSSES");
  if (!on || loss < 0 || loss >= SRHIP_NUM_LOSSES || !jit::has_dloss_routine(loss)) return nullptr;
  const uint64_t bits = bits_of(lparam);
  return lazy_module<float, jit::GradModule>(
      p, p->gjit_loss, loss, bits, p->gjit_consts, true,
      [&](const CompiledBatch<float>& cb, std::vector<int32_t>& gjl, std::vector<int32_t>& rest) {
        jit::GradStats st;
        return jit::build_grad(cb, p->const_off, p->h_gcand, gjl, rest, &st, loss, bits);
      },
      [&](const std::vector<int32_t>& gjl, const std::vector<int32_t>&) { return gjl == p->h_gjl; }, jit::destroy_grad);
}

// The same for a Float64 program (jit64.cpp GradGen64): the L2 build, or the
// same candidates compiled with that loss's seed; null: interpreted.
jit::GradModule64* grad_module64(srhip_program* p, int loss, double lparam) {
  if (!p->gjit64) return nullptr;
  if (loss == SRHIP_LOSS_L2) return p->gjit64;
  static const bool on = env_on("SRHIP_JIT_LOSSES");
  if (!on || loss < 0 || loss >= SRHIP_NUM_LOSSES || !jit::has_dloss_routine64(loss)) return nullptr;
  const uint64_t bits = bits_of(lparam);
  return lazy_module<double, jit::GradModule64>(
      p, p->gjit64_loss, loss, bits, p->gjit_consts, true,
      [&](const CompiledBatch<double>& cb, std::vector<int32_t>& gjl, std::vector<int32_t>& rest) {
        jit::GradStats st;
        return jit::build_grad64(cb, p->const_off, p->h_gcand, gjl, rest, &st, loss, bits);
      },
      [&](const std::vector<int32_t>& gjl, const std::vector<int32_t>&) { return gjl == p->h_gjl; },
      jit::destroy_grad64);
}

// The shared subtrees of a tree-code module (jit.h Columns), once per row of
// the call, into c->gderived ([ngcol][n_pad]): the subtrees are a program of
// their own (p->shared, interpreted, no tree code) run in the interpreter's
// per-row output mode — the interpreter's values, which the tree code's
// PRECISE routines equal bit for bit — and its finalize gives each subtree's
// did_succeed over the call's rows; a subtree that failed (some node
// non-finite on some row) has its whole column set to NaN, so every tree
// that reads it fails, as DynamicExpressions fails a tree with a non-finite
// node on any row (src/InterfaceDynamicExpressions.jl:17-48).
// slot / keys: the program's cache of the subtree program (p->shared for the
// loss tree code, p->gshared for the gradient tree code).
// which: the subtrees to derive (indices into jc.gkey, ascending), a program
// of just those; out: the column buffer ([jc.gspan()][n_pad]: c->gderived or
// a dataset's pool), subtree g into column jc.slot(g). The other columns of
// `out` are neither written nor poisoned.
bool derive_jit_enabled() {
  static const bool on = env_on("SRHIP_DERIVE_JIT");
  return on;
}
void derive_shared(srhip_ctx* c, srhip_program*& slot, std::vector<std::string>& keys, const jit::Columns& jc,
                   const std::vector<int>& which, float* out, const float* X, int64_t rows, int64_t n_pad,
                   int nfeat) {
  hipStream_t s = c->stream;
  const int ng = (int)which.size();
  if (ng == 0) return;
  std::vector<std::string> wkeys;
  std::vector<int32_t> wcols;
  for (int g : which) {
    wkeys.push_back(jc.gkey[(size_t)g]);
    wcols.push_back(jc.slot(g));
  }
  if (!slot || keys != wkeys || slot->h_cols != wcols) {
    if (slot) {
      free_program_device(slot);
      delete slot;
      slot = nullptr;
    }
    auto* q = new srhip_program();
    q->ctx = c;
    q->dtype = SRHIP_F32;
    q->ntrees = ng;
    // per-row output tree code for the subtrees (SRHIP_DERIVE_JIT=0: the interpreter's MODE_OUT)
    q->jit_allowed = derive_jit_enabled();
    q->jit_forced = true;
    q->node_off.assign(1, 0);
    for (int g : which) {
      q->kind.insert(q->kind.end(), jc.gkind.begin() + jc.goff[(size_t)g], jc.gkind.begin() + jc.goff[(size_t)g + 1]);
      q->arg.insert(q->arg.end(), jc.garg.begin() + jc.goff[(size_t)g], jc.garg.begin() + jc.goff[(size_t)g + 1]);
      q->node_off.push_back((int32_t)q->kind.size());
    }
    q->const_off.assign((size_t)ng + 1, 0);
    q->consts.resize(1);
    try {
      build_program_f32(q);
      // the column of every list slot's subtree, in list order
      const size_t nl = (size_t)q->nlist_a + q->nlist_b;
      std::vector<int32_t> list(std::max<size_t>(nl, 1));
      if (nl > 0) HIP_CHECK(hipMemcpy(list.data(), q->d_list, nl * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < nl; ++k) list[k] = wcols[(size_t)list[k]];
      HIP_CHECK(hipMalloc((void**)&q->d_col_list, list.size() * sizeof(int32_t)));
      HIP_CHECK(hipMemcpy(q->d_col_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      q->h_cols = wcols;
      ++c->derive_programs;
    } catch (...) {
      free_program_device(q);
      delete q;
      throw;
    }
    slot = q;
    keys = wkeys;
  }
  const srhip_program* q = slot;
  c->cols_derived += ng;
  c->gsum.ensure((size_t)jc.gspan() * sizeof(double));
  c->gok.ensure((size_t)jc.gspan());
  if (q->nlist_a + q->nlist_b != ng) throw Error(SRHIP_ERR_INVALID, "shared subtree failed statically");
  // every subtree as per-row output tree code (jit_template.hip sr_jit_out_d, PRECISE routines:
  // the interpreter's values bit for bit, test_jit_out_gpu.py): one launch per code object part
  jit::Module* om = (q->jit && q->nlist_j == ng && rows > 0) ? out_module(q) : nullptr;
  if (om && !jit::module_bails(om)) {
    const jit::Columns& jc2 = jit::columns(om);
    if (jc2.nraw > nfeat) throw Error(SRHIP_ERR_INVALID, "dataset has fewer features than the subtrees read");
    const int narr = 1 + jc2.nraw + jc2.nder;
    const int jw = jc2.waves;
    const size_t lds_wg = jit::lds_per_workgroup(jw);
    const size_t budget = std::max(jit_tile_budget() * jw / 4,
                                   lds_wg - std::min<size_t>(lds_wg / 4, 8192));
    for (int k = 0; k < jit::nparts(om); ++k) {
      int s0, nsl;
      jit::part(om, k, &s0, &nsl);
      if (nsl == 0) continue;
      EvalPlan plan;
      if (!plan_geometry(4, 4, kShallowSlots, narr, 1, rows, nsl, &plan, budget, 52 * 1024 * jw / 4,
                         16384 * 4 / jw, 64 * jw / 4))
        throw Error(SRHIP_ERR_UNSUPPORTED, "row tile of " + std::to_string(nfeat) + " features does not fit in LDS");
      plan.threads = 64 * jw;
      tail_split(c, &plan, rows, jw);
      EvalArgs<float> a;
      a.prog = static_cast<const Ins<float>*>(q->d_code);
      a.tree_off = q->d_tree_off;
      a.list = q->d_col_list + s0;
      a.list_off = q->d_list + (q->nlist_a + q->nlist_b) + s0;
      a.fail = nullptr;
      a.ti_rec = nullptr;
      a.nlist = nsl;
      a.X = X;
      a.y = nullptr;
      a.w = nullptr;
      a.n = rows;
      a.n_pad = n_pad;
      a.nfeat = nfeat;
      a.ntiles = plan.ntiles;
      a.ntg = plan.ntg;
      a.tpb = plan.tpb;
      a.nrg = plan.nrg;
      a.loss = SRHIP_LOSS_L2;
      a.rotate = rg_xcd() ? rotate_mode() : (rotate_enabled() ? 1 : 0);
      a.contig = 0;
      a.lparam = 0.0;
      c->gpartial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * sizeof(Part<float>));
      a.partial = static_cast<Part<float>*>(c->gpartial.p);
      a.out = out;
      a.out_stride = n_pad;
      HIP_CHECK(jit::launch(om, k, plan, a, false, nullptr, s, nullptr));
      HIP_CHECK(launch_finalize<float>(a, static_cast<double*>(c->gsum.p), static_cast<uint8_t*>(c->gok.p), s));
    }
    HIP_CHECK(launch_poison_columns(static_cast<const uint8_t*>(c->gok.p), q->d_col_list, ng, out, n_pad, s));
    return;
  }
  const int lists[2][2] = {{0, q->nlist_a}, {q->nlist_a, q->nlist_b}};
  for (int pass = 0; pass < 2; ++pass) {
    const int s0 = lists[pass][0], nlist = lists[pass][1];
    if (nlist == 0) continue;
    EvalPlan plan;
    plan_interp(SRHIP_F32, pass == 1, q->opset, MODE_OUT, false, nfeat, rows, nlist, &plan);
    if (plan.tile % 256 != 0)  // the tree code reads whole 256-row tiles of the columns
      throw Error(SRHIP_ERR_INVALID, "shared-subtree derive pass: tile of " + std::to_string(plan.tile) + " rows");
    EvalArgs<float> a;
    a.prog = static_cast<const Ins<float>*>(q->d_code);
    a.tree_off = q->d_tree_off;
    a.list = q->d_col_list + s0;
    a.list_off = q->d_list + (q->nlist_a + q->nlist_b) + s0;
    a.fail = nullptr;
    a.ti_rec = nullptr;
    if (ti_enabled() && pass == 0 && !plan.wide) {
      c->gti.ensure((size_t)nlist * 64 * sizeof(uint4));
      HIP_CHECK(launch_ti_records(a.prog, a.list_off, nlist, (uint32_t)(plan.ntiles * plan.tile * sizeof(float)),
                                  static_cast<uint4*>(c->gti.p), s));
      a.ti_rec = static_cast<const uint4*>(c->gti.p);
    }
    a.nlist = nlist;
    a.X = X;
    a.y = nullptr;
    a.w = nullptr;
    a.n = rows;
    a.n_pad = n_pad;
    a.nfeat = nfeat;
    a.ntiles = plan.ntiles;
    a.ntg = plan.ntg;
    a.tpb = plan.tpb;
    a.nrg = plan.nrg;
    a.loss = SRHIP_LOSS_L2;
    a.rotate = interp_dyn() ? 4 : 0;
    a.contig = 0;
    a.lparam = 0.0;
    c->gpartial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * sizeof(Part<float>));
    a.partial = static_cast<Part<float>*>(c->gpartial.p);
    a.out = out;
    a.out_stride = n_pad;
    HIP_CHECK(launch_eval<float>(plan, a, MODE_OUT, s));
    HIP_CHECK(launch_finalize<float>(a, static_cast<double*>(c->gsum.p), static_cast<uint8_t*>(c->gok.p), s));
  }
  HIP_CHECK(launch_poison_columns(static_cast<const uint8_t*>(c->gok.p), q->d_col_list, ng, out, n_pad, s));
}

// every shared subtree of jc into the context's per-call buffer
const float* percall_columns(srhip_ctx* c, srhip_program*& slot, std::vector<std::string>& keys,
                             const jit::Columns& jc, const float* X, int64_t rows, int64_t n_pad, int nfeat) {
  std::vector<int> all((size_t)jc.ngcol);
  for (int g = 0; g < jc.ngcol; ++g) all[(size_t)g] = g;
  c->gderived.ensure((size_t)jc.gspan() * (size_t)n_pad * sizeof(float));
  derive_shared(c, slot, keys, jc, all, static_cast<float*>(c->gderived.p), X, rows, n_pad, nfeat);
  return static_cast<const float*>(c->gderived.p);
}

// Room for `span` columns in the dataset's pool, within SRHIP_COLUMN_CACHE_MB (default 1024):
// allocated at the first call that needs it and grown, its columns kept, to the highest slot
// used, rounded up to 8 columns. False: over budget or out of memory (the per-call path).
bool pool_reserve(srhip_ctx* c, srhip_dataset* ds, int span) {
  if (span <= ds->pool_cols) return true;
  const size_t col = (size_t)ds->n_pad * sizeof(float);
  const size_t budget = (size_t)std::max(0, env_int("SRHIP_COLUMN_CACHE_MB", 1024)) << 20;
  if ((size_t)span * col > budget) return false;
  const int want = (int)std::min<size_t>(((size_t)span + 7) / 8 * 8, budget / col);
  DevBuf nb;
  try {
    nb.ensure((size_t)want * col);
  } catch (const Error&) {
    return false;
  }
  if (ds->pool_cols > 0) {
    const hipError_t e =
        hipMemcpyAsync(nb.p, ds->pool.p, (size_t)ds->pool_cols * col, hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) {
      nb.release();
      HIP_CHECK(e);
    }
  } else {
    c->pooled.push_back(ds);
  }
  ds->pool.release();  // (hipFree waits for the device: the copy and every earlier reader are done)
  ds->pool = nb;
  ds->pool_cols = want;
  ds->pool_key.resize((size_t)want);
  return true;
}
void pool_release(srhip_dataset* ds) {
  ds->pool.release();
  ds->pool_cols = 0;
  ds->pool_key.clear();
  auto& v = ds->ctx->pooled;
  v.erase(std::remove(v.begin(), v.end(), ds), v.end());
}

// The shared-subtree columns of a loss tree-code launch. On the dataset's own rows, by the
// dataset's own context and with registry-numbered columns (pool != null, jc.pooled): the
// dataset's pool, after deriving the columns whose key the pool does not hold under the
// program's slot — none when an earlier call, of this program or another, left them all.
// Otherwise (a gathered row subset, a program of another context and so another stream, a pool
// over budget, SRHIP_COLUMN_CACHE=0): every column into c->gderived for this call.
const float* shared_columns(srhip_ctx* c, const srhip_program* p, const jit::Columns& jc, srhip_dataset* pool,
                            const float* X, int64_t rows, int64_t n_pad, int nfeat) {
  if (pool && jc.pooled && pool->ctx == c && X == pool->X && rows == pool->rows && n_pad == pool->n_pad &&
      column_cache_enabled() && pool_reserve(c, pool, jc.gspan())) {
    std::vector<int> miss;
    for (int g = 0; g < jc.ngcol; ++g)
      if (pool->pool_key[(size_t)jc.slot(g)] != jc.gkey[(size_t)g]) miss.push_back(g);
    c->cols_reused += jc.ngcol - (int64_t)miss.size();
    float* base = static_cast<float*>(pool->pool.p);
    if (!miss.empty()) {
      for (int g : miss) pool->pool_key[(size_t)jc.slot(g)].clear();  // not valid until the launches are enqueued
      derive_shared(c, p->shared, p->shared_keys, jc, miss, base, X, rows, n_pad, nfeat);
      for (int g : miss) pool->pool_key[(size_t)jc.slot(g)] = jc.gkey[(size_t)g];
    }
    return base;
  }
  return percall_columns(c, p->shared, p->shared_keys, jc, X, rows, n_pad, nfeat);
}

// Run the evaluation kernels for both tree lists. The view (X, y, w, rows,
// n_pad) may be the dataset itself or a gathered row subset.
// pool: the dataset, when the view is the dataset itself (its column pool, shared_columns).
template <typename T>
void run_eval(srhip_ctx* c, const srhip_program* p, int mode, const T* X, const T* y,
              const T* w, int64_t rows, int64_t n_pad, int nfeat, int loss, double lparam,
              T* out, int64_t out_stride, int64_t seg = 0, const int32_t* tgt = nullptr, int ntgt = 0,
              srhip_dataset* pool = nullptr) {
  // tgt (device memory, per tree id): a target per tree; y / w are then ntgt columns
  // n_pad rows apart and every pass runs the interpreter's per-tree-targets variants
  hipStream_t s = c->stream;
  timing_reset(c);
  c->sums.ensure(std::max<size_t>(p->ntrees, 1) * sizeof(double));
  c->oks.ensure(std::max<size_t>(p->ntrees, 1));
  // the finalize writes the per-tree results straight into the pinned host
  // buffers (no copy launches; SRHIP_ZERO_COPY=0: device buffers + copies)
  c->res_host = zero_copy_enabled() && !c->want_device_results;
  if (c->res_host) {
    ensure_pinned(c, std::max<size_t>(p->ntrees, 1));
    c->res_sum = c->pin_sum;
    c->res_ok = c->pin_ok;
  } else {
    c->res_sum = static_cast<double*>(c->sums.p);
    c->res_ok = static_cast<uint8_t*>(c->oks.p);
  }
  const size_t nslots = (size_t)p->nlist_a + p->nlist_b;
  // slot ranges: [0, nj) tree code, [nj, nlist_a) shallow interpreter, then deep
  // (per-tree row sets, seg > 0: the interpreter, one tree per workgroup)
  const int wm = wide_mode();  // 1: no tree code for this call
  jit::Module* jm = (!std::is_same<T, float>::value || seg > 0 || wm == 1 || tgt) ? nullptr
                    : mode == MODE_LOSS                                     ? loss_module(p, loss, lparam)
                                                                            : out_module(p);
  // wide code addresses a feature's column with a 32-bit stride: none for a longer column
  if (jm && jit::xg(jm) && (uint64_t)n_pad * 4u > 0xffffffffu) jm = nullptr;
  // SRHIP_PROGRAM_WIDE_TREE_CODE: literal loss tree code stays in use when an interpreter pass
  // of the call runs wide (each pass follows its own plan, plan_interp)
  const bool keep_tc = jm && p->wide_tc && mode == MODE_LOSS && !jit::memc(jm) && wm != 0;
  // Float64 programs: their tree code (this loss, or per-row outputs)
  jit::Module64* jm64 = nullptr;
  if constexpr (std::is_same<T, double>::value)
    if (p->jit64 && p->nlist_j > 0 && seg == 0 && wm != 1 && !tgt) jm64 = module64(p, mode == MODE_LOSS ? loss : -2, lparam);
  // the row tile of a tree-code part (LDS columns: y, the raw features the tree code reads, its
  // derived columns, w); false: it does not fit in LDS
  auto plan_tree_code = [&](int nlist, EvalPlan* plan) {
    if (jm64) {
      // Float64 tree code: 128-row tiles of y, the features it reads, w; 4 waves
      const int narr = 1 + jit::nraw64(jm64) + (w ? 1 : 0);
      if (jit::nraw64(jm64) > nfeat) throw Error(SRHIP_ERR_INVALID, "dataset has fewer features than the program reads");
      if (!plan_geometry(8, 2, kShallowSlots, narr, 1, rows, nlist, plan, 52 * 1024, 52 * 1024, 16384, 64)) return false;
      plan->threads = 256;
      return true;
    }
    const jit::Columns& jc = jit::columns(jm);
    if (std::max(jc.nraw, jc.xfeat) > nfeat) throw Error(SRHIP_ERR_INVALID, "dataset has fewer features than the program reads");
    const int narr = 1 + jc.nraw + jc.nder + (w ? 1 : 0);
    // partials go to global memory: LDS holds the tiles (1 byte per slot keeps the slot bound away)
    // 16384 workgroups of 4 waves, >= 64 trees per group (16 per wave): config #2 kernel
    // 2.997 -> 2.867 ms at 4096 trees, 0.865 -> 0.828 at 1024, 512 unchanged
    // (profiles/r02n_targetwg.txt); scaled by the waves per workgroup
    const int jw = jc.waves;
    const size_t lds_wg = jit::lds_per_workgroup(jw);
    const size_t budget = std::max(jit_tile_budget() * jw / 4,
                                   lds_wg - std::min<size_t>(lds_wg / 4, 8192));
    if (!plan_geometry(4, 4, kShallowSlots, narr, 1, rows, nlist, plan, budget, 52 * 1024 * jw / 4,
                       16384 * 4 / jw, 64 * jw / 4))
      return false;
    plan->threads = 64 * jw;
    tail_split(c, plan, rows, jw);
    if (mode == MODE_LOSS) tail_trees(c, plan, jw);
    return true;
  };
  // A call with a pass whose row tile does not fit in LDS (the tree code's, or an interpreter
  // pass's for the trees the tree code does not hold) was UNSUPPORTED before the wide kernels:
  // it runs in the interpreter, with no tree code, wide where the tile does not fit
  // (SRHIP_WIDE=0: UNSUPPORTED, as before them). The tree-code plans are kept for the launches.
  std::vector<EvalPlan> tc_plans;
  if ((jm || jm64) && rows > 0 && p->nlist_j > 0) {
    EvalPlan ip;
    bool fits = keep_tc ||
                ((p->nlist_a == p->nlist_j ||
                  plan_eval(p->dtype, false, p->opset, mode, w != nullptr, nfeat, rows, p->nlist_a - p->nlist_j, &ip)) &&
                 (p->nlist_b == 0 || plan_eval(p->dtype, true, p->has_expr ? (int)OPSET_EXPR : (int)OPSET_FULL, mode,
                                               w != nullptr, nfeat, rows, p->nlist_b, &ip)));
    const int np = jm ? jit::nparts(jm) : jit::nparts64(jm64);
    for (int k = 0; k < np && fits; ++k) {
      int s0, nsl;
      if (jm) jit::part(jm, k, &s0, &nsl);
      else jit::part64(jm64, k, &s0, &nsl);
      tc_plans.emplace_back();
      if (nsl > 0) fits = plan_tree_code(nsl, &tc_plans.back());
    }
    if (!fits) {
      if (wm == 0) throw_lds(nfeat);
      jm = nullptr;
      jm64 = nullptr;
    }
  }
  const bool use_jit = jm != nullptr || jm64 != nullptr;
  c->last_jit_trees = (use_jit && rows > 0) ? p->nlist_j : 0;
  const int nj = use_jit ? p->nlist_j : 0;
  // failure flags (and the tree code's bail flags): the finalize kernels of
  // the previous call left them clean; one clearing launch only after a new
  // buffer, an interrupted call or a path that leaves them set (gradients,
  // tree code that can hand tiles back)
  const bool jit_bail = jm != nullptr && jit::module_bails(jm);
  if (mode == MODE_LOSS) {
    const size_t need = std::max<size_t>(nslots, 1) * sizeof(uint32_t);
    if (c->fail.bytes < need) {
      c->fail.ensure(need);
      c->fail_clean = false;
    }
    if (!c->fail_clean || jit_bail)
      HIP_CHECK(launch_zero_words(static_cast<uint32_t*>(c->fail.p), (int64_t)(c->fail.bytes / sizeof(uint32_t)),
                                  jit_bail ? jit::bail_flags(jm) : nullptr, jit_bail ? jit::flag_words(jm) : 0,
                                  s));
    c->fail_clean = false;  // until every finalize of this call is enqueued
  }
  // launches: the tree-code parts (pass -1, one per code object), the shallow
  // interpreter (0), the deep interpreter (1)
  bool any_wide = false;  // the call's kernel name says wide once an interpreter pass ran wide
  struct Launch { int pass, s0, nlist, part; };
  std::vector<Launch> launches;
  if (nj > 0) {
    if constexpr (std::is_same<T, float>::value) {
      for (int k = 0; k < jit::nparts(jm); ++k) {
        int s0, nsl;
        jit::part(jm, k, &s0, &nsl);
        launches.push_back({-1, s0, nsl, k});
      }
    } else {
      for (int k = 0; k < jit::nparts64(jm64); ++k) {
        int s0, nsl;
        jit::part64(jm64, k, &s0, &nsl);
        launches.push_back({-1, s0, nsl, k});
      }
    }
  }
  launches.push_back({0, nj, p->nlist_a - nj, -1});
  launches.push_back({1, p->nlist_a, p->nlist_b, -1});
  const float* shared_cols = nullptr;  // the shared-subtree columns of the tree-code parts
  for (size_t li = 0; li < launches.size(); ++li) {
    const int pass = launches[li].pass;
    const int s0 = launches[li].s0;
    const int nlist = launches[li].nlist;
    const bool last_jit = pass == -1 && (li + 1 == launches.size() || launches[li + 1].pass != -1);
    // no rows (an empty row shard): nothing to launch; every tree's result is
    // its static verdict (finish_results, pack_partials_kernel)
    if (rows == 0) continue;
    if (nlist == 0) {
      if (last_jit) throw Error(SRHIP_ERR_INVALID, "empty tree-code part");
      continue;
    }
    EvalPlan plan;
    if (pass == -1) {
      plan = tc_plans[(size_t)launches[li].part];
    } else {
      plan_interp(p->dtype, pass == 1, (pass == 1 && p->has_expr) ? (int)OPSET_EXPR : p->opset, mode, w != nullptr,
                  nfeat, rows, nlist, &plan, tgt ? ntgt : 0);
    }
    if (seg > 0) {
      // per-tree row sets: one tree per workgroup of one wave, staging its
      // own segment (eval_kernel.h seg0); the segment holds the row groups
      plan.tpb = 1;
      plan.ntg = nlist;
      plan.threads = 64;
      if ((int64_t)plan.nrg * plan.rows_wg > seg) throw Error(SRHIP_ERR_INVALID, "row set segment too short");
    }
    EvalArgs<T> a;
    a.prog = static_cast<const Ins<T>*>(p->d_code);
    a.tree_off = p->d_tree_off;
    a.list = p->d_list + s0;
    a.list_off = p->d_list + (p->nlist_a + p->nlist_b) + s0;
    a.fail = mode == MODE_LOSS ? static_cast<uint32_t*>(c->fail.p) + s0 : nullptr;
    a.ti_rec = nullptr;
    if (ti_enabled() && std::is_same<T, float>::value && pass == 0 && !plan.wide) {
      c->ti_rec.ensure((size_t)nlist * 64 * sizeof(uint4));
      HIP_CHECK(launch_ti_records(reinterpret_cast<const Ins<float>*>(a.prog), a.list_off, nlist,
                                  (uint32_t)(plan.ntiles * plan.tile * sizeof(T)),
                                  static_cast<uint4*>(c->ti_rec.p), s));
      a.ti_rec = static_cast<const uint4*>(c->ti_rec.p);
    }
    a.nlist = nlist;
    a.X = X;
    a.y = y;
    a.w = w;
    a.n = rows;
    a.n_pad = n_pad;
    a.nfeat = nfeat;
    a.ntiles = plan.ntiles;
    a.ntg = plan.ntg;
    a.tpb = plan.tpb;
    a.nrg = plan.nrg;
    a.loss = loss;
    a.rotate = rotate_enabled() ? 1 : 0;
    a.contig = (pass == -1 && jm && jit_contig()) ? 1 : 0;
    if (pass == -1 && jm && rg_xcd()) a.rotate = rotate_mode();  // tree code: row groups per XCD
    if (pass >= 0 && interp_dyn()) a.rotate |= 4;  // interpreter: trees from an LDS counter
    a.lparam = lparam;
    if (mode == MODE_LOSS && loss >= SRHIP_EXPR_LOSS_BEGIN) a.lprog = expr_loss_device<T>(c, loss);
    c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * sizeof(Part<T>));
    a.partial = static_cast<Part<T>*>(c->partial.p);
    a.out = out;
    a.out_stride = out_stride;
    a.seg = seg;
    a.tgt = tgt;
    a.ntgt = tgt ? ntgt : 0;
    const int tk = timed_begin(c, s);
    if (pass == -1) {
      if constexpr (std::is_same<T, float>::value) {
        // the derived columns of this call, once per row, before the first part
        const jit::Columns& jc = jit::columns(jm);
        const float* dcols = nullptr;
        if (jc.nder > 0) {
          c->derived.ensure((size_t)jc.nder * (size_t)n_pad * sizeof(float));
          if (launches[li].part == 0) HIP_CHECK(jit::launch_derive(jm, X, n_pad, static_cast<float*>(c->derived.p), s));
          dcols = static_cast<const float*>(c->derived.p);
        }
        // the shared subtrees of this call, once per row, before the first part
        // (inside the timed region: their cost is the call's)
        const float* gcols = jc.xg ? X : nullptr;  // wide code reads X itself as its columns
        if (jc.ngcol > 0) {
          if (launches[li].part == 0) shared_cols = shared_columns(c, p, jc, pool, X, rows, n_pad, nfeat);
          gcols = shared_cols;
        }
        HIP_CHECK(jit::launch(jm, launches[li].part, plan, a, jit_fast_enabled(), dcols, s, gcols));
      } else {
        HIP_CHECK(jit::launch64(jm64, launches[li].part, plan, a, s));
      }
    } else {
      // the interpreter's pass after a tree-code pass runs the few trees left
      // over: the call's main kernel stays the tree code
      any_wide = any_wide || plan.wide;
      if (nj == 0) note_kernel(interp_name(sizeof(T), any_wide));
      HIP_CHECK(launch_eval<T>(plan, a, mode, s));
    }
    timed_end(c, s, tk);
    // the last tree-code part's finalize hands over and clears the tree code's counters
    uint32_t* cnt = (last_jit && jm && !jit_bail) ? jit::bail_flags(jm) + nj : nullptr;
    EvalArgs<T> af = a;  // the hand-written tree loops write 4-byte partials
    if constexpr (std::is_same<T, float>::value) af.part4 = (pass == -1 && jit::partials4(jm, launches[li].part)) ? 1 : 0;
    HIP_CHECK(launch_finalize<T>(af, c->res_sum, c->res_ok, s, cnt, cnt ? c->pin_cnt : nullptr));
    if (cnt) c->cnt_pending = true;
    static const bool dbg = env_set("SRHIP_DEBUG_PASSES");
    if (dbg) {  // debugging only: wait for the launch to report its time
      HIP_CHECK(hipStreamSynchronize(s));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, c->tev[2 * (size_t)tk], c->tev[2 * (size_t)tk + 1]));
      std::fprintf(stderr, "srhip pass %s%s: %d trees, %.3f ms (grid %d x %d, %d tiles/wg)\n",
                   pass == -1 ? "tree-code" : pass == 0 ? "shallow" : "deep", plan.wide ? " (wide)" : "", nlist, ms,
                   plan.nrg, plan.ntg, plan.ntiles);
    }
    if (last_jit) rerun_bailed<T>(c, p, jm, a, plan, nfeat, rows, loss, lparam);
  }
  if (mode == MODE_LOSS) c->fail_clean = true;
}

// Copy per-tree results to the caller, applying the static verdicts.
void ensure_pinned(srhip_ctx* c, size_t nt) {
  if (nt <= c->pin_cap) return;
  if (c->pin_sum) (void)hipHostFree(c->pin_sum);
  if (c->pin_ok) (void)hipHostFree(c->pin_ok);
  c->pin_sum = nullptr;
  c->pin_ok = nullptr;
  c->pin_cap = 0;
  // coherent: the finalize kernel may write them directly (zero copy)
  HIP_CHECK(hipHostMalloc((void**)&c->pin_sum, nt * sizeof(double), hipHostMallocCoherent));
  HIP_CHECK(hipHostMalloc((void**)&c->pin_ok, nt, hipHostMallocCoherent));
  c->pin_cap = nt;
}

// the per-tree results to pinned host memory (asynchronous; nothing to copy
// when the finalize wrote them there)
bool enqueue_result_copies(srhip_ctx* c, const srhip_program* p, int64_t rows) {
  const int nt = p->ntrees;
  if (!(rows > 0 && nt > 0 && (p->nlist_a + p->nlist_b) > 0)) return false;
  if (c->res_host) return true;
  HIP_CHECK(hipMemcpyAsync(c->pin_sum, c->sums.p, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipMemcpyAsync(c->pin_ok, c->oks.p, nt, hipMemcpyDeviceToHost, c->stream));
  return true;
}

// wait for the call, then the per-tree results with the static verdicts applied
void finish_results(srhip_ctx* c, const srhip_program* p, int64_t rows, bool copied, double* out_sum,
                    uint8_t* out_ok) {
  wait_stream(c->stream);
  timing_finish(c);
  const int nt = p->ntrees;
  for (int t = 0; t < nt; ++t) {
    bool ok;
    double sm;
    if (p->static_fail[t]) { ok = false; sm = NAN; }
    else if (p->fail_if_rows[t]) { ok = rows == 0; sm = rows == 0 ? 0.0 : NAN; }
    else if (rows == 0 || !copied) { ok = true; sm = 0.0; }
    else { ok = c->pin_ok[t] != 0; sm = c->pin_sum[t]; }
    if (out_sum) out_sum[t] = sm;
    if (out_ok) out_ok[t] = ok ? 1 : 0;
  }
}

// Copy per-tree results to the caller, applying the static verdicts.
void collect_results(srhip_ctx* c, const srhip_program* p, int64_t rows, double* out_sum,
                     uint8_t* out_ok) {
  ensure_pinned(c, std::max(p->ntrees, 1));
  const bool copied = enqueue_result_copies(c, p, rows);
  finish_results(c, p, rows, copied, out_sum, out_ok);
}

template <typename T>
int eval_loss_impl(srhip_dataset* ds, const srhip_program* p, int loss, const double* params,
                   const int64_t* row_idx, int64_t nidx, double* out_sum, double* out_wsum,
                   uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;  // the program's context runs the call (stream, workspace, results)
  const T* X = static_cast<const T*>(ds->X);
  const T* y = static_cast<const T*>(ds->y);
  const T* w = static_cast<const T*>(ds->w);
  int64_t rows = ds->rows, n_pad = ds->n_pad;
  double wsum = ds->w ? ds->sum_w : (double)ds->rows;
  if (row_idx) {
    if (nidx < 0) throw Error(SRHIP_ERR_INVALID, "negative index count");
    for (int64_t k = 0; k < nidx; ++k)
      if (row_idx[k] < 0 || row_idx[k] >= ds->rows) throw Error(SRHIP_ERR_INVALID, "row index out of range");
    const int64_t gp = pad_rows(nidx);
    const size_t es = sizeof(T);
    c->scratch_idx.ensure(std::max<int64_t>(nidx, 1) * sizeof(int64_t));
    c->gather.ensure((size_t)gp * (ds->nfeat + 2) * es);
    T* Xg = static_cast<T*>(c->gather.p);
    T* yg = Xg + (size_t)gp * ds->nfeat;
    T* wg = yg + gp;
    if (nidx > 0) {
      HIP_CHECK(hipMemcpyAsync(c->scratch_idx.p, row_idx, nidx * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
      HIP_CHECK(launch_gather_rows<T>(X, y, w, ds->nfeat, ds->n_pad,
                                      static_cast<const int64_t*>(c->scratch_idx.p), nidx, 0, gp, Xg,
                                      yg, w ? wg : nullptr, c->stream));
    }
    if (w) {  // Σ w over the (repeated) sample
      wsum = 0.0;
      for (int64_t k = 0; k < nidx; ++k) wsum += ds->h_w[row_idx[k]];
    } else {
      wsum = (double)nidx;
    }
    X = Xg;
    y = yg;
    w = w ? wg : nullptr;
    rows = nidx;
    n_pad = gp;
  }
  run_eval<T>(c, p, MODE_LOSS, X, y, w, rows, n_pad, ds->nfeat, loss, params ? params[0] : 0.0, nullptr, 0, 0,
              nullptr, 0, row_idx ? nullptr : ds);
  collect_results(c, p, rows, out_sum, out_ok);
  if (out_wsum) *out_wsum = wsum;
  return SRHIP_OK;
}

// Per-tree row samples (src/LossFunctions.jl:95-115 draws `batch_size` rows with
// replacement per call) gathered into one segment per tree: seg rows, row set t
// in [t·seg, t·seg + bs), padded with its last row. One gathered buffer serves the
// loss (run_eval seg) and the gradient (run_grad) launches.
template <typename T>
struct RowSegs {
  const T* X = nullptr;  // [nfeat][n_pad]
  const T* y = nullptr;  // [n_pad]
  const T* w = nullptr;  // [n_pad] or nullptr
  int64_t seg = 0, n_pad = 0, bs = 0;
};

// the rules of a [nt][bs] row-set argument, answered before any launch
void check_row_sets(const srhip_dataset* ds, int nt, const int64_t* row_idx, int64_t bs) {
  if (bs < 0) throw Error(SRHIP_ERR_INVALID, "negative batch size");
  if (bs > 0 && nt > 0 && !row_idx) throw Error(SRHIP_ERR_INVALID, "row_idx is NULL");
  const int64_t nidx = (int64_t)nt * bs;
  for (int64_t k = 0; k < nidx; ++k)
    if (row_idx[k] < 0 || row_idx[k] >= ds->rows) throw Error(SRHIP_ERR_INVALID, "row index out of range");
}

// Check, upload and gather nt row sets of bs rows into `out` (index scratch
// `idx`; both the context's, or a buffer of the caller's that outlives the call).
// target (srhip_eval_loss_rowsets_targets, checked by the caller): tree t's sample
// takes its y and w from column target[t] of the dataset's target-major y / w
template <typename T>
RowSegs<T> gather_row_sets(srhip_ctx* c, const srhip_dataset* ds, int nt, const int64_t* row_idx, int64_t bs,
                           const int32_t* target, DevBuf& idx, DevBuf& out) {
  check_row_sets(ds, nt, row_idx, bs);
  const int64_t nidx = (int64_t)nt * bs;
  // segment: a power of two >= the row group of any interpreter variant
  // (rows_wg = tiles · 64R is a power of two < 2·bs, or one 512-row tile)
  int64_t seg = 512;
  while (seg < bs && seg < kRowPad) seg *= 2;
  if (seg < bs) seg = pad_rows(bs);
  const T* w = static_cast<const T*>(ds->w);
  const int64_t gp = seg * std::max(nt, 1);
  const size_t es = sizeof(T);
  idx.ensure((size_t)std::max<int64_t>(nidx, 1) * sizeof(int64_t));
  out.ensure((size_t)gp * (ds->nfeat + 2) * es);
  T* Xg = static_cast<T*>(out.p);
  T* yg = Xg + (size_t)gp * ds->nfeat;
  T* wg = yg + gp;
  if (nidx > 0) {
    HIP_CHECK(hipMemcpyAsync(idx.p, row_idx, nidx * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (target) {
      c->tgt.ensure((size_t)nt * sizeof(int32_t));
      HIP_CHECK(hipMemcpyAsync(c->tgt.p, target, (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
      HIP_CHECK(launch_gather_rows_targets<T>(static_cast<const T*>(ds->X), static_cast<const T*>(ds->y), w,
                                              static_cast<const int32_t*>(c->tgt.p), ds->nfeat, ds->n_pad,
                                              static_cast<const int64_t*>(idx.p), bs, seg, gp, Xg, yg,
                                              w ? wg : nullptr, c->stream));
    } else {
      HIP_CHECK(launch_gather_rows<T>(static_cast<const T*>(ds->X), static_cast<const T*>(ds->y), w, ds->nfeat,
                                      ds->n_pad, static_cast<const int64_t*>(idx.p), bs, seg, gp, Xg, yg,
                                      w ? wg : nullptr, c->stream));
    }
  }
  RowSegs<T> rs;
  rs.X = Xg;
  rs.y = yg;
  rs.w = w ? wg : nullptr;
  rs.seg = seg;
  rs.n_pad = gp;
  rs.bs = bs;
  return rs;
}

// Σ w over tree t's (repeated) sample, on the host
void row_set_weight_sums(const srhip_dataset* ds, int nt, const int64_t* row_idx, int64_t bs, const int32_t* target,
                         double* out_wsum) {
  for (int t = 0; t < nt; ++t) {
    double s = 0.0;
    const std::vector<double>& hw = (target && ds->ntargets > 1) ? ds->t_h_w[(size_t)target[t]] : ds->h_w;
    if (ds->w)
      for (int64_t k = 0; k < bs; ++k) s += hw[row_idx[(size_t)t * bs + k]];
    else
      s = (double)bs;
    out_wsum[t] = s;
  }
}

// score_func_batch for every tree of the program on its OWN row sample: the
// interpreter runs one tree per workgroup over its segment (run_eval seg).
// One gather, one evaluation launch and one finalize for all trees.
template <typename T>
int eval_loss_rowsets_impl(srhip_dataset* ds, const srhip_program* p, int loss, const double* params,
                           const int64_t* row_idx, int64_t bs, double* out_sum, double* out_wsum,
                           uint8_t* out_ok, const int32_t* target = nullptr) {
  srhip_ctx* c = p->ctx;
  const RowSegs<T> rs = gather_row_sets<T>(c, ds, p->ntrees, row_idx, bs, target, c->scratch_idx, c->gather);
  run_eval<T>(c, p, MODE_LOSS, rs.X, rs.y, rs.w, bs, rs.n_pad, ds->nfeat, loss, params ? params[0] : 0.0, nullptr, 0,
              rs.seg);
  collect_results(c, p, bs, out_sum, out_ok);  // (the copy of row_idx is ordered before these waits)
  if (out_wsum) row_set_weight_sums(ds, p->ntrees, row_idx, bs, target, out_wsum);
  return SRHIP_OK;
}

// srhip_eval_loss with tree t scored against column target[t] (checked by the
// caller) of a multi-target dataset: one interpreter pass per tree list whose row
// tile holds every column (run_eval tgt). A single-target dataset has one column.
template <typename T>
int eval_loss_targets_impl(srhip_dataset* ds, const srhip_program* p, int loss, const double* params,
                           const int32_t* target, double* out_sum, double* out_wsum, uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  const int nt = p->ntrees;
  c->tgt.ensure((size_t)std::max(nt, 1) * sizeof(int32_t));
  if (nt > 0)
    HIP_CHECK(hipMemcpyAsync(c->tgt.p, target, (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  run_eval<T>(c, p, MODE_LOSS, static_cast<const T*>(ds->X), static_cast<const T*>(ds->y),
              static_cast<const T*>(ds->w), ds->rows, ds->n_pad, ds->nfeat, loss, params ? params[0] : 0.0, nullptr, 0,
              0, static_cast<const int32_t*>(c->tgt.p), ds->ntargets);
  collect_results(c, p, ds->rows, out_sum, out_ok);
  if (out_wsum)
    for (int k = 0; k < ds->ntargets; ++k)
      out_wsum[k] = !ds->w ? (double)ds->rows : (ds->ntargets > 1 ? ds->t_sum_w[(size_t)k] : ds->sum_w);
  return SRHIP_OK;
}

template <typename T>
int eval_loss_packed_impl(srhip_dataset* ds, srhip_program* p, int loss, const double* params, double* d_out) {
  srhip_ctx* c = p->ctx;
  const int nt = p->ntrees;
  const double wsum = ds->w ? ds->sum_w : (double)ds->rows;
  c->want_device_results = true;
  try {
    run_eval<T>(c, p, MODE_LOSS, static_cast<const T*>(ds->X), static_cast<const T*>(ds->y),
                static_cast<const T*>(ds->w), ds->rows, ds->n_pad, ds->nfeat, loss, params ? params[0] : 0.0, nullptr, 0,
                0, nullptr, 0, ds);
  } catch (...) {
    c->want_device_results = false;
    throw;
  }
  c->want_device_results = false;
  if (p->verdict_stale || !p->d_verdict) {
    std::vector<uint8_t> v((size_t)std::max(nt, 1), 0);
    for (int t = 0; t < nt; ++t) v[t] = p->static_fail[t] ? 1 : p->fail_if_rows[t] ? 2 : 0;
    if (!p->d_verdict) HIP_CHECK(hipMalloc((void**)&p->d_verdict, v.size()));
    HIP_CHECK(hipMemcpyAsync(p->d_verdict, v.data(), v.size(), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));  // v leaves scope
    p->verdict_stale = false;
  }
  c->sums.ensure(std::max<size_t>(nt, 1) * sizeof(double));
  c->oks.ensure(std::max<size_t>(nt, 1));
  HIP_CHECK(launch_pack_partials(static_cast<const double*>(c->sums.p), static_cast<const uint8_t*>(c->oks.p),
                                 p->d_verdict, nt, ds->rows, wsum, d_out, c->stream));
  return SRHIP_OK;  // timing_finish once the stream is synchronised (srhip_sync / srhip_last_kernel_time)
}

// Device rows (pitch bytes apart) to the caller's contiguous host rows,
// through the pinned staging halves: the DMA of chunk i overlaps the host
// copy of chunk i-1 (spread over persistent threads). A pageable destination
// otherwise goes through the runtime's own staging, one chunk at a time
// (config #3's 0.82 GB output: 94 ms, profiles/r02j_configs.jsonl).
void copy_rows_to_host(srhip_ctx* c, unsigned char* dst, const unsigned char* src, size_t pitch, size_t row_bytes,
                       int64_t nrows) {
  hipStream_t s = c->stream;
  const int64_t k = std::max<int64_t>(1, (int64_t)((48u << 20) / row_bytes));  // rows per chunk
  const size_t half = (size_t)k * row_bytes;
  if (c->stage_cap < 2 * half) {
    if (c->pin_stage) (void)hipHostFree(c->pin_stage);
    c->pin_stage = nullptr;
    c->stage_cap = 0;
    HIP_CHECK(hipHostMalloc((void**)&c->pin_stage, 2 * half, hipHostMallocDefault));
    c->stage_cap = 2 * half;
  }
  const int64_t nch = (nrows + k - 1) / k;
  while ((int64_t)c->stage_evs.size() < nch) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->stage_evs.push_back(e);
  }
  // host copy threads: SRHIP_COPY_THREADS, default 16 (the CPU share of one
  // GPU on the target hosts; first-touch page faults of the caller's fresh
  // buffer are most of the cost: 0.82 GB in 43 ms on 16 threads, 63 ms on 8,
  // profiles/r03_hostcopy.txt)
  static const unsigned nthr = [] {
    const unsigned want = (unsigned)std::max(1, env_int("SRHIP_COPY_THREADS", 16));
    return std::max(1u, std::min(want, std::max(1u, std::thread::hardware_concurrency())));
  }();
  if (!c->copy_pool) c->copy_pool.reset(new CopyPool());
  c->copy_pool->start(nthr, c->device);
  // workers copy their stripe of each chunk once its DMA has landed; the DMA of
  // chunk i reuses the half of chunk i-2 after every worker is done with it
  std::atomic<int64_t> recorded{-1};
  std::atomic<bool> failed{false};
  std::unique_ptr<std::atomic<unsigned>[]> done(new std::atomic<unsigned>[(size_t)nch]);
  for (int64_t i = 0; i < nch; ++i) done[i].store(0);
  c->copy_pool->submit([&](unsigned j, bool dev_ok) {
    if (!dev_ok) failed = true;
    for (int64_t i = 0; i < nch; ++i) {
      while (recorded.load(std::memory_order_acquire) < i) {
        if (failed.load()) return;
        std::this_thread::yield();
      }
      if (failed.load() || hipEventSynchronize(c->stage_evs[i]) != hipSuccess) { failed = true; return; }
      const int64_t r0 = i * k, nr = std::min(k, nrows - r0);
      const size_t n = (size_t)nr * row_bytes;
      const size_t per = ((n + nthr - 1) / nthr + 63) / 64 * 64;
      const size_t b0 = std::min(n, (size_t)j * per), e0 = std::min(n, b0 + per);
      if (b0 < e0) std::memcpy(dst + (size_t)r0 * row_bytes + b0, c->pin_stage + (size_t)(i & 1) * half + b0, e0 - b0);
      done[i].fetch_add(1, std::memory_order_release);
    }
  });
  try {
    for (int64_t i = 0; i < nch; ++i) {
      if (i >= 2)
        while (done[i - 2].load(std::memory_order_acquire) < nthr) {
          if (failed.load()) throw Error(SRHIP_ERR_DEVICE, "host copy of the per-row outputs failed");
          std::this_thread::yield();
        }
      const int64_t r0 = i * k, nr = std::min(k, nrows - r0);
      HIP_CHECK(hipMemcpy2DAsync(c->pin_stage + (size_t)(i & 1) * half, row_bytes, src + (size_t)r0 * pitch, pitch,
                                 row_bytes, (size_t)nr, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipEventRecord(c->stage_evs[i], s));
      recorded.store(i, std::memory_order_release);
    }
  } catch (...) {
    failed = true;
    c->copy_pool->wait();
    throw;
  }
  c->copy_pool->wait();
  if (failed.load()) throw Error(SRHIP_ERR_DEVICE, "host copy of the per-row outputs failed");
}

template <typename T>
int eval_tree_array_impl(srhip_dataset* ds, const srhip_program* p, void* out, uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  const int nt = p->ntrees;
  const int64_t rows = ds->rows, n_pad = ds->n_pad;
  const size_t es = sizeof(T);
  c->gather.ensure(std::max<size_t>((size_t)nt * n_pad * es, es));
  T* d_out = static_cast<T*>(c->gather.p);
  run_eval<T>(c, p, MODE_OUT, static_cast<const T*>(ds->X), nullptr, nullptr, rows, n_pad,
              ds->nfeat, SRHIP_LOSS_L2, 0.0, d_out, n_pad);
  if (out && rows > 0 && nt > 0) {
    if ((size_t)rows * es * nt < (32u << 20))
      HIP_CHECK(hipMemcpy2DAsync(out, rows * es, d_out, n_pad * es, rows * es, nt, hipMemcpyDeviceToHost, c->stream));
    else
      copy_rows_to_host(c, static_cast<unsigned char*>(out), reinterpret_cast<const unsigned char*>(d_out),
                        (size_t)n_pad * es, (size_t)rows * es, nt);
  }
  collect_results(c, p, rows, nullptr, out_ok);
  if (out) {  // rows of trees that were never run: NaN (reference: undefined)
    T* o = static_cast<T*>(out);
    for (int t = 0; t < nt; ++t)
      if (p->static_fail[t] || p->fail_if_rows[t])
        for (int64_t i = 0; i < rows; ++i) o[(size_t)t * rows + i] = (T)NAN;
  }
  return SRHIP_OK;
}

template <typename T>
void run_grad(srhip_ctx* c, srhip_program* p, int mode, const srhip_dataset* ds, int loss, double lparam,
              T* out_value, T* out_grad, int64_t out_stride, const RowSegs<T>* rs = nullptr,
              const int32_t* tgt = nullptr, int ntgt = 0) {
  // rs (GRAD_LOSS): tree t on its own gathered sample, segment t of rs; the
  // interpreter, one work item per workgroup of one wave, no tree code
  // tgt (GRAD_LOSS, shared rows; device memory, per tree id): a target per tree; y / w
  // are then ntgt columns. The interpreter only (grad_targets_*.hip), no tree code
  build_grad_program<T>(p, rs == nullptr && tgt == nullptr);
  const T* const vX = rs ? rs->X : static_cast<const T*>(ds->X);
  const T* const vy = rs ? rs->y : static_cast<const T*>(ds->y);
  const T* const vw = rs ? rs->w : static_cast<const T*>(ds->w);
  const int64_t vrows = rs ? rs->bs : ds->rows;
  const int64_t vpad = rs ? rs->n_pad : ds->n_pad;
  const int64_t seg = rs ? rs->seg : 0;
  hipStream_t s = c->stream;
  timing_reset(c);
  const int nt = p->ntrees;
  const int nconst = p->const_off.back();
  c->sums.ensure(std::max<size_t>(nt, 1) * sizeof(double));
  c->oks.ensure(std::max<size_t>(nt, 1));
  c->dloss.ensure(std::max<size_t>(nconst, 1) * sizeof(double));
  // gradient tree code (∂L/∂c of the loss) for the trees it holds; the
  // interpreter items of the other trees follow
  bool use_gjit = false;
  if constexpr (std::is_same<T, float>::value) {
    jit::GradModule* gm = (p->gjit && !rs && !tgt && mode == GRAD_LOSS && ds->rows > 0 && wide_mode() != 1)
                              ? grad_module(p, loss, lparam)
                              : nullptr;
    if (gm) {
      const int nparts = jit::grad_nparts(gm);
      const int narr = 1 + ds->nfeat + (ds->w ? 1 : 0);
      std::vector<EvalPlan> plans(nparts);
      use_gjit = true;
      for (int k = 0; k < nparts && use_gjit; ++k) {
        int s0, nsl;
        jit::grad_part(gm, k, &s0, &nsl);
        // partials go straight to global memory: LDS holds the row tiles only (1 byte per slot below
        // keeps plan_geometry's slot bound out of the way)
        use_gjit = plan_geometry(4, 4, kShallowSlots, narr, 1, ds->rows, nsl, &plans[k], gjit_tile_budget()) &&
                   plans[k].nrg == plans[0].nrg;
      }
      if (use_gjit) {
        const int nsl_all = jit::grad_nslots(gm);
        c->fail.ensure((size_t)nsl_all * sizeof(uint32_t));
        c->fail_clean = false;  // the gradient kernels leave their flags set
        HIP_CHECK(hipMemsetAsync(c->fail.p, 0, (size_t)nsl_all * sizeof(uint32_t), s));
        c->gpart.ensure(std::max<size_t>((size_t)plans[0].nrg * nconst, 1) * sizeof(float));
        // the shared subtrees' columns of this call (jit::grad_columns), timed with the call
        const jit::Columns& gcj = jit::grad_columns(gm);
        const float* gcols = nullptr;
        if (gcj.ngcol > 0) {
          const int tk = timed_begin(c, s);
          gcols = percall_columns(c, p->gshared, p->gshared_keys, gcj, static_cast<const float*>(ds->X), ds->rows,
                                  ds->n_pad, ds->nfeat);
          timed_end(c, s, tk);
        }
        for (int k = 0; k < nparts; ++k) {
          int s0, nsl;
          jit::grad_part(gm, k, &s0, &nsl);
          const EvalPlan& plan = plans[k];
          EvalArgs<float> a;
          std::memset(&a, 0, sizeof(a));
          a.list = p->d_gjit_list + s0;
          a.fail = static_cast<uint32_t*>(c->fail.p) + s0;
          a.nlist = nsl;
          a.X = static_cast<const float*>(ds->X);
          a.y = static_cast<const float*>(ds->y);
          a.w = static_cast<const float*>(ds->w);
          a.n = ds->rows;
          a.n_pad = ds->n_pad;
          a.nfeat = ds->nfeat;
          a.ntiles = plan.ntiles;
          a.ntg = plan.ntg;
          a.tpb = plan.tpb;
          a.nrg = plan.nrg;
          a.loss = loss;
          a.contig = jit_contig() ? 1 : 0;
          a.rotate = rotate_mode();
          c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * sizeof(Part<float>));
          a.partial = static_cast<Part<float>*>(c->partial.p);
          const int tk = timed_begin(c, s);
          HIP_CHECK(jit::launch_grad_code(gm, k, plan, a, p->d_gconsts, static_cast<float*>(c->gpart.p), nconst,
                                          s, gcols));
          timed_end(c, s, tk);
          HIP_CHECK(launch_finalize<float>(a, static_cast<double*>(c->sums.p), static_cast<uint8_t*>(c->oks.p), s));
          static const bool dbg = env_set("SRHIP_DEBUG_PASSES");
          if (dbg) {
            HIP_CHECK(hipStreamSynchronize(s));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, c->tev[2 * (size_t)tk], c->tev[2 * (size_t)tk + 1]));
            std::fprintf(stderr, "srhip grad tree code part %d: %d trees, %.3f ms (grid %d x %d, %d tiles/wg)\n", k,
                         nsl, ms, plan.nrg, plan.ntg, plan.ntiles);
          }
        }
        HIP_CHECK(launch_gconst_finalize(static_cast<const float*>(c->gpart.p), plans[0].nrg, nconst,
                                         p->d_gjit_cidx, p->ngjit_cidx, static_cast<double*>(c->dloss.p), s));
      }
    }
  } else if (jit::GradModule64* gm = (p->gjit64 && !rs && !tgt && mode == GRAD_LOSS && ds->rows > 0 && wide_mode() != 1)
                                         ? grad_module64(p, loss, lparam)
                                         : nullptr) {
    // Float64 gradient tree code: 128-row tiles of y, the features it reads, w
    const int nparts = jit::grad64_nparts(gm);
    const int narr = 1 + jit::grad64_nraw(gm) + (ds->w ? 1 : 0);
    if (jit::grad64_nraw(gm) > ds->nfeat) throw Error(SRHIP_ERR_INVALID, "dataset has fewer features than the program reads");
    std::vector<EvalPlan> plans(nparts);
    use_gjit = true;
    for (int k = 0; k < nparts && use_gjit; ++k) {
      int s0, nsl;
      jit::grad64_part(gm, k, &s0, &nsl);
      use_gjit = plan_geometry(8, 2, kShallowSlots, narr, 1, ds->rows, nsl, &plans[k], gjit_tile_budget()) &&
                 plans[k].nrg == plans[0].nrg;
      plans[k].threads = 256;
    }
    if (use_gjit) {
      c->fail.ensure((size_t)jit::grad64_nslots(gm) * sizeof(uint32_t));
      c->fail_clean = false;
      HIP_CHECK(hipMemsetAsync(c->fail.p, 0, (size_t)jit::grad64_nslots(gm) * sizeof(uint32_t), s));
      c->gpart.ensure(std::max<size_t>((size_t)plans[0].nrg * nconst, 1) * sizeof(double));
      for (int k = 0; k < nparts; ++k) {
        int s0, nsl;
        jit::grad64_part(gm, k, &s0, &nsl);
        const EvalPlan& plan = plans[k];
        EvalArgs<double> a;
        std::memset(&a, 0, sizeof(a));
        a.list = p->d_gjit_list + s0;
        a.fail = static_cast<uint32_t*>(c->fail.p) + s0;
        a.nlist = nsl;
        a.X = static_cast<const double*>(ds->X);
        a.y = static_cast<const double*>(ds->y);
        a.w = static_cast<const double*>(ds->w);
        a.n = ds->rows;
        a.n_pad = ds->n_pad;
        a.nfeat = ds->nfeat;
        a.ntiles = plan.ntiles;
        a.ntg = plan.ntg;
        a.tpb = plan.tpb;
        a.nrg = plan.nrg;
        a.loss = loss;
        c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * sizeof(Part<double>));
        a.partial = static_cast<Part<double>*>(c->partial.p);
        const int tk = timed_begin(c, s);
        HIP_CHECK(jit::launch_grad_code64(gm, k, plan, a, p->d_gconsts64, static_cast<double*>(c->gpart.p), nconst, s));
        timed_end(c, s, tk);
        HIP_CHECK(launch_finalize<double>(a, static_cast<double*>(c->sums.p), static_cast<uint8_t*>(c->oks.p), s));
      }
      // gpart is not cleared: a failed tree's row groups stop writing their partials, so its constants'
      // sums here may hold an earlier call's values; collect_grad_results (the only reader of c->dloss)
      // reports NaN for every constant of a failed tree (test_jit64_grad_gpu.py
      // test_failed_trees_gradients_are_nan_not_stale)
      HIP_CHECK(launch_gconst_finalize(static_cast<const double*>(c->gpart.p), plans[0].nrg, nconst,
                                       p->d_gjit_cidx, p->ngjit_cidx, static_cast<double*>(c->dloss.p), s));
    }
  }
  c->last_jit_trees = use_gjit ? (int)p->h_gjl.size() : 0;
  const int* ngi = use_gjit ? p->ngitems_rest : p->ngitems;
  int first = 0;
  if (use_gjit)
    for (int k = 0; k < 4; ++k) first += p->ngitems[k];
  for (int pass = 0; pass < 4; ++pass) {
    const int nitems = ngi[pass];
    const int item0 = first;
    first += nitems;
    if (nitems == 0 || vrows == 0) continue;
    const bool deep = pass == 3;
    int G = pass == 0 ? 1 : pass == 1 ? 2 : kGradG;
    EvalPlan plan;
    const int wm = wide_mode();
    const int ncol = tgt ? ntgt : 0;  // columns of y (and of w) in the row tile
    if (wm == 1 || !plan_grad(p->dtype, deep, G, mode, vw != nullptr, ds->nfeat, vrows, nitems, &plan, ncol)) {
      // the wide variant: one configuration, kGradG tangents (a tree's tangents past its constants stay 0)
      G = kGradG;
      if (wm == 0 || !plan_grad_wide(p->dtype, mode, vw != nullptr, vrows, nitems, &plan, ncol)) throw_lds(ds->nfeat);
    }
    if (seg > 0) {
      // per-tree row sets: the tiles and row groups of a dataset of vrows rows (the
      // per-item arithmetic is that dataset's), one item per workgroup of one wave
      // staging its tree's segment (grad_kernels.hip seg0); the segment holds the row groups
      plan.lds_bytes -= (size_t)(plan.tpb - 1) * (2 + G) * sizeof(T);
      plan.tpb = 1;
      plan.ntg = nitems;
      plan.threads = 64;
      if ((int64_t)plan.nrg * plan.rows_wg > seg) throw Error(SRHIP_ERR_INVALID, "row set segment too short");
    }
    GradArgs<T> a;
    a.prog = static_cast<const Ins<T>*>(p->d_gcode);
    a.tree_off = p->d_gtree_off;
    a.items = p->d_gitems + item0;
    a.nitems = nitems;
    a.dyn = interp_dyn() ? 1 : 0;
    a.const_off = p->d_const_off;
    a.X = vX;
    a.y = vy;
    a.w = vw;
    a.n = vrows;
    a.n_pad = vpad;
    a.seg = seg;
    a.tgt = tgt;
    a.ntgt = ncol;
    a.nfeat = ds->nfeat;
    a.ntiles = plan.ntiles;
    a.ntg = plan.ntg;
    a.tpb = plan.tpb;
    a.nrg = plan.nrg;
    a.loss = loss;
    a.lparam = lparam;
    if (mode == GRAD_LOSS && loss >= SRHIP_EXPR_LOSS_BEGIN) a.lprog = expr_loss_device<T>(c, loss);
    a.G = G;
    a.opset = (deep || plan.wide) ? (p->g_has_expr ? (int)OPSET_EXPR : (int)OPSET_FULL) : p->g_opset;
    c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * (2 + G) * sizeof(T));
    a.partial = static_cast<T*>(c->partial.p);
    a.out_value = out_value;
    a.out_grad = out_grad;
    a.out_stride = out_stride;
    const int tk = timed_begin(c, s);
    if (seg > 0)
      note_kernel(plan.wide ? (sizeof(T) == 4 ? "grad_kernel_wide_seg<float>" : "grad_kernel_wide_seg<double>")
                            : (sizeof(T) == 4 ? "grad_kernel_seg<float>" : "grad_kernel_seg<double>"));
    else if (tgt)
      note_kernel(plan.wide ? (sizeof(T) == 4 ? "grad_kernel_wide_targets<float>" : "grad_kernel_wide_targets<double>")
                            : (sizeof(T) == 4 ? "grad_kernel_targets<float>" : "grad_kernel_targets<double>"));
    else
      note_kernel(plan.wide ? (sizeof(T) == 4 ? "grad_kernel_wide<float>" : "grad_kernel_wide<double>")
                            : (sizeof(T) == 4 ? "grad_kernel<float>" : "grad_kernel<double>"));
    HIP_CHECK(launch_grad<T>(plan, a, mode, s));
    timed_end(c, s, tk);
    HIP_CHECK(launch_grad_finalize<T>(a, static_cast<double*>(c->sums.p), static_cast<uint8_t*>(c->oks.p),
                                      static_cast<double*>(c->dloss.p), s));
    static const bool dbg = env_set("SRHIP_DEBUG_PASSES");
    if (dbg) {
      HIP_CHECK(hipStreamSynchronize(s));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, c->tev[2 * (size_t)tk], c->tev[2 * (size_t)tk + 1]));
      std::fprintf(stderr, "srhip grad pass %d: %d items, G=%d, R=%d, opset %d, %.3f ms (grid %d x %d, %d tiles/wg)\n",
                   pass, nitems, G, plan.R, a.opset, ms, plan.nrg, plan.ntg, plan.ntiles);
    }
  }
}

// per-tree results of a gradient pass: static verdicts applied
void collect_grad_results(srhip_ctx* c, const srhip_program* p, int64_t rows, double* out_sum,
                          double* out_dloss, uint8_t* out_ok) {
  const int nt = p->ntrees;
  const int nconst = p->const_off.back();
  c->h_sum.assign(nt, 0.0);
  c->h_ok.assign(nt, 1);
  std::vector<double> hd(nconst, 0.0);
  if (rows > 0 && nt > 0 && (p->ngitems[0] + p->ngitems[1] + p->ngitems[2] + p->ngitems[3]) > 0) {
    HIP_CHECK(hipMemcpyAsync(c->h_sum.data(), c->sums.p, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(c->h_ok.data(), c->oks.p, nt, hipMemcpyDeviceToHost, c->stream));
    if (nconst > 0)
      HIP_CHECK(hipMemcpyAsync(hd.data(), c->dloss.p, nconst * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_CHECK(hipStreamSynchronize(c->stream));
  timing_finish(c);
  for (int t = 0; t < nt; ++t) {
    const bool fail = p->g_static_fail[t] || (rows > 0 && !c->h_ok[t]);
    if (out_ok) out_ok[t] = fail ? 0 : 1;
    if (out_sum) out_sum[t] = fail ? NAN : (rows > 0 ? c->h_sum[t] : 0.0);
    for (int k = p->const_off[t]; k < p->const_off[t + 1]; ++k)
      if (out_dloss) out_dloss[k] = fail ? NAN : (rows > 0 ? hd[k] : 0.0);
  }
}

template <typename T>
int eval_loss_grad_impl(srhip_dataset* ds, srhip_program* p, int loss, const double* params,
                        double* out_sum, double* out_dloss, double* out_wsum, uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  run_grad<T>(c, p, GRAD_LOSS, ds, loss, params ? params[0] : 0.0, nullptr, nullptr, 0);
  if (out_wsum) *out_wsum = ds->w ? ds->sum_w : (double)ds->rows;
  const bool periodic = std::is_same<T, float>::value && loss == SRHIP_LOSS_PERIODIC && c->last_jit_trees > 0;
  if (!periodic) {
    collect_grad_results(c, p, ds->rows, out_sum, out_dloss, out_ok);
    return SRHIP_OK;
  }
  // Float32 Periodic as gradient tree code: a row beyond the Cody-Waite range made its tree fail
  // there (device_ops.h periodic_g_f32); every failed tree of the call is evaluated again in the
  // forward-mode interpreter (a program of those trees, no tree code), whose results replace the
  // tree code's — failing trees fail there too, the others get OCML's full-range sin / cos
  const int nt = p->ntrees, nconst = p->const_off.back();
  std::vector<double> sum(nt), dl(std::max(nconst, 1));
  std::vector<uint8_t> ok(nt);
  collect_grad_results(c, p, ds->rows, sum.data(), dl.data(), ok.data());
  std::vector<int32_t> redo;
  for (int t = 0; t < nt; ++t)
    if (!ok[t] && !p->g_static_fail[t]) redo.push_back(t);
  if (!redo.empty()) {
    const double ms = c->last_ms;
    const int nl = c->last_launches;
    const int ljt = c->last_jit_trees;  // the call's tree code (the rerun below reports none)
    const char* lkn = t_last_kernel;  // string literals only
    std::vector<int32_t> noff{0}, coff{0};
    std::vector<uint8_t> kind;
    std::vector<uint16_t> arg;
    std::vector<T> cs;
    const T* pc = reinterpret_cast<const T*>(p->consts.data());
    for (int32_t t : redo) {
      kind.insert(kind.end(), p->kind.begin() + p->node_off[t], p->kind.begin() + p->node_off[t + 1]);
      arg.insert(arg.end(), p->arg.begin() + p->node_off[t], p->arg.begin() + p->node_off[t + 1]);
      noff.push_back((int32_t)kind.size());
      cs.insert(cs.end(), pc + p->const_off[t], pc + p->const_off[t + 1]);
      coff.push_back((int32_t)cs.size());
    }
    // the program of those trees, built here (the caller holds the context's lock)
    auto* q = new srhip_program();
    q->ctx = c;
    q->dtype = p->dtype;
    q->ntrees = (int)redo.size();
    q->jit_allowed = false;
    q->gjit_allowed = false;
    q->node_off = noff;
    q->const_off = coff;
    q->kind = kind;
    q->arg = arg;
    q->consts.resize(std::max<size_t>(cs.size() * sizeof(T), 1));
    if (!cs.empty()) std::memcpy(q->consts.data(), cs.data(), cs.size() * sizeof(T));
    std::vector<double> s2(redo.size()), d2(std::max<size_t>(cs.size(), 1));
    std::vector<uint8_t> ok2(redo.size());
    try {
      build_program<T>(q);
      eval_loss_grad_impl<T>(ds, q, loss, params, s2.data(), d2.data(), nullptr, ok2.data());
    } catch (...) {
      (void)hipStreamSynchronize(c->stream);
      free_program_device(q);
      delete q;
      throw;
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
    free_program_device(q);
    delete q;
    for (size_t i = 0; i < redo.size(); ++i) {
      const int32_t t = redo[i];
      sum[t] = s2[i];
      ok[t] = ok2[i];
      for (int32_t k = p->const_off[t]; k < p->const_off[t + 1]; ++k) dl[k] = d2[coff[i] + (k - p->const_off[t])];
    }
    c->last_ms += ms;  // the call's kernel time: both runs
    c->last_launches += nl;
    c->last_jit_trees = ljt;
    t_last_kernel = lkn;
  }
  if (out_sum) std::copy(sum.begin(), sum.end(), out_sum);
  if (out_dloss && nconst > 0) std::copy(dl.begin(), dl.begin() + nconst, out_dloss);
  if (out_ok) std::copy(ok.begin(), ok.end(), out_ok);
  return SRHIP_OK;
}

// srhip_eval_loss_grad with tree t on its own row sample: the samples gathered as
// for srhip_eval_loss_rowsets, then the forward-mode interpreter with one work
// item per workgroup over its tree's segment (run_grad rs). No tree code.
template <typename T>
int eval_loss_grad_rowsets_impl(srhip_dataset* ds, srhip_program* p, int loss, const double* params,
                                const int64_t* row_idx, int64_t bs, double* out_sum, double* out_dloss,
                                double* out_wsum, uint8_t* out_ok, const int32_t* target = nullptr) {
  // target (srhip_eval_loss_grad_rowsets_targets, checked by the caller): the gather takes
  // tree t's y / w rows from column target[t]; the launch is the row-set one
  srhip_ctx* c = p->ctx;
  const RowSegs<T> rs = gather_row_sets<T>(c, ds, p->ntrees, row_idx, bs, target, c->scratch_idx, c->gather);
  run_grad<T>(c, p, GRAD_LOSS, ds, loss, params ? params[0] : 0.0, nullptr, nullptr, 0, &rs);
  collect_grad_results(c, p, bs, out_sum, out_dloss, out_ok);
  if (out_wsum) row_set_weight_sums(ds, p->ntrees, row_idx, bs, target, out_wsum);
  return SRHIP_OK;
}

// srhip_eval_loss_grad with tree t scored against column target[t] (checked by the
// caller) of a multi-target dataset: the forward-mode interpreter with a row tile
// of every column (run_grad tgt). No tree code. A single-target dataset has one column.
template <typename T>
int eval_loss_grad_targets_impl(srhip_dataset* ds, srhip_program* p, int loss, const double* params,
                                const int32_t* target, double* out_sum, double* out_dloss, double* out_wsum,
                                uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  const int nt = p->ntrees;
  c->tgt.ensure((size_t)std::max(nt, 1) * sizeof(int32_t));
  if (nt > 0)
    HIP_CHECK(hipMemcpyAsync(c->tgt.p, target, (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  run_grad<T>(c, p, GRAD_LOSS, ds, loss, params ? params[0] : 0.0, nullptr, nullptr, 0, nullptr,
              static_cast<const int32_t*>(c->tgt.p), ds->ntargets);
  collect_grad_results(c, p, ds->rows, out_sum, out_dloss, out_ok);  // (the copy of target is ordered before its wait)
  if (out_wsum)
    for (int k = 0; k < ds->ntargets; ++k)
      out_wsum[k] = !ds->w ? (double)ds->rows : (ds->ntargets > 1 ? ds->t_sum_w[(size_t)k] : ds->sum_w);
  return SRHIP_OK;
}

// srhip_eval_loss_deriv (checked by the caller): the forward-mode interpreter with its
// tangents seeded at feature leaves (grad_kernel.h kGradLossDeriv), one work item per
// (tree, group of kGradG directions) — one per tree, carrying ndir tangents, when
// ndir <= 2 and the tree is shallow. Shallow trees, then deep ones; the wide variant
// where the row tile of every feature and column does not fit in LDS. No tree code.
template <typename T>
int eval_loss_deriv_impl(srhip_dataset* ds, srhip_program* p, int loss, const double* params, const int32_t* dir,
                         int ndir, double* out_sum, double* out_wsum, uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  build_grad_program<T>(p, false);
  hipStream_t s = c->stream;
  timing_reset(c);
  c->last_jit_trees = 0;
  const int nt = p->ntrees, ncol = 1 + ndir;
  const int ngroups = (ndir + kGradG - 1) / kGradG;
  const int64_t rows = ds->rows;
  std::vector<int32_t> hdir((size_t)ngroups * kGradG, -1);  // (no feature index is negative)
  std::copy(dir, dir + ndir, hdir.begin());
  std::vector<int32_t> items;
  int nitems_of[2] = {0, 0};
  for (int cl = 0; cl < 2; ++cl) {
    std::vector<int32_t> ts;
    for (int t = 0; t < nt; ++t)
      if (p->g_class[t] == cl) ts.push_back(t);
    std::stable_sort(ts.begin(), ts.end(), [&](int32_t x, int32_t y) { return p->g_cost[x] > p->g_cost[y]; });
    for (int32_t t : ts)
      for (int gi = 0; gi < ngroups; ++gi) items.push_back((int32_t)(t | (gi << 24)));
    nitems_of[cl] = (int)ts.size() * ngroups;
  }
  c->tgt.ensure(hdir.size() * sizeof(int32_t));
  c->scratch_idx.ensure(std::max<size_t>(items.size(), 1) * sizeof(int32_t));
  c->dloss.ensure(std::max<size_t>((size_t)nt * ncol, 1) * sizeof(double));
  c->oks.ensure(std::max<size_t>(nt, 1));
  double* d_sum = static_cast<double*>(c->dloss.p);
  HIP_CHECK(hipMemcpyAsync(c->tgt.p, hdir.data(), hdir.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (!items.empty())
    HIP_CHECK(hipMemcpyAsync(c->scratch_idx.p, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  int first = 0;
  bool ran = false;
  for (int cl = 0; cl < 2; ++cl) {
    const int nitems = nitems_of[cl], item0 = first;
    first += nitems;
    if (nitems == 0 || rows == 0) continue;
    const bool deep = cl == 1;
    int G = (deep || ndir > 2) ? kGradG : ndir;
    EvalPlan plan;
    const int wm = wide_mode();
    if (wm == 1 || !plan_grad(p->dtype, deep, G, GRAD_LOSS, ds->w != nullptr, ds->nfeat, rows, nitems, &plan, ncol)) {
      G = kGradG;
      if (wm == 0 || !plan_grad_wide(p->dtype, GRAD_LOSS, ds->w != nullptr, rows, nitems, &plan, ncol)) throw_lds(ds->nfeat);
    }
    GradArgs<T> a;
    a.prog = static_cast<const Ins<T>*>(p->d_gcode);
    a.tree_off = p->d_gtree_off;
    a.items = static_cast<const int32_t*>(c->scratch_idx.p) + item0;
    a.nitems = nitems;
    a.dyn = interp_dyn() ? 1 : 0;
    a.const_off = p->d_const_off;
    a.X = static_cast<const T*>(ds->X);
    a.y = static_cast<const T*>(ds->y);
    a.w = static_cast<const T*>(ds->w);
    a.n = rows;
    a.n_pad = ds->n_pad;
    a.ntgt = ncol;
    a.dir = static_cast<const int32_t*>(c->tgt.p);
    a.nfeat = ds->nfeat;
    a.ntiles = plan.ntiles;
    a.ntg = plan.ntg;
    a.tpb = plan.tpb;
    a.nrg = plan.nrg;
    a.loss = loss;
    a.lparam = params ? params[0] : 0.0;
    a.G = G;
    a.opset = OPSET_FULL;
    c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * (2 + G) * sizeof(T));
    a.partial = static_cast<T*>(c->partial.p);
    a.out_value = nullptr;
    a.out_grad = nullptr;
    a.out_stride = 0;
    const int tk = timed_begin(c, s);
    note_kernel(plan.wide ? (sizeof(T) == 4 ? "grad_kernel_wide_deriv<float>" : "grad_kernel_wide_deriv<double>")
                          : (sizeof(T) == 4 ? "grad_kernel_deriv<float>" : "grad_kernel_deriv<double>"));
    HIP_CHECK(launch_grad_deriv<T>(plan, a, s));
    timed_end(c, s, tk);
    HIP_CHECK(launch_grad_deriv_finalize<T>(a, d_sum, static_cast<uint8_t*>(c->oks.p), s));
    note_loss_launch(plan.nrg, plan.ntg, plan.tpb, (unsigned)plan.nrg * (unsigned)plan.ntg, plan.nrg, 1);
    ran = true;
  }
  std::vector<double> hs((size_t)nt * ncol, 0.0);
  c->h_ok.assign(nt, 1);
  if (ran) {
    HIP_CHECK(hipMemcpyAsync(hs.data(), d_sum, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(c->h_ok.data(), c->oks.p, nt, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  timing_finish(c);
  for (int t = 0; t < nt; ++t) {
    const bool fail = p->g_static_fail[t] || (rows > 0 && !c->h_ok[t]);
    if (out_ok) out_ok[t] = fail ? 0 : 1;
    if (out_sum)
      for (int k = 0; k < ncol; ++k) out_sum[(size_t)t * ncol + k] = fail ? NAN : (rows > 0 ? hs[(size_t)t * ncol + k] : 0.0);
  }
  if (out_wsum)
    for (int k = 0; k < ncol; ++k) out_wsum[k] = !ds->w ? (double)rows : ds->t_sum_w[(size_t)k];
  return SRHIP_OK;
}

// The refusal of run_deriv2's planning, made before an optimisation starts: both classes at
// one work item each (the row tile does not depend on the item count).
void check_deriv2_fits(const srhip_dataset* ds, int ndir) {
  if (ds->rows == 0) return;
  for (int cl = 0; cl < 2; ++cl) {
    EvalPlan plan;
    if (wide_mode() == 1 || !plan_grad_deriv2(ds->dtype, cl == 1, ndir, DERIV2_LOSS, ds->w != nullptr, ds->nfeat,
                                              ds->rows, 1, &plan))
      throw Error(SRHIP_ERR_UNSUPPORTED,
                  "constant gradients of a derivative objective have no wide variant in this version: the row tile of " +
                      std::to_string(ds->nfeat) + " features and " + std::to_string(1 + ndir) +
                      " columns does not fit in LDS");
  }
}

// srhip_eval_loss_grad_deriv / srhip_eval_mixed_tree_array (checked by the caller):
// second-order forward mode (grad_deriv2.h), one work item per (tree, direction,
// group of GC constants) — one per direction for a tree without constants, so its loss
// sums are still reported. Shallow trees, then deep ones. Both launches are planned
// before anything is enqueued: a dataset whose row tile does not fit in LDS (the wide
// plan of srhip_eval_loss_deriv) is refused with the outputs untouched. No tree code.
// mode DERIV2_LOSS: out_loss [nt][1 + ndir], out_grad [nconst][1 + ndir] (host);
// DERIV2_OUT: out_deriv [nt][ndir][rows], out_mixed [nconst][ndir][rows] (host, T).
template <typename T>
int run_deriv2(srhip_dataset* ds, srhip_program* p, int mode, int loss, const double* params, const int32_t* dir,
               int ndir, double* out_loss, double* out_grad, double* out_wsum, void* out_deriv, void* out_mixed,
               uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  build_grad_program<T>(p, false);
  hipStream_t s = c->stream;
  const int nt = p->ntrees, ncol = 1 + ndir, nconst = p->const_off.back();
  const int64_t rows = ds->rows, n_pad = ds->n_pad;
  const bool weighted = mode == DERIV2_LOSS && ds->w != nullptr;
  // items and plans of the two classes
  std::vector<int32_t> items;
  int nitems_of[2] = {0, 0}, gc_of[2] = {0, 0};
  EvalPlan plans[2];
  for (int cl = 0; cl < 2; ++cl) {
    int R = 0, GC = 0;
    deriv2_variant(p->dtype, cl == 1, ndir, &R, &GC);
    gc_of[cl] = GC;
    std::vector<int32_t> ts;
    for (int t = 0; t < nt; ++t)
      if (p->g_class[t] == cl) ts.push_back(t);
    std::stable_sort(ts.begin(), ts.end(), [&](int32_t x, int32_t y) { return p->g_cost[x] > p->g_cost[y]; });
    int n = 0;
    for (int32_t t : ts) {
      const int nc = p->const_off[t + 1] - p->const_off[t];
      const int ngroups = std::max(1, (nc + GC - 1) / GC);
      if (ngroups > 256)
        throw Error(SRHIP_ERR_UNSUPPORTED, "a tree of " + std::to_string(nc) + " constants has more than 256 constant groups");
      for (int gi = 0; gi < ngroups; ++gi)
        for (int k = 0; k < ndir; ++k) {
          items.push_back((int32_t)((uint32_t)t | ((uint32_t)gi << 24)));
          items.push_back(k);
          ++n;
        }
    }
    nitems_of[cl] = n;
    if (n == 0 || rows == 0) continue;
    if (wide_mode() == 1 ||
        !plan_grad_deriv2(p->dtype, cl == 1, ndir, mode, weighted, ds->nfeat, rows, n, &plans[cl]))
      throw Error(SRHIP_ERR_UNSUPPORTED,
                  "constant gradients of a derivative objective have no wide variant in this version: the row tile of " +
                      std::to_string(ds->nfeat) + " features and " + std::to_string(ncol) + " columns does not fit in LDS");
  }
  timing_reset(c);
  c->last_jit_trees = 0;
  c->tgt.ensure((size_t)ndir * sizeof(int32_t));
  c->scratch_idx.ensure(std::max<size_t>(items.size(), 1) * sizeof(int32_t));
  c->sums.ensure(std::max<size_t>((size_t)nt * ncol, 1) * sizeof(double));
  c->dloss.ensure(std::max<size_t>((size_t)nconst * ncol, 1) * sizeof(double));
  c->oks.ensure(std::max<size_t>(nt, 1));
  const size_t es = sizeof(T);
  T* d_deriv = nullptr;
  T* d_mixed = nullptr;
  if (mode == DERIV2_OUT) {
    c->gather.ensure(std::max<size_t>((size_t)(nt + nconst) * ndir * n_pad * es, es));
    d_deriv = static_cast<T*>(c->gather.p);
    d_mixed = d_deriv + (size_t)nt * ndir * n_pad;
  }
  HIP_CHECK(hipMemcpyAsync(c->tgt.p, dir, (size_t)ndir * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (!items.empty())
    HIP_CHECK(hipMemcpyAsync(c->scratch_idx.p, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  int first = 0;
  bool ran = false;
  for (int cl = 0; cl < 2; ++cl) {
    const int nitems = nitems_of[cl], item0 = first;
    first += nitems;
    if (nitems == 0 || rows == 0) continue;
    const EvalPlan& plan = plans[cl];
    Deriv2Args<T> a;
    a.prog = static_cast<const Ins<T>*>(p->d_gcode);
    a.tree_off = p->d_gtree_off;
    a.items = static_cast<const int32_t*>(c->scratch_idx.p) + 2 * (size_t)item0;
    a.nitems = nitems;
    a.dyn = interp_dyn() ? 1 : 0;
    a.const_off = p->d_const_off;
    a.dir = static_cast<const int32_t*>(c->tgt.p);
    a.ndir = ndir;
    a.X = static_cast<const T*>(ds->X);
    a.y = static_cast<const T*>(ds->y);
    a.w = weighted ? static_cast<const T*>(ds->w) : nullptr;
    a.n = rows;
    a.n_pad = n_pad;
    a.nfeat = ds->nfeat;
    a.ntiles = plan.ntiles;
    a.ntg = plan.ntg;
    a.tpb = plan.tpb;
    a.nrg = plan.nrg;
    a.loss = loss;
    a.lparam = params ? params[0] : 0.0;
    a.GC = gc_of[cl];
    c->partial.ensure((size_t)plan.nrg * plan.ntg * plan.tpb * (3 + 2 * a.GC) * sizeof(T));
    a.partial = static_cast<T*>(c->partial.p);
    a.out_deriv = d_deriv;
    a.out_mixed = d_mixed;
    a.out_stride = n_pad;
    const int tk = timed_begin(c, s);
    note_kernel(mode == DERIV2_OUT ? (sizeof(T) == 4 ? "grad_kernel_deriv2_out<float>" : "grad_kernel_deriv2_out<double>")
                                   : (sizeof(T) == 4 ? "grad_kernel_deriv2<float>" : "grad_kernel_deriv2<double>"));
    HIP_CHECK(launch_grad_deriv2<T>(plan, a, mode, s));
    timed_end(c, s, tk);
    if (mode == DERIV2_LOSS)
      HIP_CHECK(launch_grad_deriv2_finalize<T>(a, static_cast<double*>(c->sums.p), static_cast<double*>(c->dloss.p),
                                               static_cast<uint8_t*>(c->oks.p), s));
    note_loss_launch(plan.nrg, plan.ntg, plan.tpb, (unsigned)plan.nrg * (unsigned)plan.ntg, plan.nrg, 1);
    ran = true;
  }
  c->h_ok.assign(nt, 1);
  if (mode == DERIV2_OUT) {
    // the per-row mode reports the static verdict only (a tree that fails on some row
    // has NaN or Inf in its rows)
    if (ran) {
      if (out_deriv && nt > 0)
        HIP_CHECK(hipMemcpy2DAsync(out_deriv, rows * es, d_deriv, n_pad * es, rows * es, (size_t)nt * ndir,
                                   hipMemcpyDeviceToHost, s));
      if (out_mixed && nconst > 0)
        HIP_CHECK(hipMemcpy2DAsync(out_mixed, rows * es, d_mixed, n_pad * es, rows * es, (size_t)nconst * ndir,
                                   hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    timing_finish(c);
    for (int t = 0; t < nt; ++t) {
      if (out_ok) out_ok[t] = p->g_static_fail[t] ? 0 : 1;
      if (!p->g_static_fail[t] || rows == 0) continue;
      // a tree that is never run: its rows are NaN
      const T nan = std::numeric_limits<T>::quiet_NaN();
      if (out_deriv) std::fill_n(static_cast<T*>(out_deriv) + (size_t)t * ndir * rows, (size_t)ndir * rows, nan);
      if (out_mixed)
        std::fill_n(static_cast<T*>(out_mixed) + (size_t)p->const_off[t] * ndir * rows,
                    (size_t)(p->const_off[t + 1] - p->const_off[t]) * ndir * rows, nan);
    }
    return SRHIP_OK;
  }
  std::vector<double> hs((size_t)nt * ncol, 0.0), hg((size_t)nconst * ncol, 0.0);
  if (ran) {
    HIP_CHECK(hipMemcpyAsync(hs.data(), c->sums.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (nconst > 0)
      HIP_CHECK(hipMemcpyAsync(hg.data(), c->dloss.p, hg.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(c->h_ok.data(), c->oks.p, nt, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  timing_finish(c);
  for (int t = 0; t < nt; ++t) {
    const bool fail = p->g_static_fail[t] || (rows > 0 && !c->h_ok[t]);
    if (out_ok) out_ok[t] = fail ? 0 : 1;
    for (int k = 0; k < ncol; ++k) {
      if (out_loss) out_loss[(size_t)t * ncol + k] = fail ? NAN : (rows > 0 ? hs[(size_t)t * ncol + k] : 0.0);
      if (out_grad)
        for (int j = p->const_off[t]; j < p->const_off[t + 1]; ++j)
          out_grad[(size_t)j * ncol + k] = fail ? NAN : (rows > 0 ? hg[(size_t)j * ncol + k] : 0.0);
    }
  }
  if (out_wsum)
    for (int k = 0; k < ncol; ++k) out_wsum[k] = !ds->w ? (double)rows : ds->t_sum_w[(size_t)k];
  return SRHIP_OK;
}

template <typename T>
int eval_grad_tree_array_impl(srhip_dataset* ds, srhip_program* p, void* out_value, void* out_grad,
                              uint8_t* out_ok) {
  srhip_ctx* c = p->ctx;
  const int nt = p->ntrees;
  const int nconst = p->const_off.back();
  const int64_t rows = ds->rows, n_pad = ds->n_pad;
  const size_t es = sizeof(T);
  c->gather.ensure(std::max<size_t>((size_t)(nt + nconst) * n_pad * es, es));
  T* d_val = static_cast<T*>(c->gather.p);
  T* d_grad = d_val + (size_t)nt * n_pad;
  run_grad<T>(c, p, GRAD_OUT, ds, SRHIP_LOSS_L2, 0.0, d_val, d_grad, n_pad);
  if (rows > 0) {
    if (out_value && nt > 0)
      HIP_CHECK(hipMemcpy2DAsync(out_value, rows * es, d_val, n_pad * es, rows * es, nt, hipMemcpyDeviceToHost, c->stream));
    if (out_grad && nconst > 0)
      HIP_CHECK(hipMemcpy2DAsync(out_grad, rows * es, d_grad, n_pad * es, rows * es, nconst, hipMemcpyDeviceToHost, c->stream));
  }
  collect_grad_results(c, p, rows, nullptr, nullptr, out_ok);
  return SRHIP_OK;
}

struct OpName {
  const char* name;
  int arity;
  int id;
};
// Julia operator names → ids, including binopmap/unaopmap (src/Options.jl:86-120)
const OpName kOpNames[] = {
    {"+", 2, SRHIP_BOP_ADD}, {"plus", 2, SRHIP_BOP_ADD},
    {"-", 2, SRHIP_BOP_SUB}, {"sub", 2, SRHIP_BOP_SUB},
    {"*", 2, SRHIP_BOP_MUL}, {"mult", 2, SRHIP_BOP_MUL},
    {"/", 2, SRHIP_BOP_DIV}, {"div", 2, SRHIP_BOP_DIV},
    {"^", 2, SRHIP_BOP_POW}, {"pow", 2, SRHIP_BOP_POW}, {"safe_pow", 2, SRHIP_BOP_POW},
    {"greater", 2, SRHIP_BOP_GREATER},
    {"logical_or", 2, SRHIP_BOP_LOGICAL_OR},
    {"logical_and", 2, SRHIP_BOP_LOGICAL_AND},
    {"mod", 2, SRHIP_BOP_MOD},
    {"max", 2, SRHIP_BOP_MAX},
    {"min", 2, SRHIP_BOP_MIN},
    {"neg", 1, SRHIP_UOP_NEG},
    {"square", 1, SRHIP_UOP_SQUARE},
    {"cube", 1, SRHIP_UOP_CUBE},
    {"exp", 1, SRHIP_UOP_EXP},
    {"abs", 1, SRHIP_UOP_ABS},
    {"log", 1, SRHIP_UOP_LOG}, {"safe_log", 1, SRHIP_UOP_LOG},
    {"log2", 1, SRHIP_UOP_LOG2}, {"safe_log2", 1, SRHIP_UOP_LOG2},
    {"log10", 1, SRHIP_UOP_LOG10}, {"safe_log10", 1, SRHIP_UOP_LOG10},
    {"log1p", 1, SRHIP_UOP_LOG1P}, {"safe_log1p", 1, SRHIP_UOP_LOG1P},
    {"sqrt", 1, SRHIP_UOP_SQRT}, {"safe_sqrt", 1, SRHIP_UOP_SQRT},
    {"sin", 1, SRHIP_UOP_SIN},
    {"cos", 1, SRHIP_UOP_COS},
    {"tan", 1, SRHIP_UOP_TAN},
    {"sinh", 1, SRHIP_UOP_SINH},
    {"cosh", 1, SRHIP_UOP_COSH},
    {"tanh", 1, SRHIP_UOP_TANH},
    {"atan", 1, SRHIP_UOP_ATAN},
    {"asinh", 1, SRHIP_UOP_ASINH},
    {"acosh", 1, SRHIP_UOP_ACOSH}, {"safe_acosh", 1, SRHIP_UOP_ACOSH},
    {"atanh", 1, SRHIP_UOP_ATANH_CLIP}, {"atanh_clip", 1, SRHIP_UOP_ATANH_CLIP},
    {"erf", 1, SRHIP_UOP_ERF},
    {"erfc", 1, SRHIP_UOP_ERFC},
    {"gamma", 1, SRHIP_UOP_GAMMA},
    {"relu", 1, SRHIP_UOP_RELU},
    {"round", 1, SRHIP_UOP_ROUND},
    {"floor", 1, SRHIP_UOP_FLOOR},
    {"ceil", 1, SRHIP_UOP_CEIL},
    {"sign", 1, SRHIP_UOP_SIGN},
    {"inv", 1, SRHIP_UOP_INV},
};

// `call` on a program of `trees` that lives for the call; the call's error survives the destroy
template <typename Call>
int32_t with_temp_program(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees, uint32_t flags, Call call) {
  srhip_program* p = nullptr;
  int32_t rc = srhip_program_create_ex(ctx, ds->dtype, trees, flags, &p);
  if (rc != SRHIP_OK) return rc;
  rc = call(p);
  const std::string err = g_last_error;
  srhip_program_destroy(p);
  g_last_error = err;
  return rc;
}

// ---- what the two dataset constructors share ----
void check_dataset_shape(int32_t dtype, int32_t x_layout, int64_t n, int32_t nfeat, int64_t row_begin,
                         int64_t row_end) {
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) throw Error(SRHIP_ERR_UNSUPPORTED, "dtype must be F32 or F64");
  if (x_layout != SRHIP_X_JULIA && x_layout != SRHIP_X_FEATURE_MAJOR) throw Error(SRHIP_ERR_INVALID, "bad X layout");
  if (n < 0 || nfeat <= 0 || nfeat > 65535) throw Error(SRHIP_ERR_INVALID, "bad shape");
  if (row_begin < 0 || row_end < row_begin || row_end > n) throw Error(SRHIP_ERR_INVALID, "bad row range");
}

// Staging of one upload: the raw shard of X, one raw column, the count of
// non-finite X values. Freed on every path (ScopedBuf), the error path included.
struct UploadStage {
  ScopedBuf raw, rawv, bad;
  UploadStage(srhip_ctx* ctx, int64_t rows, int nfeat, size_t es) {
    raw.ensure((size_t)rows * nfeat * es);
    rawv.ensure((size_t)rows * es);
    bad.ensure(sizeof(int));
    HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), ctx->stream));
  }
};

// rows [row_begin, row_begin + rows) of the host's X: raw shard upload, then
// packed / transposed on the device into dX ([nfeat][n_pad])
void upload_x(srhip_ctx* ctx, UploadStage& st, int dtype, int x_layout, const void* X, int64_t n, int nfeat,
              int64_t row_begin, int64_t rows, int64_t n_pad, void* dX) {
  const size_t es = dtype_size(dtype);
  if (x_layout == SRHIP_X_JULIA) {
    HIP_CHECK(hipMemcpyAsync(st.raw.p, static_cast<const char*>(X) + (size_t)row_begin * nfeat * es,
                             (size_t)rows * nfeat * es, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIP_CHECK(hipMemcpy2DAsync(st.raw.p, rows * es, static_cast<const char*>(X) + row_begin * es, n * es, rows * es,
                               nfeat, hipMemcpyHostToDevice, ctx->stream));
  }
  by_dtype(dtype, [&](auto t) {  // (source stride rows: the packed feature-major shard)
    using T = decltype(t);
    HIP_CHECK(launch_pack_x<T>((const T*)st.raw.p, x_layout, rows, rows, nfeat, n_pad, (T*)dX,
                               static_cast<int*>(st.bad.p), ctx->stream));
  });
}

// `rows` values of a host column from src on, padded into dst ([n_pad])
void upload_column(srhip_ctx* ctx, UploadStage& st, int dtype, const void* src, int64_t rows, int64_t n_pad,
                   void* dst) {
  HIP_CHECK(hipMemcpyAsync(st.rawv.p, src, (size_t)rows * dtype_size(dtype), hipMemcpyHostToDevice, ctx->stream));
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    HIP_CHECK(launch_pack_vec<T>((const T*)st.rawv.p, rows, n_pad, (T*)dst, ctx->stream));
  });
}

// waits for the uploads; whether every X value was finite
bool finish_upload(srhip_ctx* ctx, UploadStage& st) {
  int hbad = 0;
  HIP_CHECK(hipMemcpyAsync(&hbad, st.bad.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return hbad == 0;
}

// Σw and Σ y·w over elements [b, e) of the host columns y and w (w may be null),
// in double (src/Dataset.jl:56-60); the weights are appended to hw
void weight_sums(int dtype, const void* y, const void* w, size_t b, size_t e, double* sum_w, double* sum_yw,
                 std::vector<double>& hw) {
  auto at = [&](const void* base, size_t j) {
    return dtype == SRHIP_F32 ? (double)static_cast<const float*>(base)[j] : static_cast<const double*>(base)[j];
  };
  double sw = 0.0, syw = 0.0;
  for (size_t j = b; j < e; ++j) {
    double wi = 1.0;
    if (w) {
      wi = at(w, j);
      hw.push_back(wi);
    }
    sw += wi;
    syw += at(y, j) * wi;
  }
  *sum_w = sw;
  *sum_yw = syw;
}

}  // namespace

extern "C" {

int32_t srhip_version(void) { return SRHIP_ABI_VERSION; }

const char* srhip_last_error(void) { return g_last_error.c_str(); }

int32_t srhip_device_count(int32_t* out_count) {
  return guarded([&] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (out_count) *out_count = n;
    return n > 0 ? SRHIP_OK : set_error(SRHIP_ERR_DEVICE, "no HIP device available");
  });
}

int32_t srhip_open(int32_t device, srhip_ctx** out_ctx) {
  return guarded([&] {
    if (!out_ctx) throw Error(SRHIP_ERR_INVALID, "out_ctx is null");
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw Error(SRHIP_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= n) throw Error(SRHIP_ERR_INVALID, "device index out of range");
    HIP_CHECK(hipSetDevice(device));
    auto* c = new srhip_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->pin_cnt, 2 * sizeof(uint32_t), hipHostMallocCoherent);
    if (e != hipSuccess) {
      delete c;
      throw Error(SRHIP_ERR_DEVICE, std::string("stream/event creation: ") + hipGetErrorString(e));
    }
    *out_ctx = c;
    return SRHIP_OK;
  });
}

int32_t srhip_close(srhip_ctx* ctx) {
  return guarded([&] {
    if (!ctx) return SRHIP_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->copy_pool.reset();  // joins the host-copy workers
    ctx->partial.release();
    ctx->sums.release();
    ctx->oks.release();
    ctx->dloss.release();
    ctx->scratch_idx.release();
    ctx->gather.release();
    ctx->fail.release();
    ctx->ti_rec.release();
    ctx->bail_list.release();
    ctx->bail_fail.release();
    for (auto& e : ctx->ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->tev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->stage_evs)
      if (e) (void)hipEventDestroy(e);
    for (void* h : {(void*)ctx->pin_sum, (void*)ctx->pin_ok, (void*)ctx->pin_cnt, (void*)ctx->pin_stage})
      if (h) (void)hipHostFree(h);
    ctx->gpart.release();
    ctx->derived.release();
    ctx->gderived.release();
    while (!ctx->pooled.empty()) pool_release(ctx->pooled.back());
    ctx->gpartial.release();
    ctx->gsum.release();
    ctx->gok.release();
    ctx->gti.release();
    for (auto& lp : ctx->lprogs)
      if (lp.d) (void)hipFree(lp.d);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return SRHIP_OK;
  });
}

int32_t srhip_op_lookup(const char* name, int32_t* out_arity, int32_t* out_id) {
  return guarded([&] {
    if (!name) throw Error(SRHIP_ERR_INVALID, "null name");
    for (const auto& o : kOpNames) {
      if (std::strcmp(o.name, name) == 0) {
        if (out_arity) *out_arity = o.arity;
        if (out_id) *out_id = o.id;
        return SRHIP_OK;
      }
    }
    throw Error(SRHIP_ERR_UNSUPPORTED, std::string("operator not supported by the engine: ") + name);
  });
}

int32_t srhip_last_kernel_name(char* buf, int32_t len) {
  return guarded([&] {
    if (!buf || len <= 0) throw Error(SRHIP_ERR_INVALID, "null or empty buffer");
    std::snprintf(buf, (size_t)len, "%s", srhip::last_kernel());
    return SRHIP_OK;
  });
}

int32_t srhip_last_loss_launch(int32_t* out6) {
  return guarded([&] {
    if (!out6) throw Error(SRHIP_ERR_INVALID, "null buffer");
    std::copy(srhip::last_loss_launch(), srhip::last_loss_launch() + 6, out6);
    return SRHIP_OK;
  });
}

int32_t srhip_op_eval(int32_t dtype, int32_t arity, int32_t id, double a, double b, double* out) {
  return guarded([&] {
    if (!out) throw Error(SRHIP_ERR_INVALID, "null out");
    if (dtype != SRHIP_F32 && dtype != SRHIP_F64) throw Error(SRHIP_ERR_UNSUPPORTED, "dtype must be F32 or F64");
    if (id >= SRHIP_EXPR_OP_BEGIN) {  // an expression operator: its body with the same routines
      const std::shared_ptr<const ExprOp> e = expr_op_find(id, /*live=*/true);
      if (e->arity != arity) throw Error(SRHIP_ERR_INVALID, "the expression operator has another arity");
      *out = dtype == SRHIP_F32 ? (double)expr_op_eval<float>(*e, (float)a, (float)b) : expr_op_eval<double>(*e, a, b);
      return SRHIP_OK;
    }
    bool known = false;
    for (const auto& o : kOpNames) known = known || (o.arity == arity && o.id == id);
    if (!known) throw Error(SRHIP_ERR_UNSUPPORTED, "unknown operator id for this arity");
    if (dtype == SRHIP_F32) {
      const float x = (float)a, y = (float)b;
      *out = arity == 1 ? (double)host::unop<float>(id, x) : (double)host::binop<float>(id, x, y);
    } else {
      *out = arity == 1 ? host::unop<double>(id, a) : host::binop<double>(id, a, b);
    }
    return SRHIP_OK;
  });
}

int32_t srhip_op_expr_create(int32_t arity, const uint8_t* kind, const uint16_t* arg, int32_t nnodes,
                             const double* consts, int32_t nconsts, int32_t* out_op_id) {
  return guarded([&] {
    if (!out_op_id) throw Error(SRHIP_ERR_INVALID, "null out_op_id");
    *out_op_id = expr_op_create(arity, kind, arg, nnodes, consts, nconsts);
    return SRHIP_OK;
  });
}

int32_t srhip_op_expr_destroy(int32_t op_id) {
  return guarded([&] {
    expr_op_destroy(op_id);
    return SRHIP_OK;
  });
}

int32_t srhip_loss_expr_create(const uint8_t* kind, const uint16_t* arg, int32_t nnodes, const double* consts,
                               int32_t nconsts, int32_t* out_loss_kind) {
  return guarded([&] {
    if (!out_loss_kind) throw Error(SRHIP_ERR_INVALID, "null out_loss_kind");
    std::shared_ptr<const ExprLoss> e = expr_loss_compile(kind, arg, nnodes, consts, nconsts);
    std::lock_guard<std::mutex> lk(g_expr_mu);
    if (g_expr_next == std::numeric_limits<int32_t>::max()) throw Error(SRHIP_ERR_NOMEM, "expression loss handles exhausted");
    const int32_t id = g_expr_next++;
    g_expr.emplace_back(id, std::move(e));
    *out_loss_kind = id;
    return SRHIP_OK;
  });
}

int32_t srhip_loss_expr_destroy(int32_t loss_kind) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(g_expr_mu);
    for (size_t i = 0; i < g_expr.size(); ++i)
      if (g_expr[i].first == loss_kind) {
        g_expr.erase(g_expr.begin() + (std::ptrdiff_t)i);
        return SRHIP_OK;
      }
    throw Error(SRHIP_ERR_INVALID, "loss kind " + std::to_string(loss_kind) + " is not a registered expression loss");
  });
}

int32_t srhip_loss_expr_eval(int32_t loss_kind, int32_t dtype, const void* yhat, const void* y, const void* w,
                             int64_t n, void* out) {
  return guarded([&] {
    if (loss_kind < SRHIP_EXPR_LOSS_BEGIN) throw Error(SRHIP_ERR_INVALID, "not an expression loss kind");
    const std::shared_ptr<const ExprLoss> e = expr_loss_lookup(loss_kind);
    if (dtype != SRHIP_F32 && dtype != SRHIP_F64) throw Error(SRHIP_ERR_UNSUPPORTED, "dtype must be F32 or F64");
    if (n < 0 || (n > 0 && (!yhat || !y || !out))) throw Error(SRHIP_ERR_INVALID, "null array or negative length");
    if (e->uses_w && !w) throw Error(SRHIP_ERR_INVALID, "the expression loss reads the weight (feature 2) but w is NULL");
    by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      expr_loss_eval_host<T>(*e, static_cast<const T*>(yhat), static_cast<const T*>(y), static_cast<const T*>(w), n,
                             static_cast<T*>(out));
    });
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_create(srhip_ctx* ctx, int32_t dtype, int32_t x_layout, const void* X,
                             const void* y, const void* w, int64_t n, int32_t nfeat,
                             int64_t row_begin, int64_t row_end, srhip_dataset** out_ds) {
  return guarded([&] {
    if (!ctx || !out_ds) throw Error(SRHIP_ERR_INVALID, "null ctx or out_ds");
    *out_ds = nullptr;
    check_dataset_shape(dtype, x_layout, n, nfeat, row_begin, row_end);
    if ((row_end > row_begin) && (!X || !y)) throw Error(SRHIP_ERR_INVALID, "null X or y");
    CALL_SCOPE(ctx);
    const size_t es = dtype_size(dtype);
    const int64_t rows = row_end - row_begin;
    const int64_t n_pad = pad_rows(rows);
    auto* ds = new srhip_dataset();
    ds->ctx = ctx;
    ds->dtype = dtype;
    ds->rows = rows;
    ds->nfeat = nfeat;
    ds->n_pad = n_pad;
    try {
      HIP_CHECK(hipMalloc(&ds->X, (size_t)n_pad * nfeat * es));
      HIP_CHECK(hipMalloc(&ds->y, (size_t)n_pad * es));
      if (w) HIP_CHECK(hipMalloc(&ds->w, (size_t)n_pad * es));
      HIP_CHECK(hipMemsetAsync(ds->X, 0, (size_t)n_pad * nfeat * es, ctx->stream));
      HIP_CHECK(hipMemsetAsync(ds->y, 0, (size_t)n_pad * es, ctx->stream));
      if (w) HIP_CHECK(hipMemsetAsync(ds->w, 0, (size_t)n_pad * es, ctx->stream));
      if (rows > 0) {
        UploadStage st(ctx, rows, nfeat, es);
        upload_x(ctx, st, dtype, x_layout, X, n, nfeat, row_begin, rows, n_pad, ds->X);
        upload_column(ctx, st, dtype, static_cast<const char*>(y) + (size_t)row_begin * es, rows, n_pad, ds->y);
        if (w) upload_column(ctx, st, dtype, static_cast<const char*>(w) + (size_t)row_begin * es, rows, n_pad, ds->w);
        ds->x_finite = finish_upload(ctx, st);
      }
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      weight_sums(dtype, y, w, (size_t)row_begin, (size_t)row_end, &ds->sum_w, &ds->sum_yw, ds->h_w);
    } catch (...) {
      if (ds->X) (void)hipFree(ds->X);
      if (ds->y) (void)hipFree(ds->y);
      if (ds->w) (void)hipFree(ds->w);
      delete ds;
      throw;
    }
    *out_ds = ds;
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_destroy(srhip_dataset* ds) {
  return guarded([&] {
    if (!ds) return SRHIP_OK;
    std::lock_guard<std::mutex> lk(ds->ctx->mu);
    (void)hipSetDevice(ds->ctx->device);
    (void)hipStreamSynchronize(ds->ctx->stream);
    pool_release(ds);
    if (ds->mem) {
      ds->mem.reset();  // the last of a multi-target dataset and its views frees the memory
    } else {
      if (ds->X) (void)hipFree(ds->X);
      if (ds->y) (void)hipFree(ds->y);
      if (ds->w) (void)hipFree(ds->w);
    }
    delete ds;
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_info(const srhip_dataset* ds, int64_t* out_rows, int32_t* out_nfeat,
                           double* out_sum_w, double* out_sum_yw, int32_t* out_x_finite) {
  return guarded([&] {
    if (!ds) throw Error(SRHIP_ERR_INVALID, "null dataset");
    if (out_rows) *out_rows = ds->rows;
    if (out_nfeat) *out_nfeat = ds->nfeat;
    if (out_sum_w) *out_sum_w = ds->sum_w;
    if (out_sum_yw) *out_sum_yw = ds->sum_yw;
    if (out_x_finite) *out_x_finite = ds->x_finite ? 1 : 0;
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_create_multi(srhip_ctx* ctx, int32_t dtype, int32_t x_layout, const void* X, const void* Y,
                                   const void* W, int64_t n, int32_t nfeat, int32_t ntargets, int64_t row_begin,
                                   int64_t row_end, srhip_dataset** out_ds) {
  return guarded([&] {
    // the target count and Y are answered first: no context, no device work
    if (ntargets < 1 || ntargets > SRHIP_MAX_TARGETS)
      throw Error(SRHIP_ERR_INVALID, "ntargets must be 1.." + std::to_string(SRHIP_MAX_TARGETS));
    if (!Y) throw Error(SRHIP_ERR_INVALID, "null Y");
    if (!ctx || !out_ds) throw Error(SRHIP_ERR_INVALID, "null ctx or out_ds");
    *out_ds = nullptr;
    check_dataset_shape(dtype, x_layout, n, nfeat, row_begin, row_end);
    if (row_end > row_begin && !X) throw Error(SRHIP_ERR_INVALID, "null X");
    CALL_SCOPE(ctx);
    const size_t es = dtype_size(dtype);
    const int64_t rows = row_end - row_begin;
    const int64_t n_pad = pad_rows(rows);
    const size_t K = (size_t)ntargets;
    std::unique_ptr<srhip_dataset> ds(new srhip_dataset());  // (mem frees the device memory on every path)
    ds->ctx = ctx;
    ds->dtype = dtype;
    ds->rows = rows;
    ds->nfeat = nfeat;
    ds->n_pad = n_pad;
    ds->ntargets = ntargets;
    ds->mem = std::make_shared<MultiMem>();
    MultiMem* m = ds->mem.get();
    m->device = ctx->device;
    HIP_CHECK(hipMalloc(&m->X, (size_t)n_pad * nfeat * es));
    HIP_CHECK(hipMalloc(&m->Y, K * (size_t)n_pad * es));
    if (W) HIP_CHECK(hipMalloc(&m->W, K * (size_t)n_pad * es));
    HIP_CHECK(hipMemsetAsync(m->X, 0, (size_t)n_pad * nfeat * es, ctx->stream));
    HIP_CHECK(hipMemsetAsync(m->Y, 0, K * (size_t)n_pad * es, ctx->stream));
    if (W) HIP_CHECK(hipMemsetAsync(m->W, 0, K * (size_t)n_pad * es, ctx->stream));
    if (rows > 0) {
      UploadStage st(ctx, rows, nfeat, es);
      upload_x(ctx, st, dtype, x_layout, X, n, nfeat, row_begin, rows, n_pad, m->X);
      // column k of Y / W: rows [row_begin, row_end) of the host's row k, padded as a single y is
      const void* blocks[2] = {Y, W};
      void* dsts[2] = {m->Y, m->W};
      for (int b = 0; b < 2; ++b) {
        if (!blocks[b]) continue;
        for (size_t k = 0; k < K; ++k)
          upload_column(ctx, st, dtype, static_cast<const char*>(blocks[b]) + (k * (size_t)n + (size_t)row_begin) * es,
                        rows, n_pad, static_cast<char*>(dsts[b]) + k * (size_t)n_pad * es);
      }
      ds->x_finite = finish_upload(ctx, st);
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // Σw and Σ y·w of every target over the shard
    ds->t_sum_w.assign(K, 0.0);
    ds->t_sum_yw.assign(K, 0.0);
    ds->t_h_w.assign(K, std::vector<double>());
    for (size_t k = 0; k < K; ++k) {
      if (W) ds->t_h_w[k].reserve((size_t)rows);
      weight_sums(dtype, Y, W, k * (size_t)n + (size_t)row_begin, k * (size_t)n + (size_t)row_end, &ds->t_sum_w[k],
                  &ds->t_sum_yw[k], ds->t_h_w[k]);
    }
    ds->X = m->X;
    ds->y = m->Y;
    ds->w = m->W;
    ds->sum_w = ds->t_sum_w[0];
    ds->sum_yw = ds->t_sum_yw[0];
    if (ntargets == 1) ds->h_w = ds->t_h_w[0];  // an ordinary dataset everywhere
    *out_ds = ds.release();
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_targets(const srhip_dataset* ds, int32_t* out_ntargets) {
  return guarded([&] {
    if (!ds || !out_ntargets) throw Error(SRHIP_ERR_INVALID, "null dataset or output");
    *out_ntargets = ds->ntargets;
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_target_info(const srhip_dataset* ds, int32_t k, double* out_sum_w, double* out_sum_yw) {
  return guarded([&] {
    if (!ds) throw Error(SRHIP_ERR_INVALID, "null dataset");
    if (k < 0 || k >= ds->ntargets) throw Error(SRHIP_ERR_INVALID, "target index out of range");
    const bool multi = ds->ntargets > 1;
    if (out_sum_w) *out_sum_w = multi ? ds->t_sum_w[(size_t)k] : ds->sum_w;
    if (out_sum_yw) *out_sum_yw = multi ? ds->t_sum_yw[(size_t)k] : ds->sum_yw;
    return SRHIP_OK;
  });
}

int32_t srhip_dataset_view(srhip_dataset* ds, int32_t k, srhip_dataset** out_view) {
  return guarded([&] {
    if (!ds || !out_view) throw Error(SRHIP_ERR_INVALID, "null dataset or out_view");
    *out_view = nullptr;
    if (!ds->mem) throw Error(SRHIP_ERR_INVALID, "views are taken of datasets made by srhip_dataset_create_multi");
    if (k < 0 || k >= ds->ntargets) throw Error(SRHIP_ERR_INVALID, "target index out of range");
    const size_t col = (size_t)k * (size_t)ds->n_pad * dtype_size(ds->dtype);
    std::unique_ptr<srhip_dataset> v(new srhip_dataset());
    v->ctx = ds->ctx;
    v->dtype = ds->dtype;
    v->rows = ds->rows;
    v->nfeat = ds->nfeat;
    v->n_pad = ds->n_pad;
    v->x_finite = ds->x_finite;
    v->mem = ds->mem;
    v->X = ds->X;
    v->y = static_cast<char*>(ds->y) + col;  // (a view's own column when ds is a view: k = 0)
    v->w = ds->w ? static_cast<char*>(ds->w) + col : nullptr;
    const bool multi = ds->ntargets > 1;
    v->sum_w = multi ? ds->t_sum_w[(size_t)k] : ds->sum_w;
    v->sum_yw = multi ? ds->t_sum_yw[(size_t)k] : ds->sum_yw;
    v->h_w = multi ? ds->t_h_w[(size_t)k] : ds->h_w;
    *out_view = v.release();
    return SRHIP_OK;
  });
}

int32_t srhip_program_create(srhip_ctx* ctx, int32_t dtype, const srhip_trees* trees,
                             srhip_program** out_prog) {
  return srhip_program_create_ex(ctx, dtype, trees, 0u, out_prog);
}

int32_t srhip_program_create_ex(srhip_ctx* ctx, int32_t dtype, const srhip_trees* trees, uint32_t flags,
                                srhip_program** out_prog) {
  return guarded([&] {
    if (!ctx || !trees || !out_prog) throw Error(SRHIP_ERR_INVALID, "null argument");
    *out_prog = nullptr;
    if (dtype != SRHIP_F32 && dtype != SRHIP_F64) throw Error(SRHIP_ERR_UNSUPPORTED, "dtype must be F32 or F64");
    if (trees->ntrees < 0) throw Error(SRHIP_ERR_INVALID, "negative tree count");
    if (flags & ~(SRHIP_PROGRAM_VARYING_CONSTANTS | SRHIP_PROGRAM_INTERPRETED | SRHIP_PROGRAM_WIDE_TREE_CODE))
      throw Error(SRHIP_ERR_INVALID, "unknown program flags");
    const int nt = trees->ntrees;
    auto* p = new srhip_program();
    p->ctx = ctx;
    p->dtype = dtype;
    p->ntrees = nt;
    p->jit_memc = (flags & SRHIP_PROGRAM_VARYING_CONSTANTS) != 0;
    if (flags & SRHIP_PROGRAM_INTERPRETED) p->jit_allowed = false;
    p->wide_tc = (flags & SRHIP_PROGRAM_WIDE_TREE_CODE) != 0 && dtype == SRHIP_F32;
    try {
      if (nt > 0) {
        if (!trees->node_off || !trees->const_off) throw Error(SRHIP_ERR_INVALID, "null offsets");
        const int nn = trees->node_off[nt];
        const int nc = trees->const_off[nt];
        if (trees->node_off[0] != 0 || trees->const_off[0] != 0 || nn < 0 || nc < 0)
          throw Error(SRHIP_ERR_INVALID, "offsets must start at 0");
        for (int t = 0; t < nt; ++t)
          if (trees->node_off[t + 1] < trees->node_off[t] || trees->const_off[t + 1] < trees->const_off[t])
            throw Error(SRHIP_ERR_INVALID, "offsets must be non-decreasing");
        if (nn > 0 && (!trees->kind || !trees->arg)) throw Error(SRHIP_ERR_INVALID, "null node arrays");
        if (nc > 0 && !trees->consts) throw Error(SRHIP_ERR_INVALID, "null constants");
        p->node_off.assign(trees->node_off, trees->node_off + nt + 1);
        p->const_off.assign(trees->const_off, trees->const_off + nt + 1);
        p->kind.assign(trees->kind, trees->kind + nn);
        p->arg.assign(trees->arg, trees->arg + nn);
        const size_t cb = (size_t)nc * dtype_size(dtype);
        p->consts.resize(std::max<size_t>(cb, 1));
        if (cb) std::memcpy(p->consts.data(), trees->consts, cb);
        p->xops = expr_ops_of(*trees);
      } else {
        p->node_off.assign(1, 0);
        p->const_off.assign(1, 0);
        p->consts.resize(1);
      }
      CALL_SCOPE(ctx);
      by_dtype(dtype, [&](auto t) { build_program<decltype(t)>(p); });
    } catch (...) {
      free_program_device(p);
      delete p;
      throw;
    }
    *out_prog = p;
    return SRHIP_OK;
  });
}

int32_t srhip_program_destroy(srhip_program* prog) {
  return guarded([&] {
    if (!prog) return SRHIP_OK;
    std::lock_guard<std::mutex> lk(prog->ctx->mu);
    (void)hipSetDevice(prog->ctx->device);
    (void)hipStreamSynchronize(prog->ctx->stream);
    free_program_device(prog);
    delete prog;
    return SRHIP_OK;
  });
}

int32_t srhip_program_info(const srhip_program* prog, int32_t* out_ntrees, int64_t* out_total_nodes,
                           int32_t* out_nodes) {
  return guarded([&] {
    if (!prog) throw Error(SRHIP_ERR_INVALID, "null program");
    if (out_ntrees) *out_ntrees = prog->ntrees;
    if (out_total_nodes) *out_total_nodes = prog->total_nodes;
    if (out_nodes) std::copy(prog->nodes.begin(), prog->nodes.end(), out_nodes);
    return SRHIP_OK;
  });
}

int32_t srhip_program_set_constants(srhip_program* prog, const void* consts) {
  return guarded([&] {
    if (!prog) throw Error(SRHIP_ERR_INVALID, "null program");
    const size_t cb = (size_t)prog->const_off.back() * dtype_size(prog->dtype);
    if (cb && !consts) throw Error(SRHIP_ERR_INVALID, "null constants");
    if (cb) std::memcpy(prog->consts.data(), consts, cb);
    CALL_SCOPE(prog->ctx);
    by_dtype(prog->dtype, [&](auto t) { update_constants<decltype(t)>(prog); });
    return SRHIP_OK;
  });
}

// A SRHIP_LOSS_* kind and its parameter: UNSUPPORTED beyond the table,
// INVALID without a needed parameter or for LPDistLoss{n} with n not an integer
// of magnitude below 2^31. Of the margin losses only SmoothedL1Hinge (γ > 0) and
// DWDMargin take one (q > 0; a q that is not integral, or not below 2^31, is
// UNSUPPORTED: the reference raises a DomainError for a negative agreement under
// a non-integer power, so the CPU path owns that case).
static void check_loss(int32_t kind, const double* params) {
  if (kind >= SRHIP_EXPR_LOSS_BEGIN) {  // an expression loss: a registered handle, no parameter
    (void)expr_loss_lookup(kind);
    return;
  }
  if (kind < 0 || kind >= SRHIP_NUM_LOSSES) throw Error(SRHIP_ERR_UNSUPPORTED, "unsupported loss");
  if (kind >= SRHIP_MARGIN_LOSS_BEGIN) {
    if (kind != SRHIP_LOSS_SMOOTHEDL1HINGE && kind != SRHIP_LOSS_DWDMARGIN) return;
    if (!params) throw Error(SRHIP_ERR_INVALID, "loss needs a parameter");
    if (!(params[0] > 0.0))
      throw Error(SRHIP_ERR_INVALID, kind == SRHIP_LOSS_DWDMARGIN ? "DWDMarginLoss needs q > 0"
                                                                  : "SmoothedL1HingeLoss needs gamma > 0");
    if (kind == SRHIP_LOSS_DWDMARGIN && !(params[0] == std::trunc(params[0]) && params[0] < 2147483648.0))
      throw Error(SRHIP_ERR_UNSUPPORTED, "DWDMarginLoss with a q that is not an integer below 2^31");
    return;
  }
  const bool needs = kind != SRHIP_LOSS_L2 && kind != SRHIP_LOSS_L1 && kind != SRHIP_LOSS_LOGCOSH &&
                     kind != SRHIP_LOSS_LOGITDIST;
  if (needs && !params) throw Error(SRHIP_ERR_INVALID, "loss needs a parameter");
  if (kind == SRHIP_LOSS_LPINT && !(params[0] == std::trunc(params[0]) && std::fabs(params[0]) < 2147483648.0))
    throw Error(SRHIP_ERR_INVALID, "LPDistLoss{n} (SRHIP_LOSS_LPINT) needs an integer n");
}

int32_t srhip_eval_loss(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                        const double* loss_params, const int64_t* row_idx, int64_t nidx,
                        double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    check_loss(loss_kind, loss_params);
    check_expr_loss_weights(loss_kind, ds->w != nullptr);
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_impl<decltype(t)>(ds, prog, loss_kind, loss_params, row_idx, nidx, out_loss_sum, out_weight_sum, out_ok);
    });
  });
}

int32_t srhip_eval_loss_packed(srhip_dataset* ds, srhip_program* prog, int32_t loss_kind, const double* loss_params,
                               double* d_out) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    if (!d_out) throw Error(SRHIP_ERR_INVALID, "null output");
    check_loss(loss_kind, loss_params);
    check_expr_loss_weights(loss_kind, ds->w != nullptr);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, d_out) != hipSuccess || at.type != hipMemoryTypeDevice)
      throw Error(SRHIP_ERR_INVALID, "d_out is not device memory");
    if (at.device != prog->ctx->device)
      throw Error(SRHIP_ERR_INVALID, "d_out is on device " + std::to_string(at.device) + ", the program on device " +
                                         std::to_string(prog->ctx->device));
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_packed_impl<decltype(t)>(ds, prog, loss_kind, loss_params, d_out);
    });
  });
}

int32_t srhip_eval_loss_batch(srhip_dataset* ds, const srhip_trees* trees, int32_t loss_kind,
                              const double* loss_params, const int64_t* row_idx, int64_t nidx,
                              double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok) {
  if (!ds) return set_error(SRHIP_ERR_INVALID, "null dataset");
  return srhip_eval_loss_batch_ctx(ds->ctx, ds, trees, loss_kind, loss_params, row_idx, nidx, out_loss_sum,
                                   out_weight_sum, out_ok);
}

int32_t srhip_eval_loss_batch_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees, int32_t loss_kind,
                                  const double* loss_params, const int64_t* row_idx, int64_t nidx,
                                  double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok) {
  if (!ds) return set_error(SRHIP_ERR_INVALID, "null dataset");
  if (!ctx) return set_error(SRHIP_ERR_INVALID, "null ctx");
  return with_temp_program(ctx, ds, trees, 0u, [&](srhip_program* p) {
    return srhip_eval_loss(ds, p, loss_kind, loss_params, row_idx, nidx, out_loss_sum, out_weight_sum, out_ok);
  });
}

int32_t srhip_eval_loss_rowsets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                const double* loss_params, const int64_t* row_idx, int64_t batch_size,
                                double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    check_loss(loss_kind, loss_params);
    check_expr_loss_weights(loss_kind, ds->w != nullptr);
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_rowsets_impl<decltype(t)>(ds, prog, loss_kind, loss_params, row_idx, batch_size, out_loss_sum,
                                                 out_weight_sum, out_ok);
    });
  });
}

int32_t srhip_eval_loss_batch_rowsets_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                          int32_t loss_kind, const double* loss_params, const int64_t* row_idx,
                                          int64_t batch_size, double* out_loss_sum, double* out_weight_sum,
                                          uint8_t* out_ok) {
  if (!ds) return set_error(SRHIP_ERR_INVALID, "null dataset");
  // row sets run in the interpreter: no tree code to build
  return with_temp_program(ctx ? ctx : ds->ctx, ds, trees, SRHIP_PROGRAM_INTERPRETED, [&](srhip_program* p) {
    return srhip_eval_loss_rowsets(ds, p, loss_kind, loss_params, row_idx, batch_size, out_loss_sum, out_weight_sum,
                                   out_ok);
  });
}

// the fused calls' own checks: table losses only, every target within the dataset's columns
static void check_targets(const srhip_dataset* ds, int ntrees, int32_t loss_kind, const int32_t* target) {
  if (loss_kind >= SRHIP_EXPR_LOSS_BEGIN)
    throw Error(SRHIP_ERR_UNSUPPORTED, "expression losses are not scored per target in this version: take views");
  if (ntrees > 0 && !target) throw Error(SRHIP_ERR_INVALID, "target is NULL");
  for (int t = 0; t < ntrees; ++t)
    if (target[t] < 0 || target[t] >= ds->ntargets)
      throw Error(SRHIP_ERR_INVALID, "target " + std::to_string(target[t]) + " of tree " + std::to_string(t) +
                                         " is outside 0.." + std::to_string(ds->ntargets - 1));
}

int32_t srhip_eval_loss_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                const double* loss_params, const int32_t* target, double* out_loss_sum,
                                double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_loss(loss_kind, loss_params);
    check_targets(ds, prog->ntrees, loss_kind, target);
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_targets_impl<decltype(t)>(ds, prog, loss_kind, loss_params, target, out_loss_sum, out_weight_sum,
                                                 out_ok);
    });
  });
}

int32_t srhip_eval_loss_batch_targets_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                          int32_t loss_kind, const double* loss_params, const int32_t* target,
                                          double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok) {
  if (!ds) return set_error(SRHIP_ERR_INVALID, "null dataset");
  // the fused call runs in the interpreter: no tree code to build
  return with_temp_program(ctx ? ctx : ds->ctx, ds, trees, SRHIP_PROGRAM_INTERPRETED, [&](srhip_program* p) {
    return srhip_eval_loss_targets(ds, p, loss_kind, loss_params, target, out_loss_sum, out_weight_sum, out_ok);
  });
}

int32_t srhip_eval_loss_rowsets_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                        const double* loss_params, const int32_t* target, const int64_t* row_idx,
                                        int64_t batch_size, double* out_loss_sum, double* out_weight_sum,
                                        uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_loss(loss_kind, loss_params);
    check_targets(ds, prog->ntrees, loss_kind, target);
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_rowsets_impl<decltype(t)>(ds, prog, loss_kind, loss_params, row_idx, batch_size, out_loss_sum,
                                                 out_weight_sum, out_ok, target);
    });
  });
}

int32_t srhip_eval_tree_array(srhip_dataset* ds, const srhip_program* prog, void* out, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_tree_array_impl<decltype(t)>(ds, prog, out, out_ok);
    });
  });
}

int32_t srhip_eval_loss_grad(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                             const double* loss_params, double* out_loss_sum, double* out_dloss,
                             double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    check_loss(loss_kind, loss_params);
    check_expr_loss_weights(loss_kind, ds->w != nullptr);
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);  // gradient programs are built lazily
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_grad_impl<decltype(t)>(ds, p, loss_kind, loss_params, out_loss_sum, out_dloss, out_weight_sum,
                                              out_ok);
    });
  });
}

int32_t srhip_eval_loss_grad_rowsets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                     const double* loss_params, const int64_t* row_idx, int64_t batch_size,
                                     double* out_loss_sum, double* out_dloss, double* out_weight_sum,
                                     uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    check_loss(loss_kind, loss_params);
    check_expr_loss_weights(loss_kind, ds->w != nullptr);
    check_row_sets(ds, prog->ntrees, row_idx, batch_size);  // before the gradient programs are built
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);  // gradient programs are built lazily
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_grad_rowsets_impl<decltype(t)>(ds, p, loss_kind, loss_params, row_idx, batch_size, out_loss_sum,
                                                      out_dloss, out_weight_sum, out_ok);
    });
  });
}

int32_t srhip_eval_loss_grad_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                     const double* loss_params, const int32_t* target, double* out_loss_sum,
                                     double* out_dloss, double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_loss(loss_kind, loss_params);
    check_targets(ds, prog->ntrees, loss_kind, target);
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);  // gradient programs are built lazily
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_grad_targets_impl<decltype(t)>(ds, p, loss_kind, loss_params, target, out_loss_sum, out_dloss,
                                                      out_weight_sum, out_ok);
    });
  });
}

// srhip_eval_loss_deriv's own checks, made before anything is built, launched or written
static void check_direction_list(const srhip_dataset* ds, const int32_t* dir, int32_t ndir) {
  for (int k = 0; k < ndir; ++k) {
    if (dir[k] < 0 || dir[k] >= ds->nfeat)
      throw Error(SRHIP_ERR_INVALID, "direction " + std::to_string(dir[k]) + " is outside 0.." + std::to_string(ds->nfeat - 1));
    for (int j = 0; j < k; ++j)
      if (dir[j] == dir[k]) throw Error(SRHIP_ERR_INVALID, "direction " + std::to_string(dir[k]) + " is repeated");
  }
}

// srhip_eval_mixed_tree_array's: the directions alone (no column is read)
static void check_directions(const srhip_dataset* ds, const srhip_program* prog, const int32_t* dir, int32_t ndir) {
  if (ndir > 0 && !dir) throw Error(SRHIP_ERR_INVALID, "dir is NULL");
  if (ndir < 1 || ndir > 15) throw Error(SRHIP_ERR_INVALID, "ndir must be within 1..15");
  check_direction_list(ds, dir, ndir);
  if (prog->has_expr || !prog->xops.empty())
    throw Error(SRHIP_ERR_UNSUPPORTED, "expression operators are not part of derivative objectives in this version");
}

static void check_deriv(const srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind, const double* loss_params,
                        const int32_t* dir, int32_t ndir) {
  if (ndir > 0 && !dir) throw Error(SRHIP_ERR_INVALID, "dir is NULL");
  if (ndir < 1 || ndir > 15) throw Error(SRHIP_ERR_INVALID, "ndir must be within 1..15");
  if (ds->ntargets != 1 + ndir)
    throw Error(SRHIP_ERR_INVALID, "a derivative objective over " + std::to_string(ndir) + " directions needs a dataset of " +
                                       std::to_string(1 + ndir) + " columns (y, then one per direction); this one has " +
                                       std::to_string(ds->ntargets));
  check_direction_list(ds, dir, ndir);
  if (loss_kind >= SRHIP_MARGIN_LOSS_BEGIN && loss_kind < SRHIP_EXPR_LOSS_BEGIN)
    throw Error(SRHIP_ERR_INVALID, "a margin loss scores a class label, not a derivative");
  check_loss(loss_kind, loss_params);
  if (loss_kind >= SRHIP_EXPR_LOSS_BEGIN)
    throw Error(SRHIP_ERR_UNSUPPORTED, "expression losses are not part of derivative objectives in this version");
  if (prog->has_expr || !prog->xops.empty())
    throw Error(SRHIP_ERR_UNSUPPORTED, "expression operators are not part of derivative objectives in this version");
}

int32_t srhip_eval_loss_deriv(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                              const double* loss_params, const int32_t* dir, int32_t ndir, double* out_loss_sum,
                              double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_deriv(ds, prog, loss_kind, loss_params, dir, ndir);
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);  // gradient programs are built lazily
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_deriv_impl<decltype(t)>(ds, p, loss_kind, loss_params, dir, ndir, out_loss_sum, out_weight_sum,
                                               out_ok);
    });
  });
}

int32_t srhip_eval_loss_deriv_batch_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees, int32_t loss_kind,
                                        const double* loss_params, const int32_t* dir, int32_t ndir,
                                        double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok) {
  if (!ds) return set_error(SRHIP_ERR_INVALID, "null dataset");
  // the fused call runs in the interpreter: no tree code to build
  return with_temp_program(ctx ? ctx : ds->ctx, ds, trees, SRHIP_PROGRAM_INTERPRETED, [&](srhip_program* p) {
    return srhip_eval_loss_deriv(ds, p, loss_kind, loss_params, dir, ndir, out_loss_sum, out_weight_sum, out_ok);
  });
}

int32_t srhip_eval_loss_grad_deriv(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                   const double* loss_params, const int32_t* dir, int32_t ndir, double* out_loss_sum,
                                   double* out_grad_sum, double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_deriv(ds, prog, loss_kind, loss_params, dir, ndir);
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);  // gradient programs are built lazily
    return by_dtype(ds->dtype, [&](auto t) {
      return run_deriv2<decltype(t)>(ds, p, DERIV2_LOSS, loss_kind, loss_params, dir, ndir, out_loss_sum, out_grad_sum,
                                     out_weight_sum, nullptr, nullptr, out_ok);
    });
  });
}

int32_t srhip_eval_loss_grad_deriv_batch_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                             int32_t loss_kind, const double* loss_params, const int32_t* dir,
                                             int32_t ndir, double* out_loss_sum, double* out_grad_sum,
                                             double* out_weight_sum, uint8_t* out_ok) {
  if (!ds) return set_error(SRHIP_ERR_INVALID, "null dataset");
  return with_temp_program(ctx ? ctx : ds->ctx, ds, trees, SRHIP_PROGRAM_INTERPRETED, [&](srhip_program* p) {
    return srhip_eval_loss_grad_deriv(ds, p, loss_kind, loss_params, dir, ndir, out_loss_sum, out_grad_sum,
                                      out_weight_sum, out_ok);
  });
}

int32_t srhip_eval_mixed_tree_array(srhip_dataset* ds, const srhip_program* prog, const int32_t* dir, int32_t ndir,
                                    void* out_deriv, void* out_mixed, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_directions(ds, prog, dir, ndir);
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);
    return by_dtype(ds->dtype, [&](auto t) {
      return run_deriv2<decltype(t)>(ds, p, DERIV2_OUT, SRHIP_LOSS_L2, nullptr, dir, ndir, nullptr, nullptr, nullptr,
                                     out_deriv, out_mixed, out_ok);
    });
  });
}

int32_t srhip_eval_loss_grad_rowsets_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                             const double* loss_params, const int32_t* target,
                                             const int64_t* row_idx, int64_t batch_size, double* out_loss_sum,
                                             double* out_dloss, double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog, true);
    check_loss(loss_kind, loss_params);
    check_targets(ds, prog->ntrees, loss_kind, target);
    check_row_sets(ds, prog->ntrees, row_idx, batch_size);  // before the gradient programs are built
    CALL_SCOPE(prog->ctx);
    auto* p = const_cast<srhip_program*>(prog);  // gradient programs are built lazily
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_loss_grad_rowsets_impl<decltype(t)>(ds, p, loss_kind, loss_params, row_idx, batch_size, out_loss_sum,
                                                      out_dloss, out_weight_sum, out_ok, target);
    });
  });
}

int32_t srhip_eval_grad_tree_array(srhip_dataset* ds, const srhip_program* prog, void* out_value,
                                   void* out_grad, uint8_t* out_ok) {
  return guarded([&] {
    check_program_vs_dataset(ds, prog);
    CALL_SCOPE(prog->ctx);
    return by_dtype(ds->dtype, [&](auto t) {
      return eval_grad_tree_array_impl<decltype(t)>(ds, const_cast<srhip_program*>(prog), out_value, out_grad, out_ok);
    });
  });
}

int32_t srhip_last_kernel_time(const srhip_ctx* ctx, double* out_ms, int32_t* out_launches) {
  return guarded([&] {
    if (!ctx) throw Error(SRHIP_ERR_INVALID, "null ctx");
    flush_pending(const_cast<srhip_ctx*>(ctx));
    if (out_ms) *out_ms = ctx->last_ms;
    if (out_launches) *out_launches = ctx->last_launches;
    return SRHIP_OK;
  });
}

int32_t srhip_sync(srhip_ctx* ctx) {
  return guarded([&] {
    if (!ctx) throw Error(SRHIP_ERR_INVALID, "null ctx");
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SRHIP_OK;
  });
}

}  // extern "C"

int32_t srhip_program_update_stats(const srhip_program* prog, int64_t* out_inplace, int64_t* out_rebuilt) {
  return guarded([&] {
    if (!prog) throw Error(SRHIP_ERR_INVALID, "null program");
    if (out_inplace) *out_inplace = prog->n_inplace;
    if (out_rebuilt) *out_rebuilt = prog->n_rebuild;
    return SRHIP_OK;
  });
}

int32_t srhip_program_grad_jit_info(const srhip_program* prog, int32_t* out_ntrees, int32_t* out_nrejected,
                                    int64_t* out_code_bytes, double* out_ms_codegen, double* out_ms_load) {
  return guarded([&] {
    if (!prog) throw Error(SRHIP_ERR_INVALID, "null program");
    const bool on = prog->gjit != nullptr || prog->gjit64 != nullptr;
    if (out_ntrees) *out_ntrees = on ? prog->gjit_stats.ntrees : 0;
    if (out_nrejected) *out_nrejected = on ? prog->gjit_stats.nrejected : 0;
    if (out_code_bytes) *out_code_bytes = on ? (int64_t)prog->gjit_stats.code_bytes : 0;
    if (out_ms_codegen) *out_ms_codegen = on ? prog->gjit_stats.ms_codegen : 0.0;
    if (out_ms_load) *out_ms_load = on ? prog->gjit_stats.ms_load : 0.0;
    return SRHIP_OK;
  });
}

int32_t srhip_program_pass_info(const srhip_program* prog, int32_t* out_eval, int32_t* out_grad_items,
                                int32_t* out_grad_rest, int32_t* out_grad_opset) {
  return guarded([&] {
    if (!prog) throw Error(SRHIP_ERR_INVALID, "null program");
    if (out_eval) {
      out_eval[0] = prog->nlist_a;
      out_eval[1] = prog->nlist_b;
      out_eval[2] = (prog->jit != nullptr || prog->jit64 != nullptr) ? prog->nlist_j : 0;
      out_eval[3] = prog->opset;
    }
    const bool g = prog->grad_built;  // the counts of an earlier build are stale
    const bool gj = g && (prog->gjit != nullptr || prog->gjit64 != nullptr);
    for (int k = 0; k < 4; ++k) {
      if (out_grad_items) out_grad_items[k] = g ? prog->ngitems[k] : 0;
      if (out_grad_rest) out_grad_rest[k] = gj ? prog->ngitems_rest[k] : 0;
    }
    if (out_grad_opset) *out_grad_opset = g ? prog->g_opset : 0;
    return SRHIP_OK;
  });
}

int32_t srhip_program_jit_info(const srhip_program* prog, int32_t* out_ntrees, int32_t* out_nfast,
                               int64_t* out_code_bytes, double* out_ms_codegen, double* out_ms_load) {
  return guarded([&] {
    if (!prog) throw Error(SRHIP_ERR_INVALID, "null program");
    const bool on = prog->jit != nullptr || prog->jit64 != nullptr;
    if (out_ntrees) *out_ntrees = on ? prog->nlist_j : 0;
    if (out_nfast) *out_nfast = on ? prog->jit_stats.nfast : 0;
    if (out_code_bytes) *out_code_bytes = on ? (int64_t)prog->jit_stats.code_bytes : 0;
    if (out_ms_codegen) *out_ms_codegen = on ? prog->jit_stats.ms_codegen : 0.0;
    if (out_ms_load) *out_ms_load = on ? prog->jit_stats.ms_load : 0.0;
    return SRHIP_OK;
  });
}

int32_t srhip_last_tree_code(const srhip_ctx* ctx, int32_t* out_ntrees) {
  return guarded([&] {
    if (!ctx || !out_ntrees) throw Error(SRHIP_ERR_INVALID, "null argument");
    *out_ntrees = ctx->last_jit_trees;
    return SRHIP_OK;
  });
}

int32_t srhip_column_cache_info(const srhip_ctx* ctx, int64_t* out_derived, int64_t* out_reused,
                                int64_t* out_programs, int32_t* out_nslot) {
  return guarded([&] {
    if (!ctx) throw Error(SRHIP_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(const_cast<srhip_ctx*>(ctx)->mu);
    if (out_derived) *out_derived = ctx->cols_derived;
    if (out_reused) *out_reused = ctx->cols_reused;
    if (out_programs) *out_programs = ctx->derive_programs;
    if (out_nslot) *out_nslot = ctx->slots.nslot();
    return SRHIP_OK;
  });
}

int32_t srhip_program_shared_columns(const srhip_program* prog, char* out_text, int64_t* inout_n) {
  return guarded([&] {
    if (!prog || !inout_n) throw Error(SRHIP_ERR_INVALID, "null argument");
    std::string text;
    if (prog->jit) {
      const jit::Columns& jc = jit::columns(prog->jit);
      for (int g = 0; g < jc.ngcol; ++g) text += std::to_string(jc.slot(g)) + " " + jc.gkey[(size_t)g] + "\n";
    }
    const int64_t cap = *inout_n;
    *inout_n = (int64_t)text.size();
    if (!out_text || cap < (int64_t)text.size() + 1) throw Error(SRHIP_ERR_INVALID, "output buffer too small");
    std::memcpy(out_text, text.c_str(), text.size() + 1);
    return SRHIP_OK;
  });
}

int32_t srhip_last_bailed(const srhip_ctx* ctx, int32_t* out_ntrees, int64_t* out_redone) {
  return guarded([&] {
    if (!ctx || !out_ntrees) throw Error(SRHIP_ERR_INVALID, "null argument");
    flush_pending(const_cast<srhip_ctx*>(ctx));
    *out_ntrees = ctx->last_bailed;
    if (out_redone) *out_redone = ctx->last_redone;
    return SRHIP_OK;
  });
}

namespace {
// the trees a tree compiler is offered: compiled, no expression-operator code, and
// (loss and output code) within the shallow interpreter's slots
template <typename T>
std::vector<int32_t> candidates(const CompiledBatch<T>& cb, bool shallow) {
  std::vector<int32_t> cand;
  for (int t = 0; t < cb.ntrees; ++t)
    if (cb.tree_off[t] >= 0 && (!shallow || cb.need[t] <= kShallowSlots) && !cb.expr[t]) cand.push_back(t);
  return cand;
}

int32_t jit_compile_hook(const srhip_trees* trees, int mode, uint8_t* out_bytes, int64_t* inout_nbytes,
                         char* out_text, int64_t* inout_ntext, int32_t* out_offsets, int64_t* inout_noffsets,
                         int loss = SRHIP_LOSS_L2, double lparam = 0.0, bool out_mode = false, bool notext = false,
                         bool wide = false) {
  return guarded([&] {
    if (!trees || !inout_nbytes || !inout_ntext || !inout_noffsets) throw Error(SRHIP_ERR_INVALID, "null argument");
    if (!jit::available()) throw Error(SRHIP_ERR_UNSUPPORTED, std::string("tree compiler: ") + jit::unavailable_reason());
    std::vector<uint8_t> bytes;
    std::string text;
    std::vector<int32_t> offs;
    if (loss >= SRHIP_EXPR_LOSS_BEGIN) throw Error(SRHIP_ERR_UNSUPPORTED, "no tree code for expression losses");
    // expression operators: live handles only, and their trees have no tree code
    const std::vector<std::shared_ptr<const ExprOp>> xops = expr_ops_of(*trees);
    if (loss < 0 || loss >= SRHIP_NUM_LOSSES) throw Error(SRHIP_ERR_INVALID, "unknown loss");
    uint64_t lbits;
    std::memcpy(&lbits, &lparam, 8);
    if (mode == 2 && !jit::has_dloss_routine(loss))
      throw Error(SRHIP_ERR_UNSUPPORTED, "no gradient tree code for this loss");
    if (mode != 2 && mode != 5 && mode != 6 && !jit::has_loss_routine(loss))
      throw Error(SRHIP_ERR_UNSUPPORTED, "no tree code for this loss");
    if (mode == 5 && !out_mode && loss >= SRHIP_MARGIN_LOSS_BEGIN)  // margin losses: Float32 loss code only
      throw Error(SRHIP_ERR_UNSUPPORTED, "no Float64 tree code for this loss");
    if (mode == 6) {  // Float64 gradient tree code (jit64.cpp GradGen64)
      if (!jit::has_dloss_routine64(loss)) throw Error(SRHIP_ERR_UNSUPPORTED, "no Float64 gradient tree code for this loss");
      CompiledBatch<double> cb = compile_batch<double>(*trees, /*grad=*/true);
      const std::vector<int32_t> coff(trees->const_off, trees->const_off + trees->ntrees + 1);
      jit::compile_grad_only64(cb, coff, candidates(cb, false), &bytes, &text, &offs, loss, lbits);
    } else if (mode == 5) {  // Float64 tree code (jit64.cpp): L2, another loss's tail, or per-row outputs
      CompiledBatch<double> cb = compile_batch<double>(*trees);
      jit::Opts64 o;
      o.out = out_mode;
      o.loss = out_mode ? SRHIP_LOSS_L2 : loss;
      o.lparam = lbits;
      jit::compile_only64(cb, candidates(cb, true), &bytes, &text, &offs, o);
    } else if (mode == 2) {  // gradient tree code
      CompiledBatch<float> cb = compile_batch<float>(*trees, /*grad=*/true);
      const std::vector<int32_t> coff(trees->const_off, trees->const_off + trees->ntrees + 1);
      jit::compile_grad_only(cb, coff, candidates(cb, false), &bytes, &text, &offs, nullptr, loss, lbits);
    } else {
      CompiledBatch<float> cb = compile_batch<float>(*trees);
      jit::Options jo;
      jo.fast = mode == 1 || mode == 4;
      jo.memc = mode == 3 || mode == 4;
      jo.text = !notext;  // no text: the parallel code generation of build()
      jo.loss = loss;
      jo.lparam = lbits;
      jo.out = out_mode;
      jo.xg = wide;
      jit::compile_only(cb, candidates(cb, true), jo, &bytes, &text, &offs, nullptr);
    }
    if ((int64_t)bytes.size() > *inout_nbytes || (int64_t)text.size() + 1 > *inout_ntext ||
        (int64_t)offs.size() > *inout_noffsets) {
      *inout_nbytes = (int64_t)bytes.size();
      *inout_ntext = (int64_t)text.size() + 1;
      *inout_noffsets = (int64_t)offs.size();
      throw Error(SRHIP_ERR_INVALID, "output buffers too small");
    }
    if (out_bytes && !bytes.empty()) std::memcpy(out_bytes, bytes.data(), bytes.size());
    if (out_text) std::memcpy(out_text, text.c_str(), text.size() + 1);
    if (out_offsets && !offs.empty()) std::memcpy(out_offsets, offs.data(), offs.size() * sizeof(int32_t));
    *inout_nbytes = (int64_t)bytes.size();
    *inout_ntext = (int64_t)text.size() + 1;
    *inout_noffsets = (int64_t)offs.size();
    return SRHIP_OK;
  });
}
}  // namespace

int32_t srhip_jit_compile(const srhip_trees* trees, int32_t fast, uint8_t* out_bytes, int64_t* inout_nbytes,
                          char* out_text, int64_t* inout_ntext, int32_t* out_offsets,
                          int64_t* inout_noffsets) {
  // fast: bit 0 the FAST path, bit 1 memory-constant code (mode 3 / 4 below),
  // bit 2 per-row output code, bit 3 Float64 trees (jit64.cpp; the other bits ignored),
  // bit 4 no assembly text, bit 5 wide code (jit::Options::xg; literal loss code only)
  if (fast & 8)  // Float64 trees (bit 2: their per-row output code)
    return jit_compile_hook(trees, 5, out_bytes, inout_nbytes, out_text, inout_ntext, out_offsets, inout_noffsets,
                            SRHIP_LOSS_L2, 0.0, (fast & 4) != 0);
  return jit_compile_hook(trees, (fast & 2) ? ((fast & 1) ? 4 : 3) : ((fast & 1) ? 1 : 0), out_bytes, inout_nbytes,
                          out_text, inout_ntext, out_offsets, inout_noffsets, SRHIP_LOSS_L2, 0.0, (fast & 4) != 0,
                          (fast & 16) != 0, (fast & 32) != 0);
}

int32_t srhip_jit_compile_grad(const srhip_trees* trees, uint8_t* out_bytes, int64_t* inout_nbytes,
                               char* out_text, int64_t* inout_ntext, int32_t* out_offsets,
                               int64_t* inout_noffsets) {
  return jit_compile_hook(trees, 2, out_bytes, inout_nbytes, out_text, inout_ntext, out_offsets, inout_noffsets);
}

int32_t srhip_jit_compile_loss(const srhip_trees* trees, int32_t grad, int32_t fast, int32_t loss, double loss_param,
                               uint8_t* out_bytes, int64_t* inout_nbytes, char* out_text, int64_t* inout_ntext,
                               int32_t* out_offsets, int64_t* inout_noffsets) {
  // fast bit 3: the Float64 tree compiler (jit64.cpp) with this loss's tail, or with grad its gradient code;
  // bit 5: wide loss code (Float32 loss code only)
  return jit_compile_hook(trees, (fast & 8) ? (grad ? 6 : 5) : grad ? 2 : ((fast & 1) ? 1 : 0), out_bytes, inout_nbytes, out_text,
                          inout_ntext, out_offsets, inout_noffsets, loss, loss_param, false, false, (fast & 32) != 0);
}

namespace {
template <typename T>
void constant_map_check(const srhip_trees* trees, bool grad, bool keep, const void* new_consts, int64_t* mismatch,
                        int64_t* recompiled, int32_t* relayout) {
  srhip_program p;  // host state only: patch_image reads the trees and writes the images
  p.ntrees = trees->ntrees;
  p.jit_memc = keep;  // patch_image recompiles with keep_layout for such programs
  const int nt = trees->ntrees;
  p.node_off.assign(trees->node_off, trees->node_off + nt + 1);
  p.const_off.assign(trees->const_off, trees->const_off + nt + 1);
  p.kind.assign(trees->kind, trees->kind + p.node_off[nt]);
  p.arg.assign(trees->arg, trees->arg + p.node_off[nt]);
  const size_t cbytes = (size_t)p.const_off[nt] * sizeof(T);
  p.consts.resize(std::max<size_t>(cbytes, 1));
  if (cbytes) std::memcpy(p.consts.data(), trees->consts, cbytes);
  CompiledBatch<T> cb = compile_batch_par<T>(*trees, grad, keep);
  std::vector<unsigned char> code(reinterpret_cast<const unsigned char*>(cb.code.data()),
                                  reinterpret_cast<const unsigned char*>(cb.code.data() + cb.code.size()));
  std::vector<uint8_t> sfail = cb.static_fail, fir = cb.fail_if_rows;
  std::vector<unsigned char> cprev = p.consts;  // the constants the image was compiled with
  if (cbytes) std::memcpy(p.consts.data(), new_consts, cbytes);
  bool vchg = false;
  *relayout = patch_image<T>(&p, code, cb.tree_off, cb.len, cb.cmap, cb.direct, cb.folds, sfail, grad ? nullptr : &fir,
                             grad, &vchg, cprev, recompiled) ? 0 : 1;
  if (*relayout) return;
  srhip_trees fresh_trees = *trees;
  fresh_trees.consts = new_consts;
  const CompiledBatch<T> fresh = compile_batch_par<T>(fresh_trees, grad, keep);
  const Ins<T>* ins = reinterpret_cast<const Ins<T>*>(code.data());
  *mismatch = 0;
  for (int t = 0; t < nt; ++t) {
    bool bad = sfail[t] != fresh.static_fail[t] || (!grad && fir[t] != fresh.fail_if_rows[t]);
    // a tree that fails statically is never evaluated: its immediates are free
    if (!bad && fresh.tree_off[t] >= 0 && !fresh.static_fail[t] && !fresh.fail_if_rows[t]) {
      bad = cb.tree_off[t] < 0 || cb.len[t] != fresh.len[t] ||
            std::memcmp(ins + cb.tree_off[t], &fresh.code[fresh.tree_off[t]], sizeof(Ins<T>) * fresh.len[t]) != 0;
    }
    if (bad && env_set("SRHIP_DEBUG_CMAP"))
      std::fprintf(stderr, "cmap mismatch tree %d: sfail %d/%d fir %d/%d toff %d/%d len %d/%d\n", t, sfail[t],
                   fresh.static_fail[t], fir[t], fresh.fail_if_rows[t], cb.tree_off[t], fresh.tree_off[t], cb.len[t],
                   fresh.len[t]);
    *mismatch += bad ? 1 : 0;
  }
}
}  // namespace

int32_t srhip_debug_constant_map(const srhip_trees* trees, int32_t dtype, int32_t grad, const void* new_consts,
                                 int64_t* out_mismatch, int64_t* out_recompiled, int32_t* out_relayout) {
  return guarded([&] {
    if (!trees || !out_mismatch || !out_recompiled || !out_relayout) throw Error(SRHIP_ERR_INVALID, "null argument");
    if (trees->ntrees < 0 || (trees->ntrees > 0 && (!trees->node_off || !trees->const_off)))
      throw Error(SRHIP_ERR_INVALID, "bad trees");
    if (trees->ntrees > 0 && trees->const_off[trees->ntrees] > 0 && !new_consts) throw Error(SRHIP_ERR_INVALID, "null constants");
    *out_mismatch = 0;
    *out_recompiled = 0;
    *out_relayout = 0;
    const bool g = (grad & 1) != 0, keep = (grad & 2) != 0;
    const std::vector<std::shared_ptr<const ExprOp>> xops = expr_ops_of(*trees);  // live handles, held for the call
    if (dtype == SRHIP_F32) constant_map_check<float>(trees, g, keep, new_consts, out_mismatch, out_recompiled, out_relayout);
    else if (dtype == SRHIP_F64) constant_map_check<double>(trees, g, keep, new_consts, out_mismatch, out_recompiled, out_relayout);
    else throw Error(SRHIP_ERR_UNSUPPORTED, "dtype must be F32 or F64");
    return SRHIP_OK;
  });
}

// ---- batched constant optimisation (constopt.cpp) ------------------------------
namespace {

void check_rc(int32_t rc) {
  if (rc != SRHIP_OK) throw Error(rc, g_last_error);
}

copt::Problem make_problem(const srhip_trees* trees, int dtype) {
  if (!trees || trees->ntrees < 0 || !trees->const_off || (trees->ntrees > 0 && !trees->node_off))
    throw Error(SRHIP_ERR_INVALID, "null or malformed trees");
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) throw Error(SRHIP_ERR_UNSUPPORTED, "dtype must be F32 or F64");
  copt::Problem pb;
  pb.dtype = dtype;
  pb.const_off.assign(trees->const_off, trees->const_off + trees->ntrees + 1);
  if (pb.const_off[0] != 0) throw Error(SRHIP_ERR_INVALID, "const_off[0] must be 0");
  for (int t = 0; t < trees->ntrees; ++t)
    if (pb.const_off[t + 1] < pb.const_off[t]) throw Error(SRHIP_ERR_INVALID, "const_off must be non-decreasing");
  const size_t nc = (size_t)pb.const_off.back();
  if (nc && !trees->consts) throw Error(SRHIP_ERR_INVALID, "null consts");
  pb.consts.resize(nc);
  for (size_t j = 0; j < nc; ++j)
    pb.consts[j] = dtype == SRHIP_F32 ? (double)static_cast<const float*>(trees->consts)[j]
                                      : static_cast<const double*>(trees->consts)[j];
  return pb;
}

copt::Options make_copt_options(const srhip_constopt_options* o) {
  if (!o) throw Error(SRHIP_ERR_INVALID, "null options");
  copt::Options r;
  r.algorithm = o->algorithm;
  r.iterations = o->iterations;
  r.nrestarts = o->nrestarts;
  r.noise = o->start_noise;
  r.seed = o->seed;
  return r;
}

void write_result(const copt::Result& r, int dtype, void* out_consts, double* out_loss, uint8_t* out_conv,
                  double* out_nev, bool loss_in_t) {
  const size_t nc = r.consts.size(), nt = r.loss.size();
  if (out_consts)
    for (size_t j = 0; j < nc; ++j) {
      if (dtype == SRHIP_F32) static_cast<float*>(out_consts)[j] = (float)r.consts[j];
      else static_cast<double*>(out_consts)[j] = r.consts[j];
    }
  for (size_t t = 0; t < nt; ++t) {
    if (out_loss) {
      double v = r.loss[t];
      if (loss_in_t && dtype == SRHIP_F32) v = (double)(float)v;
      out_loss[t] = v;
    }
    if (out_conv) out_conv[t] = r.converged[t];
    if (out_nev) out_nev[t] = r.num_evals[t];
  }
}

// Where the time of the last srhip_optimize_constants_batch call on this
// thread went (srhip_constopt_profile): program builds, constant uploads,
// loss and gradient calls (wall), the kernels inside them (HIP events).
struct CoptProfile {
  double total = 0, create = 0, set = 0, loss = 0, grad = 0, kernel_ms = 0;
  int64_t ncreate = 0, nloss = 0, ngrad = 0, nrebuilt = 0;
  double jit_codegen_ms = 0, jit_load_ms = 0;  // of the builds (tree code)
  // srhip_optimize_constants_rowsets: the sets' gathers (wall), evaluations run on row segments
  double gather = 0;
  int64_t nseg = 0;
};
thread_local CoptProfile t_copt;
double secs_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The candidates of one evaluation set as a program on the engine (memory-
// constant tree code: constant updates never recompile); loss and ∂L/∂c of
// every member in one call each, finished as the reference's loss (:12-19).
// The members of an evaluation set (input tree indices, with repetition) as a
// batch of their own: the trees' streams and constants copied in member order.
struct MemberTrees {
  std::vector<int32_t> noff{0}, coff{0};
  std::vector<uint8_t> kind;
  std::vector<uint16_t> arg;
  std::vector<unsigned char> cst;
  srhip_trees tr;
  MemberTrees(const srhip_trees* trees, int dt, const std::vector<int32_t>& members) {
    const size_t es = dt == SRHIP_F32 ? 4 : 8;
    for (int32_t t : members) {
      if (t < 0 || t >= trees->ntrees) throw Error(SRHIP_ERR_INVALID, "member out of range");
      const int32_t a = trees->node_off[t], b = trees->node_off[t + 1];
      kind.insert(kind.end(), trees->kind + a, trees->kind + b);
      arg.insert(arg.end(), trees->arg + a, trees->arg + b);
      noff.push_back((int32_t)kind.size());
      const int32_t ca = trees->const_off[t], cb = trees->const_off[t + 1];
      const unsigned char* src = static_cast<const unsigned char*>(trees->consts);
      cst.insert(cst.end(), src + (size_t)ca * es, src + (size_t)cb * es);
      coff.push_back(coff.back() + (cb - ca));
    }
    tr.ntrees = (int32_t)members.size();
    tr.node_off = noff.data();
    tr.kind = kind.data();
    tr.arg = arg.data();
    tr.const_off = coff.data();
    tr.consts = cst.data();
  }
};

struct EngineSet : copt::Set {
  srhip_ctx* ctx;
  srhip_dataset* ds;
  int dtype, loss;
  const double* params;
  srhip_program* prog = nullptr;
  std::vector<int32_t> coff;  // members' constant offsets
  // row sets (srhip_optimize_constants_rowsets): member m is evaluated on the sample
  // of its input tree in every evaluation. The members are fixed for the set's
  // lifetime, so their segments are gathered once, into buffers of the set (the
  // context's scratch belongs to whichever set evaluates next).
  int64_t bs = 0;
  DevBuf seg_idx, seg_rows;
  RowSegs<float> rs32;
  RowSegs<double> rs64;
  RowSegs<float>& segs(float) { return rs32; }
  RowSegs<double>& segs(double) { return rs64; }
  std::vector<double> wsums;  // Σ w over each member's sample
  // a target per tree (srhip_optimize_constants_targets): member m is scored against
  // column target[members[m]] of the dataset in every evaluation, through the fused
  // calls (interpreter only); empty with fused == false: one y, one w
  bool fused = false;
  std::vector<int32_t> mtgt;
  const int32_t* member_targets() const { return fused ? mtgt.data() : nullptr; }
  EngineSet(srhip_ctx* c, srhip_dataset* d, const srhip_trees* trees, int dt, int ls, const double* pr,
            const std::vector<int32_t>& members, const int64_t* row_idx = nullptr, int64_t batch = 0,
            const int32_t* target = nullptr)
      : ctx(c), ds(d), dtype(dt), loss(ls), params(pr), bs(row_idx ? batch : 0), fused(target != nullptr) {
    MemberTrees mt(trees, dt, members);  // (checks the members' range)
    if (fused) {
      mtgt.resize(std::max<size_t>(members.size(), 1), 0);
      for (size_t m = 0; m < members.size(); ++m) mtgt[m] = target[members[m]];
    }
    coff = mt.coff;
    const srhip_trees& tr = mt.tr;
    const auto t0 = std::chrono::steady_clock::now();
    // (row sets run in the interpreter: no tree code to build)
    check_rc(srhip_program_create_ex(
        ctx, dtype, &tr, SRHIP_PROGRAM_VARYING_CONSTANTS | ((bs > 0 || fused) ? SRHIP_PROGRAM_INTERPRETED : 0u),
        &prog));
    t_copt.create += secs_since(t0);
    t_copt.ncreate += 1;
    if (bs > 0) {
      try {
        gather_members(members, row_idx);
      } catch (...) {
        release();
        throw;
      }
    }
    {
      int32_t nt = 0, nf = 0;
      int64_t nb = 0;
      double mc = 0, ml = 0;
      if (srhip_program_jit_info(prog, &nt, &nf, &nb, &mc, &ml) == SRHIP_OK) {
        t_copt.jit_codegen_ms += mc;
        t_copt.jit_load_ms += ml;
      }
    }
  }
  void release() {
    if (prog) (void)srhip_program_destroy(prog);  // (waits for the stream: nothing reads the segments after it)
    prog = nullptr;
    if (seg_idx.p || seg_rows.p) {
      (void)hipSetDevice(ctx->device);
      seg_idx.release();
      seg_rows.release();
    }
  }
  ~EngineSet() override {
    int64_t inplace = 0, rebuilt = 0;
    if (prog && srhip_program_update_stats(prog, &inplace, &rebuilt) == SRHIP_OK) t_copt.nrebuilt += rebuilt;
    release();
  }
  // the members' row sets (row_idx[members[m]], checked by the caller) gathered into the set's buffers
  void gather_members(const std::vector<int32_t>& members, const int64_t* row_idx) {
    const int n = (int)members.size();
    std::vector<int64_t> idx((size_t)n * bs);
    for (int m = 0; m < n; ++m)
      std::copy(row_idx + (size_t)members[m] * bs, row_idx + (size_t)(members[m] + 1) * bs, idx.begin() + (size_t)m * bs);
    wsums.assign(std::max(n, 1), 0.0);
    const auto t0 = std::chrono::steady_clock::now();
    check_program_vs_dataset(ds, prog, fused);
    {
      CALL_SCOPE(ctx);
      by_dtype(dtype, [&](auto t) {
        segs(t) = gather_row_sets<decltype(t)>(ctx, ds, n, idx.data(), bs, member_targets(), seg_idx, seg_rows);
      });
      HIP_CHECK(hipStreamSynchronize(ctx->stream));  // idx leaves scope
    }
    row_set_weight_sums(ds, n, idx.data(), bs, member_targets(), wsums.data());
    t_copt.gather += secs_since(t0);
  }
  // loss (and ∂L/∂c) of every member on its gathered sample
  void eval_segments(bool grad, double* sums, double* dl, uint8_t* ok) {
    check_program_vs_dataset(ds, prog, fused);  // as the public entry points: device, dtype, feature count, finite X
    CALL_SCOPE(ctx);
    const double lp = params ? params[0] : 0.0;
    by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      const RowSegs<T>& rs = segs(t);
      if (grad) run_grad<T>(ctx, prog, GRAD_LOSS, ds, loss, lp, nullptr, nullptr, 0, &rs);
      else run_eval<T>(ctx, prog, MODE_LOSS, rs.X, rs.y, rs.w, bs, rs.n_pad, ds->nfeat, loss, lp, nullptr, 0, rs.seg);
    });
    if (grad) collect_grad_results(ctx, prog, bs, sums, dl, ok);
    else collect_results(ctx, prog, bs, sums, ok);
  }
  void eval(const std::vector<double>& X, bool grad, std::vector<double>& f, std::vector<double>& g) override {
    const int n = (int)coff.size() - 1;
    const size_t nc = (size_t)coff.back();
    if (X.size() != nc) throw Error(SRHIP_ERR_INVALID, "constant count mismatch");
    auto t0 = std::chrono::steady_clock::now();
    if (dtype == SRHIP_F32) {
      std::vector<float> c(nc);
      for (size_t j = 0; j < nc; ++j) c[j] = (float)X[j];
      check_rc(srhip_program_set_constants(prog, c.data()));
    } else {
      check_rc(srhip_program_set_constants(prog, X.data()));
    }
    t_copt.set += secs_since(t0);
    std::vector<double> sums(std::max(n, 1)), dl(std::max<size_t>(nc, 1));
    std::vector<uint8_t> ok(std::max(n, 1));
    double wsum = 0.0;
    std::vector<double> twsum(fused ? std::max(ds->ntargets, 1) : 0);  // Σ w per target
    t0 = std::chrono::steady_clock::now();
    if (bs > 0) {
      eval_segments(grad, sums.data(), dl.data(), ok.data());
      t_copt.nseg += 1;
    } else if (fused && grad) {
      check_rc(srhip_eval_loss_grad_targets(ds, prog, loss, params, mtgt.data(), sums.data(), dl.data(), twsum.data(),
                                            ok.data()));
    } else if (fused) {
      check_rc(srhip_eval_loss_targets(ds, prog, loss, params, mtgt.data(), sums.data(), twsum.data(), ok.data()));
    } else if (grad) {
      check_rc(srhip_eval_loss_grad(ds, prog, loss, params, sums.data(), dl.data(), &wsum, ok.data()));
    } else {
      check_rc(srhip_eval_loss(ds, prog, loss, params, nullptr, 0, sums.data(), &wsum, ok.data()));
    }
    (grad ? t_copt.grad : t_copt.loss) += secs_since(t0);
    (grad ? t_copt.ngrad : t_copt.nloss) += 1;
    {
      double ms = 0.0;
      if (srhip_last_kernel_time(ctx, &ms, nullptr) == SRHIP_OK) t_copt.kernel_ms += ms;
    }
    f.assign(n, 0.0);
    for (int t = 0; t < n; ++t) {
      // (row sets: Σ w of the member's own sample; a target per tree: of the member's target)
      const double ws = bs > 0 ? wsums[t] : fused ? twsum[(size_t)mtgt[t]] : wsum;
      const double v = sums[t] / ws;
      f[t] = (ok[t] && std::isfinite(v)) ? v : INFINITY;
    }
    if (grad) {
      g.assign(nc, 0.0);
      for (int t = 0; t < n; ++t) {
        const double ws = bs > 0 ? wsums[t] : fused ? twsum[(size_t)mtgt[t]] : wsum;
        for (int32_t j = coff[t]; j < coff[t + 1]; ++j) g[j] = ok[t] ? dl[j] / ws : NAN;
      }
    }
  }
};
struct EngineFactory : copt::Factory {
  srhip_ctx* ctx;
  srhip_dataset* ds;
  const srhip_trees* trees;
  int dtype, loss;
  const double* params;
  // srhip_optimize_constants_rowsets: [ntrees][batch_size], input tree t's sample
  const int64_t* row_idx = nullptr;
  int64_t batch_size = 0;
  // srhip_optimize_constants_targets: [ntrees], input tree t's target
  const int32_t* target = nullptr;
  std::unique_ptr<copt::Set> make(const std::vector<int32_t>& members) override {
    return std::unique_ptr<copt::Set>(
        new EngineSet(ctx, ds, trees, dtype, loss, params, members, row_idx, batch_size, target));
  }
};

// the caller's evaluator
struct CallbackSet : copt::Set {
  srhip_constopt_eval_fn fn;
  void* user;
  std::vector<int32_t> members;
  size_t nconst;
  void eval(const std::vector<double>& X, bool grad, std::vector<double>& f, std::vector<double>& g) override {
    if (X.size() != nconst) throw Error(SRHIP_ERR_INVALID, "constant count mismatch");
    f.assign(members.size(), 0.0);
    g.assign(grad ? nconst : 0, 0.0);
    const int32_t rc = fn(user, (int64_t)members.size(), members.data(), X.data(), grad ? 1 : 0, f.data(),
                          grad ? g.data() : nullptr);
    if (rc != 0) throw Error(SRHIP_ERR_INVALID, "constant optimisation: the evaluator callback failed");
  }
};
struct CallbackFactory : copt::Factory {
  srhip_constopt_eval_fn fn;
  void* user;
  const std::vector<int32_t>* const_off;
  std::unique_ptr<copt::Set> make(const std::vector<int32_t>& members) override {
    std::unique_ptr<CallbackSet> s(new CallbackSet());
    s->fn = fn;
    s->user = user;
    s->members = members;
    s->nconst = 0;
    const int nt = (int)const_off->size() - 1;
    for (int32_t t : members) {
      if (t < 0 || t >= nt) throw Error(SRHIP_ERR_INVALID, "member out of range");
      s->nconst += (size_t)((*const_off)[t + 1] - (*const_off)[t]);
    }
    return s;
  }
};

// srhip_optimize_constants_batch, and with row sets (row_idx [ntrees][batch_size]) _rowsets;
// targets: srhip_optimize_constants_targets (target [ntrees], a multi-target dataset allowed)
int32_t optimize_on_engine(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                           const srhip_constopt_options* opts, bool rowsets, const int64_t* row_idx, int64_t batch_size,
                           void* out_consts, double* out_loss, uint8_t* out_converged, double* out_num_evals,
                           bool targets = false, const int32_t* target = nullptr) {
  return guarded([&] {
    if (!ds) throw Error(SRHIP_ERR_INVALID, "null dataset");
    if (!opts) throw Error(SRHIP_ERR_INVALID, "null options");
    if (targets && opts->loss_kind >= SRHIP_EXPR_LOSS_BEGIN)
      throw Error(SRHIP_ERR_UNSUPPORTED, "expression losses are not optimised per target in this version: take views");
    if (targets && batch_size < 0) throw Error(SRHIP_ERR_INVALID, "negative batch size");
    if (ds->ntargets > 1 && !targets)
      throw Error(SRHIP_ERR_INVALID, "dataset has several targets: take a view of one (srhip_dataset_view)");
    check_loss(opts->loss_kind, opts->loss_params);
    check_expr_loss_weights(opts->loss_kind, ds->w != nullptr);
    if (rowsets && batch_size < 1) throw Error(SRHIP_ERR_INVALID, "batch_size must be at least 1");
    t_copt = CoptProfile();
    const auto t0 = std::chrono::steady_clock::now();
    copt::Problem pb = make_problem(trees, ds->dtype);
    static const int32_t no_trees = 0;  // (an empty batch: the sets still run fused)
    if (targets) {
      check_targets(ds, trees->ntrees, opts->loss_kind, target);
      if (!target) target = &no_trees;
    }
    if (rowsets) check_row_sets(ds, trees->ntrees, row_idx, batch_size);
    EngineFactory fac;
    fac.ctx = ctx ? ctx : ds->ctx;
    fac.ds = ds;
    fac.trees = trees;
    fac.dtype = ds->dtype;
    fac.loss = opts->loss_kind;
    fac.params = opts->loss_params;
    fac.row_idx = rowsets ? row_idx : nullptr;
    fac.batch_size = rowsets ? batch_size : 0;
    fac.target = targets ? target : nullptr;
    const copt::Result r = copt::optimize(pb, make_copt_options(opts), fac);
    write_result(r, ds->dtype, out_consts, out_loss, out_converged, out_num_evals, true);
    t_copt.total = secs_since(t0);
    return SRHIP_OK;
  });
}

// srhip_optimize_constants_deriv: the candidates of one evaluation set as an interpreted
// program, scored under a derivative objective. Loss-only phases are one
// srhip_eval_loss_deriv, gradient phases one srhip_eval_loss_grad_deriv; f and g are
// Σ_c coef[c]·sum_c / wsum_c in float64, in channel order.
struct DerivSet : copt::Set {
  srhip_ctx* ctx;
  srhip_dataset* ds;
  int dtype, loss;
  const double* params;
  const int32_t* dir;
  int ndir;
  const double* coef;
  srhip_program* prog = nullptr;
  std::vector<int32_t> coff;
  DerivSet(srhip_ctx* c, srhip_dataset* d, const srhip_trees* trees, int ls, const double* pr, const int32_t* dr,
           int nd, const double* cf, const std::vector<int32_t>& members)
      : ctx(c), ds(d), dtype(d->dtype), loss(ls), params(pr), dir(dr), ndir(nd), coef(cf) {
    MemberTrees mt(trees, dtype, members);
    coff = mt.coff;
    const auto t0 = std::chrono::steady_clock::now();
    check_rc(srhip_program_create_ex(ctx, dtype, &mt.tr, SRHIP_PROGRAM_VARYING_CONSTANTS | SRHIP_PROGRAM_INTERPRETED,
                                     &prog));
    t_copt.create += secs_since(t0);
    t_copt.ncreate += 1;
  }
  ~DerivSet() override {
    int64_t inplace = 0, rebuilt = 0;
    if (prog && srhip_program_update_stats(prog, &inplace, &rebuilt) == SRHIP_OK) t_copt.nrebuilt += rebuilt;
    if (prog) (void)srhip_program_destroy(prog);
  }
  void eval(const std::vector<double>& X, bool grad, std::vector<double>& f, std::vector<double>& g) override {
    const int n = (int)coff.size() - 1, ncol = 1 + ndir;
    const size_t nc = (size_t)coff.back();
    if (X.size() != nc) throw Error(SRHIP_ERR_INVALID, "constant count mismatch");
    auto t0 = std::chrono::steady_clock::now();
    if (dtype == SRHIP_F32) {
      std::vector<float> c(nc);
      for (size_t j = 0; j < nc; ++j) c[j] = (float)X[j];
      check_rc(srhip_program_set_constants(prog, c.data()));
    } else {
      check_rc(srhip_program_set_constants(prog, X.data()));
    }
    t_copt.set += secs_since(t0);
    std::vector<double> sums((size_t)std::max(n, 1) * ncol), gs(std::max<size_t>(nc, 1) * ncol), ws(ncol);
    std::vector<uint8_t> ok(std::max(n, 1));
    t0 = std::chrono::steady_clock::now();
    if (grad)
      check_rc(srhip_eval_loss_grad_deriv(ds, prog, loss, params, dir, ndir, sums.data(), gs.data(), ws.data(), ok.data()));
    else
      check_rc(srhip_eval_loss_deriv(ds, prog, loss, params, dir, ndir, sums.data(), ws.data(), ok.data()));
    (grad ? t_copt.grad : t_copt.loss) += secs_since(t0);
    (grad ? t_copt.ngrad : t_copt.nloss) += 1;
    {
      double ms = 0.0;
      if (srhip_last_kernel_time(ctx, &ms, nullptr) == SRHIP_OK) t_copt.kernel_ms += ms;
    }
    auto combine = [&](const double* row) {
      double v = 0.0;
      for (int c = 0; c < ncol; ++c) v += coef[c] * row[c] / ws[c];
      return v;
    };
    f.assign(n, 0.0);
    for (int t = 0; t < n; ++t) {
      const double v = combine(&sums[(size_t)t * ncol]);
      f[t] = (ok[t] && std::isfinite(v)) ? v : INFINITY;
    }
    if (grad) {
      g.assign(nc, 0.0);
      for (int t = 0; t < n; ++t)
        for (int32_t j = coff[t]; j < coff[t + 1]; ++j) g[j] = ok[t] ? combine(&gs[(size_t)j * ncol]) : NAN;
    }
  }
};
struct DerivFactory : copt::Factory {
  srhip_ctx* ctx;
  srhip_dataset* ds;
  const srhip_trees* trees;
  int loss;
  const double* params;
  const int32_t* dir;
  int ndir;
  const double* coef;
  std::unique_ptr<copt::Set> make(const std::vector<int32_t>& members) override {
    return std::unique_ptr<copt::Set>(new DerivSet(ctx, ds, trees, loss, params, dir, ndir, coef, members));
  }
};

}  // namespace

int32_t srhip_optimize_constants_deriv(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                       const srhip_constopt_options* opts, const int32_t* dir, int32_t ndir,
                                       const double* coef, void* out_consts, double* out_loss, uint8_t* out_converged,
                                       double* out_num_evals) {
  return guarded([&] {
    if (!ds) throw Error(SRHIP_ERR_INVALID, "null dataset");
    if (!opts) throw Error(SRHIP_ERR_INVALID, "null options");
    copt::Problem pb = make_problem(trees, ds->dtype);
    srhip_ctx* c = ctx ? ctx : ds->ctx;
    // srhip_eval_loss_grad_deriv's refusals, on a program of the input trees (never run)
    {
      srhip_program* probe = nullptr;
      check_rc(srhip_program_create_ex(c, ds->dtype, trees, SRHIP_PROGRAM_VARYING_CONSTANTS | SRHIP_PROGRAM_INTERPRETED,
                                       &probe));
      try {
        check_program_vs_dataset(ds, probe, true);
        check_deriv(ds, probe, opts->loss_kind, opts->loss_params, dir, ndir);
        check_deriv2_fits(ds, ndir);
      } catch (...) {
        (void)srhip_program_destroy(probe);
        throw;
      }
      (void)srhip_program_destroy(probe);
    }
    if (!coef) throw Error(SRHIP_ERR_INVALID, "coef is NULL");
    for (int k = 0; k <= ndir; ++k)
      if (!std::isfinite(coef[k])) throw Error(SRHIP_ERR_INVALID, "coefficient " + std::to_string(k) + " is not finite");
    t_copt = CoptProfile();
    const auto t0 = std::chrono::steady_clock::now();
    DerivFactory fac;
    fac.ctx = c;
    fac.ds = ds;
    fac.trees = trees;
    fac.loss = opts->loss_kind;
    fac.params = opts->loss_params;
    fac.dir = dir;
    fac.ndir = ndir;
    fac.coef = coef;
    const copt::Result r = copt::optimize(pb, make_copt_options(opts), fac);
    write_result(r, ds->dtype, out_consts, out_loss, out_converged, out_num_evals, false);
    t_copt.total = secs_since(t0);
    return SRHIP_OK;
  });
}

int32_t srhip_optimize_constants_batch(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                       const srhip_constopt_options* opts, void* out_consts, double* out_loss,
                                       uint8_t* out_converged, double* out_num_evals) {
  return optimize_on_engine(ctx, ds, trees, opts, false, nullptr, 0, out_consts, out_loss, out_converged,
                            out_num_evals);
}

int32_t srhip_optimize_constants_rowsets(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                         const srhip_constopt_options* opts, const int64_t* row_idx,
                                         int64_t batch_size, void* out_consts, double* out_loss,
                                         uint8_t* out_converged, double* out_num_evals) {
  return optimize_on_engine(ctx, ds, trees, opts, true, row_idx, batch_size, out_consts, out_loss, out_converged,
                            out_num_evals);
}

int32_t srhip_optimize_constants_targets(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                         const srhip_constopt_options* opts, const int32_t* target,
                                         const int64_t* row_idx, int64_t batch_size, void* out_consts,
                                         double* out_loss, uint8_t* out_converged, double* out_num_evals) {
  return optimize_on_engine(ctx, ds, trees, opts, row_idx != nullptr, row_idx, batch_size, out_consts, out_loss,
                            out_converged, out_num_evals, true, target);
}

int32_t srhip_constopt_profile(double* out, int32_t n) {
  return guarded([&] {
    if (!out || n < 0) throw Error(SRHIP_ERR_INVALID, "null output");
    const CoptProfile& q = t_copt;
    const double v[14] = {q.total, q.create, q.set, q.loss, q.grad, q.kernel_ms * 1e-3,
                          (double)q.ncreate, (double)q.nloss, (double)q.ngrad, (double)q.nrebuilt,
                          q.jit_codegen_ms * 1e-3, q.jit_load_ms * 1e-3, q.gather, (double)q.nseg};
    for (int32_t i = 0; i < n && i < 14; ++i) out[i] = v[i];
    return SRHIP_OK;
  });
}

int32_t srhip_optimize_constants_cb(const srhip_trees* trees, int32_t dtype, const srhip_constopt_options* opts,
                                    srhip_constopt_eval_fn fn, void* user, void* out_consts, double* out_loss,
                                    uint8_t* out_converged, double* out_num_evals) {
  return guarded([&] {
    if (!fn) throw Error(SRHIP_ERR_INVALID, "null evaluator");
    copt::Problem pb = make_problem(trees, dtype);
    CallbackFactory fac;
    fac.fn = fn;
    fac.user = user;
    fac.const_off = &pb.const_off;
    const copt::Result r = copt::optimize(pb, make_copt_options(opts), fac);
    write_result(r, dtype, out_consts, out_loss, out_converged, out_num_evals, false);
    return SRHIP_OK;
  });
}

// ---- device groups (srhip.h "device groups") ----------------------------------------
// One process, several contexts: member k is a context on devices[k] with a
// persistent driver thread that does the member's hipSetDevice, host planning
// and enqueues. A group call is handed to every driver; each member leaves its
// row shard's packed partials in slot k of a pinned host buffer every device
// maps, member 0's stream waits for the others' events and one combine kernel
// adds the slots in member order. DESIGN.md §5 "Device groups".
namespace {

constexpr int kMaxGroup = 16;

// The driver thread of one member: runs the jobs posted to it, one at a time.
class Driver {
 public:
  Driver() : th_([this] { loop(); }) {}
  ~Driver() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  void post(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = std::move(f);
      has_ = true;
    }
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return !has_; });
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || has_; });
      if (!has_) return;  // stop_
      std::function<void()> f = std::move(job_);
      lk.unlock();
      f();
      lk.lock();
      has_ = false;
      cv_done_.notify_all();
    }
  }
  std::mutex m_;
  std::condition_variable cv_, cv_done_;
  std::function<void()> job_;
  bool has_ = false, stop_ = false;
  std::thread th_;  // last: the loop uses the members above
};

struct MemberStatus {
  int rc = SRHIP_OK;
  std::string msg;
};

}  // namespace

struct srhip_group {
  int ndev = 0;
  std::vector<int32_t> devices;
  std::vector<srhip_ctx*> ctx;
  std::vector<std::unique_ptr<Driver>> drv;
  std::vector<hipEvent_t> done;  // member k records it after its partials are enqueued
  std::mutex mu;                 // one group call at a time
  // pinned, mapped, portable host memory (coherent): the members' packed
  // partials [ndev][slot_len], the gradient programs' static verdicts
  // [ndev][verd_len], and the combined results — sums [nt], ∂L/∂c [nconst], Σw
  // in res, ok [nt] in res_ok — with their addresses on each member's device
  double* slots = nullptr;
  uint8_t* verd = nullptr;
  double* res = nullptr;
  uint8_t* res_ok = nullptr;
  size_t slot_len = 0, verd_len = 0;
  std::vector<double*> d_slot;   // slot k as member k's device sees it
  std::vector<uint8_t*> d_verd;
  double* d_slots0 = nullptr;    // all slots, the results: member 0's device
  double* d_res = nullptr;
  uint8_t* d_res_ok = nullptr;
};

struct srhip_group_dataset {
  srhip_group* g = nullptr;
  int dtype = SRHIP_F32;
  int64_t n = 0;
  int nfeat = 0;
  bool weighted = false;
  std::vector<srhip_dataset*> ds;
};

struct srhip_group_program {
  srhip_group* g = nullptr;
  int dtype = SRHIP_F32;
  int ntrees = 0, nconst = 0;
  std::vector<srhip_program*> prog;
  std::vector<int32_t> const_off;
  std::vector<int32_t*> d_const_off;  // on each member's device (pack and combine kernels)
};

namespace {

// fn(k) on every member's driver thread, all at once; returns when all are done
template <typename F>
std::vector<MemberStatus> run_members(srhip_group* g, F&& fn) {
  std::vector<MemberStatus> st((size_t)g->ndev);
  for (int k = 0; k < g->ndev; ++k)
    g->drv[k]->post([&, k] {
      st[k].rc = guarded([&] {
        fn(k);
        return SRHIP_OK;
      });
      if (st[k].rc != SRHIP_OK) st[k].msg = g_last_error;
    });
  for (int k = 0; k < g->ndev; ++k) g->drv[k]->wait();
  return st;
}

// the first error in member order, as an Error on the calling thread
void throw_first(const srhip_group* g, const std::vector<MemberStatus>& st) {
  for (int k = 0; k < g->ndev; ++k)
    if (st[k].rc != SRHIP_OK)
      throw Error(st[k].rc, "group member " + std::to_string(k) + " (device " + std::to_string(g->devices[k]) +
                                "): " + st[k].msg);
}

void free_group_pinned(srhip_group* g) {
  for (void* h : {(void*)g->slots, (void*)g->verd, (void*)g->res, (void*)g->res_ok})
    if (h) (void)hipHostFree(h);
  g->slots = g->res = nullptr;
  g->verd = g->res_ok = nullptr;
  g->slot_len = g->verd_len = 0;
}

// the pinned buffers for partials of len doubles and nt trees (grow only)
void ensure_group_buffers(srhip_group* g, size_t len, size_t nt) {
  if (len <= g->slot_len && nt <= g->verd_len) return;
  const size_t nl = std::max<size_t>(std::max(len, g->slot_len), 1024);
  const size_t nv = std::max<size_t>(std::max(nt, g->verd_len), 512);
  const unsigned flags = hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent;
  auto st = run_members(g, [&](int k) {
    if (k != 0) return;
    HIP_CHECK(hipSetDevice(g->ctx[0]->device));
    free_group_pinned(g);
    HIP_CHECK(hipHostMalloc((void**)&g->slots, (size_t)g->ndev * nl * sizeof(double), flags));
    HIP_CHECK(hipHostMalloc((void**)&g->verd, (size_t)g->ndev * nv, flags));
    HIP_CHECK(hipHostMalloc((void**)&g->res, nl * sizeof(double), flags));
    HIP_CHECK(hipHostMalloc((void**)&g->res_ok, nv, flags));
    g->slot_len = nl;
    g->verd_len = nv;
  });
  throw_first(g, st);
  st = run_members(g, [&](int k) {
    HIP_CHECK(hipSetDevice(g->ctx[k]->device));
    void* d = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&d, g->slots, 0));
    g->d_slot[k] = static_cast<double*>(d) + (size_t)k * nl;
    if (k == 0) g->d_slots0 = static_cast<double*>(d);
    HIP_CHECK(hipHostGetDevicePointer(&d, g->verd, 0));
    g->d_verd[k] = static_cast<uint8_t*>(d) + (size_t)k * nv;
    if (k == 0) {
      HIP_CHECK(hipHostGetDevicePointer(&d, g->res, 0));
      g->d_res = static_cast<double*>(d);
      HIP_CHECK(hipHostGetDevicePointer(&d, g->res_ok, 0));
      g->d_res_ok = static_cast<uint8_t*>(d);
    }
  });
  throw_first(g, st);
}

void shard_range(int64_t n, int32_t ndev, int32_t k, int64_t* begin, int64_t* end) {
  const int64_t base = n / ndev, extra = n % ndev;
  *begin = k * base + std::min<int64_t>(k, extra);
  *end = *begin + base + (k < extra ? 1 : 0);
}

void destroy_group_program(srhip_group_program* gp) {
  srhip_group* g = gp->g;
  (void)run_members(g, [&](int k) {
    if (gp->d_const_off[k]) {
      (void)hipSetDevice(g->ctx[k]->device);
      (void)hipFree(gp->d_const_off[k]);
    }
    if (gp->prog[k]) (void)srhip_program_destroy(gp->prog[k]);
  });
  delete gp;
}

srhip_group_program* create_group_program(srhip_group* g, int32_t dtype, const srhip_trees* trees, uint32_t flags) {
  if (!g || !trees) throw Error(SRHIP_ERR_INVALID, "null argument");
  std::unique_ptr<srhip_group_program> gp(new srhip_group_program());
  gp->g = g;
  gp->dtype = dtype;
  gp->prog.assign((size_t)g->ndev, nullptr);
  gp->d_const_off.assign((size_t)g->ndev, nullptr);
  // the members build at once: the builders' host threads (8 for one program)
  // are divided between them
  const int cap = std::max(1, 8 / g->ndev);
  std::lock_guard<std::mutex> lk(g->mu);
  auto st = run_members(g, [&](int k) {
    host_thread_cap() = cap;
    const int32_t rc = srhip_program_create_ex(g->ctx[k], dtype, trees, flags, &gp->prog[k]);
    host_thread_cap() = 0;
    check_rc(rc);
    const srhip_program* p = gp->prog[k];
    HIP_CHECK(hipSetDevice(g->ctx[k]->device));
    HIP_CHECK(hipMalloc((void**)&gp->d_const_off[k], p->const_off.size() * sizeof(int32_t)));
    HIP_CHECK(hipMemcpy(gp->d_const_off[k], p->const_off.data(), p->const_off.size() * sizeof(int32_t),
                        hipMemcpyHostToDevice));
  });
  for (int k = 0; k < g->ndev; ++k)
    if (st[k].rc != SRHIP_OK) {
      destroy_group_program(gp.release());
      throw_first(g, st);
    }
  gp->ntrees = gp->prog[0]->ntrees;
  gp->const_off = gp->prog[0]->const_off;
  gp->nconst = gp->const_off.back();
  return gp.release();
}

void set_group_constants(srhip_group_program* gp, const void* consts) {
  if (!gp) throw Error(SRHIP_ERR_INVALID, "null group program");
  srhip_group* g = gp->g;
  std::lock_guard<std::mutex> lk(g->mu);
  auto st = run_members(g, [&](int k) { check_rc(srhip_program_set_constants(gp->prog[k], consts)); });
  throw_first(g, st);
}

// Member k's part of a group evaluation: its shard's packed partials into slot k
// (enqueued on the member's stream, then its event recorded; *recorded false: the
// host wrote the slot, nothing is in flight).
template <typename T>
void member_enqueue(srhip_group* g, int k, srhip_dataset* ds, srhip_program* p, const int32_t* d_const_off, bool grad,
                    int loss, const double* params, bool* recorded) {
  srhip_ctx* c = g->ctx[k];
  check_program_vs_dataset(ds, p);
  CALL_SCOPE(c);
  const int nt = p->ntrees;
  const double wsum = ds->w ? ds->sum_w : (double)ds->rows;
  double* slot = g->slots + (size_t)k * g->slot_len;  // host address
  *recorded = false;
  if (!grad) {
    if (ds->rows == 0) {  // an empty shard launches nothing: the static verdicts, written here
      timing_reset(c);
      c->last_jit_trees = 0;
      for (int t = 0; t < nt; ++t) {
        slot[2 * (size_t)t] = 0.0;
        slot[2 * (size_t)t + 1] = p->static_fail[t] ? 1.0 : 0.0;
      }
      slot[2 * (size_t)nt] = wsum;
      return;
    }
    eval_loss_packed_impl<T>(ds, p, loss, params, g->d_slot[k]);
  } else {
    const int nconst = p->const_off.back();
    build_grad_program<T>(p);
    if (std::is_same<T, float>::value && loss == SRHIP_LOSS_PERIODIC && p->gjit) {
      // Float32 Periodic with gradient tree code: the trees a tile of it failed are evaluated
      // again by the forward-mode interpreter, which needs the host (eval_loss_grad_impl); the
      // member packs the finished results here
      std::vector<double> sum((size_t)std::max(nt, 1)), dl((size_t)std::max(nconst, 1));
      std::vector<uint8_t> ok((size_t)std::max(nt, 1));
      eval_loss_grad_impl<T>(ds, p, loss, params, sum.data(), dl.data(), nullptr, ok.data());
      for (int t = 0; t < nt; ++t) {
        slot[2 * (size_t)t] = ok[t] ? sum[t] : 0.0;
        slot[2 * (size_t)t + 1] = ok[t] ? 0.0 : 1.0;
        for (int32_t j = p->const_off[t]; j < p->const_off[t + 1]; ++j) slot[2 * (size_t)nt + j] = ok[t] ? dl[j] : 0.0;
      }
      slot[2 * (size_t)nt + nconst] = wsum;
      return;
    }
    run_grad<T>(c, p, GRAD_LOSS, ds, loss, params ? params[0] : 0.0, nullptr, nullptr, 0);
    const bool have = ds->rows > 0 && nt > 0 && (p->ngitems[0] + p->ngitems[1] + p->ngitems[2] + p->ngitems[3]) > 0;
    if (ds->rows == 0) {
      for (int t = 0; t < nt; ++t) {
        slot[2 * (size_t)t] = 0.0;
        slot[2 * (size_t)t + 1] = p->g_static_fail[t] ? 1.0 : 0.0;
      }
      for (int j = 0; j < nconst; ++j) slot[2 * (size_t)nt + j] = 0.0;
      slot[2 * (size_t)nt + nconst] = wsum;
      return;
    }
    uint8_t* verd = g->verd + (size_t)k * g->verd_len;
    for (int t = 0; t < nt; ++t) verd[t] = p->g_static_fail[t] ? 1 : 0;
    HIP_CHECK(launch_pack_grad_partials(static_cast<const double*>(c->sums.p), static_cast<const uint8_t*>(c->oks.p),
                                        static_cast<const double*>(c->dloss.p), g->d_verd[k], d_const_off, nt, nconst,
                                        have, wsum, g->d_slot[k], c->stream));
  }
  HIP_CHECK(hipEventRecord(g->done[k], c->stream));
  *recorded = true;
}

// One group evaluation (loss, or loss and ∂L/∂c): every member enqueues its
// shard and its partials; member 0 then makes its stream wait for the other
// members' events, launches the combine kernel over the slots and waits for
// its own stream — the call's one host wait on a device. The results reach the
// caller's arrays only when every member succeeded.
template <typename T>
void group_eval(srhip_group_dataset* gds, srhip_group_program* gp, bool grad, int loss, const double* params,
                double* out_sum, double* out_dloss, double* out_wsum, uint8_t* out_ok) {
  srhip_group* g = gds->g;
  const int ndev = g->ndev, nt = gp->ntrees, nconst = grad ? gp->nconst : 0;
  const size_t len = 2 * (size_t)nt + nconst + 1;
  std::lock_guard<std::mutex> call(g->mu);
  ensure_group_buffers(g, len, (size_t)std::max(nt, 1));
  std::mutex m;
  std::condition_variable cv;
  int left = ndev - 1;  // members other than 0 still enqueueing
  bool failed = false;
  std::vector<uint8_t> recorded((size_t)ndev, 0);
  auto st = run_members(g, [&](int k) {
    srhip_ctx* c = g->ctx[k];
    auto arrive = [&](bool ok) {
      std::lock_guard<std::mutex> lk(m);
      if (!ok) failed = true;
      if (k != 0) --left;
      cv.notify_all();
    };
    try {
      bool rec = false;
      member_enqueue<T>(g, k, gds->ds[k], gp->prog[k], gp->d_const_off[k], grad, loss, params, &rec);
      recorded[k] = rec ? 1 : 0;
    } catch (...) {
      (void)hipSetDevice(c->device);
      (void)hipStreamSynchronize(c->stream);
      arrive(false);
      throw;
    }
    arrive(true);
    if (k != 0) return;
    {
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return left == 0; });
      if (failed) return;  // the caller drains every stream and reports the member's error
    }
    CALL_SCOPE(c);
    for (int j = 1; j < ndev; ++j)
      if (recorded[j]) HIP_CHECK(hipStreamWaitEvent(c->stream, g->done[j], 0));
    HIP_CHECK(launch_combine_partials(g->d_slots0, g->slot_len, ndev, nt, nconst, grad ? gp->d_const_off[0] : nullptr,
                                      g->d_res, g->d_res_ok, grad ? g->d_res + nt : nullptr, g->d_res + nt + nconst,
                                      c->stream));
    wait_stream(c->stream);
    timing_finish(c);
  });
  bool bad = false;
  for (const auto& s : st) bad = bad || s.rc != SRHIP_OK;
  if (bad) {
    (void)run_members(g, [&](int k) {
      (void)hipSetDevice(g->ctx[k]->device);
      (void)hipStreamSynchronize(g->ctx[k]->stream);
    });
    throw_first(g, st);
  }
  if (out_sum) std::copy(g->res, g->res + nt, out_sum);
  if (out_ok) std::copy(g->res_ok, g->res_ok + nt, out_ok);
  if (grad && out_dloss) std::copy(g->res + nt, g->res + nt + nconst, out_dloss);
  if (out_wsum) *out_wsum = g->res[nt + nconst];
}

void group_eval_checked(srhip_group_dataset* gds, srhip_group_program* gp, bool grad, int32_t loss_kind,
                        const double* loss_params, double* out_sum, double* out_dloss, double* out_wsum,
                        uint8_t* out_ok) {
  if (!gds || !gp) throw Error(SRHIP_ERR_INVALID, "null group dataset or program");
  if (gds->g != gp->g) throw Error(SRHIP_ERR_INVALID, "the group program belongs to another group than the dataset");
  if (gds->dtype != gp->dtype) throw Error(SRHIP_ERR_INVALID, "dataset and program dtypes differ");
  check_loss(loss_kind, loss_params);
  check_expr_loss_weights(loss_kind, gds->weighted);
  by_dtype(gds->dtype, [&](auto t) {
    group_eval<decltype(t)>(gds, gp, grad, loss_kind, loss_params, out_sum, out_dloss, out_wsum, out_ok);
  });
}

// The candidates of one evaluation set as a group program (EngineSet with the
// rows sharded): the two group evaluations, finished as the reference's loss.
struct GroupSet : copt::Set {
  srhip_group_dataset* gds;
  int dtype, loss;
  const double* params;
  srhip_group_program* gp = nullptr;
  std::vector<int32_t> coff;
  GroupSet(srhip_group_dataset* d, const srhip_trees* trees, int ls, const double* pr,
           const std::vector<int32_t>& members)
      : gds(d), dtype(d->dtype), loss(ls), params(pr) {
    MemberTrees mt(trees, dtype, members);
    coff = mt.coff;
    gp = create_group_program(gds->g, dtype, &mt.tr, SRHIP_PROGRAM_VARYING_CONSTANTS);
  }
  ~GroupSet() override {
    if (!gp) return;
    std::lock_guard<std::mutex> lk(gds->g->mu);
    destroy_group_program(gp);
  }
  void eval(const std::vector<double>& X, bool grad, std::vector<double>& f, std::vector<double>& g) override {
    const int n = (int)coff.size() - 1;
    const size_t nc = (size_t)coff.back();
    if (X.size() != nc) throw Error(SRHIP_ERR_INVALID, "constant count mismatch");
    if (dtype == SRHIP_F32) {
      std::vector<float> c(nc);
      for (size_t j = 0; j < nc; ++j) c[j] = (float)X[j];
      set_group_constants(gp, c.data());
    } else {
      set_group_constants(gp, X.data());
    }
    std::vector<double> sums(std::max(n, 1)), dl(std::max<size_t>(nc, 1));
    std::vector<uint8_t> ok(std::max(n, 1));
    double wsum = 0.0;
    group_eval_checked(gds, gp, grad, loss, params, sums.data(), grad ? dl.data() : nullptr, &wsum, ok.data());
    f.assign(n, 0.0);
    for (int t = 0; t < n; ++t) {
      const double v = sums[t] / wsum;
      f[t] = (ok[t] && std::isfinite(v)) ? v : INFINITY;
    }
    if (grad) {
      g.assign(nc, 0.0);
      for (int t = 0; t < n; ++t)
        for (int32_t j = coff[t]; j < coff[t + 1]; ++j) g[j] = ok[t] ? dl[j] / wsum : NAN;
    }
  }
};
struct GroupFactory : copt::Factory {
  srhip_group_dataset* gds;
  const srhip_trees* trees;
  int loss;
  const double* params;
  std::unique_ptr<copt::Set> make(const std::vector<int32_t>& members) override {
    return std::unique_ptr<copt::Set>(new GroupSet(gds, trees, loss, params, members));
  }
};

}  // namespace

extern "C" {

int32_t srhip_group_shard_range(int64_t n, int32_t ndev, int32_t k, int64_t* begin, int64_t* end) {
  return guarded([&] {
    if (n < 0 || ndev < 1 || ndev > kMaxGroup || k < 0 || k >= ndev)
      throw Error(SRHIP_ERR_INVALID, "shard range: need n >= 0, 1 <= ndev <= 16 and 0 <= k < ndev");
    if (!begin || !end) throw Error(SRHIP_ERR_INVALID, "null output");
    shard_range(n, ndev, k, begin, end);
    return SRHIP_OK;
  });
}

int32_t srhip_group_open(const int32_t* devices, int32_t ndev, srhip_group** out) {
  return guarded([&] {
    if (!out) throw Error(SRHIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!devices) throw Error(SRHIP_ERR_INVALID, "null device list");
    if (ndev < 1 || ndev > kMaxGroup) throw Error(SRHIP_ERR_INVALID, "a group has 1 to 16 members");
    for (int k = 0; k < ndev; ++k)
      if (devices[k] < 0) throw Error(SRHIP_ERR_INVALID, "negative device index");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    for (int k = 0; k < ndev; ++k)
      if (devices[k] >= n)
        throw Error(SRHIP_ERR_DEVICE, n == 0 ? std::string("no HIP device available")
                                             : "group member " + std::to_string(k) + ": device " +
                                                   std::to_string(devices[k]) + " of " + std::to_string(n));
    std::unique_ptr<srhip_group> g(new srhip_group());
    g->ndev = ndev;
    g->devices.assign(devices, devices + ndev);
    g->ctx.assign((size_t)ndev, nullptr);
    g->done.assign((size_t)ndev, nullptr);
    g->d_slot.assign((size_t)ndev, nullptr);
    g->d_verd.assign((size_t)ndev, nullptr);
    for (int k = 0; k < ndev; ++k) g->drv.emplace_back(new Driver());
    auto st = run_members(g.get(), [&](int k) {
      check_rc(srhip_open(g->devices[k], &g->ctx[k]));
      // no timing; a system-scope release, so that what the member wrote to the
      // pinned slots is visible to another device once the event has completed
      HIP_CHECK(hipEventCreateWithFlags(&g->done[k], hipEventDisableTiming | hipEventReleaseToSystem));
    });
    for (int k = 0; k < ndev; ++k)
      if (st[k].rc != SRHIP_OK) {
        srhip_group* raw = g.release();
        std::string msg;
        try {
          throw_first(raw, st);
        } catch (const Error& e) {
          msg = e.what();
        }
        (void)srhip_group_close(raw);
        throw Error(st[k].rc, msg);
      }
    *out = g.release();
    return SRHIP_OK;
  });
}

int32_t srhip_group_close(srhip_group* group) {
  return guarded([&] {
    if (!group) return SRHIP_OK;
    {
      std::lock_guard<std::mutex> lk(group->mu);
      (void)run_members(group, [&](int k) {
        if (!group->ctx[k]) return;
        (void)hipSetDevice(group->ctx[k]->device);
        (void)hipStreamSynchronize(group->ctx[k]->stream);
        if (group->done[k]) (void)hipEventDestroy(group->done[k]);
        if (k == 0) free_group_pinned(group);
        (void)srhip_close(group->ctx[k]);
        group->ctx[k] = nullptr;
      });
      group->drv.clear();  // joins the driver threads
    }
    delete group;
    return SRHIP_OK;
  });
}

int32_t srhip_group_info(const srhip_group* group, int32_t* out_ndev, int32_t* devices_out) {
  return guarded([&] {
    if (!group) throw Error(SRHIP_ERR_INVALID, "null group");
    if (out_ndev) *out_ndev = group->ndev;
    if (devices_out) std::copy(group->devices.begin(), group->devices.end(), devices_out);
    return SRHIP_OK;
  });
}

int32_t srhip_group_ctx(srhip_group* group, int32_t k, srhip_ctx** out) {
  return guarded([&] {
    if (!group || !out) throw Error(SRHIP_ERR_INVALID, "null group or out");
    *out = nullptr;
    if (k < 0 || k >= group->ndev) throw Error(SRHIP_ERR_INVALID, "member index out of range");
    *out = group->ctx[k];
    return SRHIP_OK;
  });
}

int32_t srhip_group_dataset_destroy(srhip_group_dataset* gds) {
  return guarded([&] {
    if (!gds) return SRHIP_OK;
    {
      std::lock_guard<std::mutex> lk(gds->g->mu);
      (void)run_members(gds->g, [&](int k) {
        if (gds->ds[k]) (void)srhip_dataset_destroy(gds->ds[k]);
      });
    }
    delete gds;
    return SRHIP_OK;
  });
}

int32_t srhip_group_dataset_create(srhip_group* group, int32_t dtype, int32_t x_layout, const void* X, const void* y,
                                   const void* w, int64_t n, int32_t nfeat, srhip_group_dataset** out) {
  return guarded([&] {
    if (!group || !out) throw Error(SRHIP_ERR_INVALID, "null group or out");
    *out = nullptr;
    if (n < 0) throw Error(SRHIP_ERR_INVALID, "bad shape");
    std::unique_ptr<srhip_group_dataset> gds(new srhip_group_dataset());
    gds->g = group;
    gds->dtype = dtype;
    gds->n = n;
    gds->nfeat = nfeat;
    gds->weighted = w != nullptr;
    gds->ds.assign((size_t)group->ndev, nullptr);
    std::vector<MemberStatus> st;
    {
      std::lock_guard<std::mutex> lk(group->mu);
      st = run_members(group, [&](int k) {
        int64_t b, e;
        shard_range(n, group->ndev, k, &b, &e);
        check_rc(srhip_dataset_create(group->ctx[k], dtype, x_layout, X, y, w, n, nfeat, b, e, &gds->ds[k]));
      });
    }
    for (int k = 0; k < group->ndev; ++k)
      if (st[k].rc != SRHIP_OK) {
        (void)srhip_group_dataset_destroy(gds.release());
        throw_first(group, st);
      }
    *out = gds.release();
    return SRHIP_OK;
  });
}

int32_t srhip_group_dataset_info(const srhip_group_dataset* gds, int64_t* out_rows, int32_t* out_nfeat,
                                 double* out_sum_w, double* out_sum_yw, int32_t* out_x_finite) {
  return guarded([&] {
    if (!gds) throw Error(SRHIP_ERR_INVALID, "null group dataset");
    double sw = 0.0, syw = 0.0;
    bool fin = true;
    for (const srhip_dataset* d : gds->ds) {  // member order
      sw += d->sum_w;
      syw += d->sum_yw;
      fin = fin && d->x_finite;
    }
    if (out_rows) *out_rows = gds->n;
    if (out_nfeat) *out_nfeat = gds->nfeat;
    if (out_sum_w) *out_sum_w = sw;
    if (out_sum_yw) *out_sum_yw = syw;
    if (out_x_finite) *out_x_finite = fin ? 1 : 0;
    return SRHIP_OK;
  });
}

int32_t srhip_group_program_create(srhip_group* group, int32_t dtype, const srhip_trees* trees, uint32_t flags,
                                   srhip_group_program** out) {
  return guarded([&] {
    if (!out) throw Error(SRHIP_ERR_INVALID, "out is null");
    *out = nullptr;
    *out = create_group_program(group, dtype, trees, flags);
    return SRHIP_OK;
  });
}

int32_t srhip_group_program_destroy(srhip_group_program* gp) {
  return guarded([&] {
    if (!gp) return SRHIP_OK;
    std::lock_guard<std::mutex> lk(gp->g->mu);
    destroy_group_program(gp);
    return SRHIP_OK;
  });
}

int32_t srhip_group_program_set_constants(srhip_group_program* gp, const void* consts) {
  return guarded([&] {
    set_group_constants(gp, consts);
    return SRHIP_OK;
  });
}

int32_t srhip_group_eval_loss(srhip_group_dataset* gds, srhip_group_program* gp, int32_t loss_kind,
                              const double* loss_params, double* out_loss_sum, double* out_weight_sum,
                              uint8_t* out_ok) {
  return guarded([&] {
    group_eval_checked(gds, gp, false, loss_kind, loss_params, out_loss_sum, nullptr, out_weight_sum, out_ok);
    return SRHIP_OK;
  });
}

int32_t srhip_group_eval_loss_grad(srhip_group_dataset* gds, srhip_group_program* gp, int32_t loss_kind,
                                   const double* loss_params, double* out_loss_sum, double* out_dloss,
                                   double* out_weight_sum, uint8_t* out_ok) {
  return guarded([&] {
    group_eval_checked(gds, gp, true, loss_kind, loss_params, out_loss_sum, out_dloss, out_weight_sum, out_ok);
    return SRHIP_OK;
  });
}

int32_t srhip_group_optimize_constants(srhip_group_dataset* gds, const srhip_trees* trees,
                                       const srhip_constopt_options* opts, void* out_consts, double* out_loss,
                                       uint8_t* out_converged, double* out_num_evals) {
  return guarded([&] {
    if (!gds) throw Error(SRHIP_ERR_INVALID, "null group dataset");
    if (!opts) throw Error(SRHIP_ERR_INVALID, "null options");
    check_loss(opts->loss_kind, opts->loss_params);
    check_expr_loss_weights(opts->loss_kind, gds->weighted);
    copt::Problem pb = make_problem(trees, gds->dtype);
    GroupFactory fac;
    fac.gds = gds;
    fac.trees = trees;
    fac.loss = opts->loss_kind;
    fac.params = opts->loss_params;
    const copt::Result r = copt::optimize(pb, make_copt_options(opts), fac);
    write_result(r, gds->dtype, out_consts, out_loss, out_converged, out_num_evals, true);
    return SRHIP_OK;
  });
}

}  // extern "C"
