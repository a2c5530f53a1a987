// compile.cpp — postfix node streams → device accumulator-machine programs.
//
// Per tree:
//  1. parse the post-order stream into nodes (DAG sharing was already
//     expanded by the flattener: a shared child appears once per reference,
//     as DynamicExpressions evaluates it, test_preserve_multiple_parents.jl:9-14);
//  2. fold every maximal feature-free subtree of degree >= 1 into one
//     constant with host_ops.h, reproducing `_eval_constant_tree` (a folded
//     operator output that is non-finite makes the tree fail for every row
//     count, as the reference does before looking at rows);
//  3. static checks of the remaining constant leaves: DynamicExpressions
//     checks every constant leaf that sits next to a feature-bearing subtree
//     (`@return_on_check` in the fused deg2_l0*/deg1_l2* kernels), so a
//     non-finite one fails the tree; a non-finite constant ROOT fails only
//     when there are rows (fill + final array check);
//  4. emit code in Sethi–Ullman order (the operand needing more stack slots
//     first), fusing leaf operands into the consuming instruction.
#include "compile.h"

#include <algorithm>
#include <limits>
#include <exception>
#include <mutex>
#include <thread>
#include <utility>

#include <cmath>
#include <cstring>

#include "host_ops.h"

namespace srhip {

// ---- expression operators: registry and host semantics -------------------------------
namespace {
struct ExprOpEntry {
  int32_t id;
  std::shared_ptr<const ExprOp> live;  // reset by destroy
  std::weak_ptr<const ExprOp> held;    // still reachable while a program holds it
};
std::mutex g_xop_mu;
std::vector<ExprOpEntry> g_xop;
int32_t g_xop_next = SRHIP_EXPR_OP_BEGIN;
}  // namespace

int32_t expr_op_create(int32_t arity, const uint8_t* kind, const uint16_t* arg, int32_t nnodes, const double* consts,
                       int32_t nconsts) {
  if (arity != 1 && arity != 2) throw Error(SRHIP_ERR_INVALID, "expression operator: arity must be 1 or 2");
  if (!kind || !arg || nnodes <= 0 || nconsts < 0 || (nconsts > 0 && !consts))
    throw Error(SRHIP_ERR_INVALID, "expression operator: null or empty node stream");
  auto e = std::make_shared<ExprOp>();
  e->arity = arity;
  e->nd.resize((size_t)nnodes);
  std::vector<int> st;
  int nc = 0, maxdepth = 0;
  bool beyond_ops = false;
  for (int i = 0; i < nnodes; ++i) {
    ExprOp::N& n = e->nd[(size_t)i];
    n = ExprOp::N{0, 0, -1, 0.0, -1, -1, 0};
    switch (kind[i]) {
      case SRHIP_NODE_CONST:
        if (nc >= nconsts) throw Error(SRHIP_ERR_INVALID, "expression operator: more constant leaves than constants");
        if (!std::isfinite(consts[nc])) throw Error(SRHIP_ERR_INVALID, "expression operator: non-finite constant");
        n.val = consts[nc++];
        e->cost += 1;
        break;
      case SRHIP_NODE_FEATURE:
        if ((int)arg[i] >= arity)
          throw Error(SRHIP_ERR_INVALID, "expression operator: feature index beyond the arity (0: first argument, 1: second)");
        n.feat = arg[i];
        e->cost += 1;
        break;
      case SRHIP_NODE_UNARY:
        if (st.empty()) throw Error(SRHIP_ERR_INVALID, "expression operator: stack underflow");
        n.deg = 1;
        n.op = arg[i];
        if (arg[i] >= SRHIP_NUM_UOPS) beyond_ops = true;
        else e->cost += uop_cost(arg[i]);
        n.l = st.back();
        st.pop_back();
        n.need = e->nd[(size_t)n.l].need;
        break;
      case SRHIP_NODE_BINARY: {
        if (st.size() < 2) throw Error(SRHIP_ERR_INVALID, "expression operator: stack underflow");
        n.deg = 2;
        n.op = arg[i];
        if (arg[i] >= SRHIP_NUM_BOPS) beyond_ops = true;
        else e->cost += bop_cost(arg[i]);
        n.r = st.back();
        st.pop_back();
        n.l = st.back();
        st.pop_back();
        const ExprOp::N& L = e->nd[(size_t)n.l];
        const ExprOp::N& R = e->nd[(size_t)n.r];
        const int hi = std::max(L.need, R.need), lo = std::min(L.need, R.need);
        n.need = (L.deg == 0 || R.deg == 0) ? hi : std::max(hi, lo + 1);
        break;
      }
      default: throw Error(SRHIP_ERR_INVALID, "expression operator: unknown node kind");
    }
    st.push_back(i);
    maxdepth = std::max(maxdepth, (int)st.size());
  }
  if (st.size() != 1)
    throw Error(SRHIP_ERR_INVALID, "expression operator: the stream leaves " + std::to_string(st.size()) + " values");
  if (nc != nconsts) throw Error(SRHIP_ERR_INVALID, "expression operator: constant count mismatch");
  if (beyond_ops)
    throw Error(SRHIP_ERR_UNSUPPORTED, "expression operator: operator id beyond the engine's table (a body holds primitives only)");
  if (nnodes > kExprOpMaxNodes) throw Error(SRHIP_ERR_UNSUPPORTED, "expression operator: more than 64 nodes");
  if (maxdepth > kExprOpMaxDepth)
    throw Error(SRHIP_ERR_UNSUPPORTED, "expression operator: more than 4 values live on the stack");
  std::lock_guard<std::mutex> lk(g_xop_mu);
  if (g_xop_next > 0xffff) throw Error(SRHIP_ERR_NOMEM, "expression operator handles exhausted");  // srhip_trees.arg is 16 bits
  const int32_t id = g_xop_next++;
  g_xop.push_back({id, e, e});
  return id;
}

void expr_op_destroy(int32_t id) {
  std::lock_guard<std::mutex> lk(g_xop_mu);
  for (auto& x : g_xop)
    if (x.id == id && x.live) {
      x.live.reset();
      return;
    }
  throw Error(SRHIP_ERR_INVALID, "operator id " + std::to_string(id) + " is not a registered expression operator");
}

std::shared_ptr<const ExprOp> expr_op_find(int32_t id, bool live) {
  std::lock_guard<std::mutex> lk(g_xop_mu);
  if (id >= g_xop_next) throw Error(SRHIP_ERR_UNSUPPORTED, "unknown operator id " + std::to_string(id));
  for (const auto& x : g_xop)
    if (x.id == id) {
      std::shared_ptr<const ExprOp> e = x.live ? x.live : live ? nullptr : x.held.lock();
      if (e) return e;
      break;
    }
  throw Error(SRHIP_ERR_INVALID, "operator id " + std::to_string(id) + " is a destroyed expression operator");
}

std::vector<std::shared_ptr<const ExprOp>> expr_ops_of(const srhip_trees& trees) {
  std::vector<std::shared_ptr<const ExprOp>> ops;
  std::vector<int32_t> seen;
  if (trees.ntrees <= 0 || !trees.node_off || !trees.kind || !trees.arg) return ops;
  for (int i = trees.node_off[0], e = trees.node_off[trees.ntrees]; i < e; ++i) {
    const int k = trees.kind[i], id = trees.arg[i];
    if ((k != SRHIP_NODE_UNARY && k != SRHIP_NODE_BINARY) || id < SRHIP_EXPR_OP_BEGIN) continue;
    if (std::find(seen.begin(), seen.end(), id) != seen.end()) continue;
    seen.push_back(id);
    ops.push_back(expr_op_find(id, /*live=*/true));
  }
  return ops;
}

template <typename T>
T expr_op_eval(const ExprOp& e, T a, T b) {
  T st[kExprOpMaxDepth];
  int sp = 0;
  for (const ExprOp::N& n : e.nd) {
    if (n.deg == 0) st[sp++] = n.feat < 0 ? (T)n.val : n.feat == 0 ? a : b;
    else if (n.deg == 1) st[sp - 1] = host::unop<T>(n.op, st[sp - 1]);
    else {
      st[sp - 2] = host::binop<T>(n.op, st[sp - 2], st[sp - 1]);
      --sp;
    }
  }
  return st[0];
}
template float expr_op_eval<float>(const ExprOp&, float, float);
template double expr_op_eval<double>(const ExprOp&, double, double);

namespace {


struct HNode {
  int deg;       // 0, 1, 2
  int op;        // operator id (deg >= 1)
  int feat;      // feature index (deg 0, -1 for a constant)
  int l, r;      // children
  double val;    // constant value (deg 0 const), held in T precision
  int cidx;      // constant index in get_constants order (deg 0 const); <= -2: folded (cmap fold ref)
  int size;      // nodes in the subtree (postfix: it spans [i - size + 1, i])
  int cpre;      // constants before the subtree's first node (tree-local)
  bool has_feature;
  int need;      // stack slots needed (Sethi–Ullman number for this machine)
  const ExprOp* xop;  // deg >= 1: the body of an expression operator (op >= SRHIP_EXPR_OP_BEGIN), else null
};

template <typename T>
struct TreeCompiler {
  std::vector<HNode> nd;
  std::vector<Ins<T>>* out;
  std::vector<int32_t>* cmap;  // parallel to out: batch-wide constant index of each immediate
  std::vector<FoldRec>* folds;
  int cbase = 0;               // batch-wide index of this tree's first constant
  int nbase = 0;               // batch-wide index of this tree's first node
  bool grad = false;  // slot field carries constant indices
  bool fold_fail = false;
  int max_feat = -1;
  // expression operators met so far (kept alive for the batch) and, per tree,
  // whether emit() expanded one into the program
  std::vector<std::pair<int32_t, std::shared_ptr<const ExprOp>>> xops;
  bool emitted_xop = false;
  uint32_t body_flag = 0;  // the no-mark flag, set while a body is emitted

  const ExprOp* xop_of(int32_t id, int arity) {
    const ExprOp* e = nullptr;
    for (const auto& x : xops)
      if (x.first == id) e = x.second.get();
    if (!e) {
      xops.emplace_back(id, expr_op_find(id, /*live=*/false));
      e = xops.back().second.get();
    }
    if (e->arity != arity)
      throw Error(SRHIP_ERR_INVALID, "expression operator " + std::to_string(id) + " takes " + std::to_string(e->arity) +
                                         " argument(s) but sits in a node of " + std::to_string(arity));
    return e;
  }

  static bool is_leaf(const HNode& x) { return x.deg == 0; }

  // Scalar evaluation of a feature-free subtree (`_eval_constant_tree`).
  bool eval_const(int i, T* v) {
    const HNode& x = nd[i];
    if (x.deg == 0) { *v = (T)x.val; return true; }
    if (x.deg == 1) {
      T a;
      if (!eval_const(x.l, &a)) return false;
      *v = x.xop ? expr_op_eval<T>(*x.xop, a, T(0)) : host::unop<T>(x.op, a);
      return std::isfinite(*v);
    }
    T a, b;
    if (!eval_const(x.l, &a) || !eval_const(x.r, &b)) return false;
    *v = x.xop ? expr_op_eval<T>(*x.xop, a, b) : host::binop<T>(x.op, a, b);
    return std::isfinite(*v);
  }

  void fold(int i) {
    HNode& x = nd[i];
    if (x.deg == 0) return;
    if (!x.has_feature) {
      T v;
      if (!eval_const(i, &v)) {
        fold_fail = true;
        v = std::numeric_limits<T>::quiet_NaN();  // the tree fails statically; a defined immediate (keep_layout)
      }
      const int first = i - x.size + 1;
      folds->push_back({nbase + first, nbase + i + 1, cbase + nd[first].cpre});
      x.deg = 0; x.feat = -1; x.val = (double)v; x.l = x.r = -1; x.xop = nullptr;
      x.cidx = -2 - ((int)folds->size() - 1);  // a folded value: its cmap reference
      return;
    }
    fold(x.l);
    if (x.deg == 2) fold(x.r);
  }

  int compute_need(int i) {
    HNode& x = nd[i];
    if (x.deg == 0) return x.need = 0;
    if (x.xop) {
      // computed arguments sit in reserved slots (the one needing more first),
      // the body's own temporaries above them
      const int body = x.xop->nd.back().need;
      const int a = compute_need(x.l), b = x.deg == 2 ? compute_need(x.r) : 0;
      const bool cl = !is_leaf(nd[x.l]), cr = x.deg == 2 && !is_leaf(nd[x.r]);
      if (cl && cr) return x.need = std::max({std::max(a, b), std::min(a, b) + 1, 2 + body});
      if (cl || cr) return x.need = std::max(cl ? a : b, 1 + body);
      return x.need = body;
    }
    if (x.deg == 1) return x.need = compute_need(x.l);
    int a = compute_need(x.l), b = compute_need(x.r);
    const HNode& L = nd[x.l];
    const HNode& R = nd[x.r];
    if (is_leaf(L) || is_leaf(R)) return x.need = std::max(a, b);
    int hi = std::max(a, b), lo = std::min(a, b);
    return x.need = std::max(hi, lo + 1);
  }

  bool nonroot_const_nonfinite(int i) {
    const HNode& x = nd[i];
    if (x.deg == 0) return x.feat < 0 && !std::isfinite(x.val);
    if (nonroot_const_nonfinite(x.l)) return true;
    return x.deg == 2 && nonroot_const_nonfinite(x.r);
  }

  uint32_t need_x(int opc) const {
    if (grad) return 0;
    const bool nx = opc == OP_LDX || (opc >= OP_BIN0 && variant_needs_x((opc - OP_BIN0) / SRHIP_NUM_BOPS));
    return nx ? kNeedX : 0;
  }
  void put(int opc, int slot, int feat, T imm, int32_t gidx = -1) {
    Ins<T> ins;
    std::memset(&ins, 0, sizeof(ins));
    ins.code = make_code(opc, slot, feat) | need_x(opc) | body_flag;
    ins.imm = imm;
    out->push_back(ins);
    cmap->push_back(gidx);
  }
  // the constant operand x: its immediate and batch-wide index
  void putc(int opc, const HNode& x, int feat) {
    put(opc, ci(x), feat, (T)x.val, x.cidx >= 0 ? cbase + x.cidx : x.cidx <= -2 ? x.cidx : -1);
  }
  void put_feat2(int opc, int f, int g) {
    Ins<T> ins;
    std::memset(&ins, 0, sizeof(ins));
    ins.code = make_code(opc, 0, f) | need_x(opc) | body_flag;
    if constexpr (sizeof(T) == 4) {
      uint32_t gg = (uint32_t)g;
      std::memcpy(&ins.imm, &gg, 4);
    } else {
      uint64_t gg = (uint64_t)g;
      std::memcpy(&ins.imm, &gg, 8);
    }
    out->push_back(ins);
    cmap->push_back(-1);
  }

  // ---- expression operators -----------------------------------------------------
  // An argument of the operator as the body reads it: a feature or constant leaf
  // of the enclosing tree (bound directly: the fused X / C variants serve it), a
  // body constant (fixed: no constant index, no tangent), or a reserved slot.
  struct Leaf {
    int k;         // 0: X[feat], 1: immediate, 2: slot
    int feat;
    T val;
    int cslot;     // slot field of an immediate (gradient programs: the constant's index)
    int32_t gidx;  // its cmap entry
    int slot;
  };
  struct Bind { const HNode* leaf; int slot; };

  Leaf leaf_of(const ExprOp::N& n, const Bind* b) const {
    if (n.feat < 0) return Leaf{1, 0, (T)n.val, grad ? kBodyConst : 0, -1, 0};
    const Bind& q = b[n.feat];
    if (!q.leaf) return Leaf{2, 0, T(0), 0, -1, q.slot};
    const HNode& h = *q.leaf;
    if (h.feat >= 0) return Leaf{0, h.feat, T(0), 0, -1, 0};
    return Leaf{1, 0, (T)h.val, ci(h), h.cidx >= 0 ? cbase + h.cidx : h.cidx <= -2 ? h.cidx : -1, 0};
  }
  void putl(int opc, const Leaf& c, int feat) { put(opc, c.cslot, feat, c.val, c.gidx); }

  // Emit the body subtree i leaving its value in acc; slots [base, ...) are free.
  void emit_body(const ExprOp& e, int i, int base, const Bind* b) {
    const ExprOp::N& n = e.nd[(size_t)i];
    if (n.deg == 0) {
      const Leaf q = leaf_of(n, b);
      if (q.k == 0) put(OP_LDX, 0, q.feat, T(0));
      else if (q.k == 1) putl(OP_LDC, q, 0);
      else put(OP_LDS0 + q.slot, q.slot, 0, T(0));
      return;
    }
    if (n.deg == 1) {
      emit_body(e, n.l, base, b);
      put(OP_UN0 + n.op, 0, 0, T(0));
      return;
    }
    const ExprOp::N& L = e.nd[(size_t)n.l];
    const ExprOp::N& R = e.nd[(size_t)n.r];
    const int op = n.op;
    if (L.deg == 0 && R.deg == 0) {
      const Leaf a = leaf_of(L, b), c = leaf_of(R, b);
      if (a.k == 0 && c.k == 0) put_feat2(bin_opcode(V_XX, op), a.feat, c.feat);
      else if (a.k == 0 && c.k == 1) putl(bin_opcode(V_XC, op), c, a.feat);
      else if (a.k == 1 && c.k == 0) putl(bin_opcode(V_CX, op), a, c.feat);
      else if (a.k == 1 && c.k == 1) {
        putl(OP_LDC, a, 0);
        putl(bin_opcode(V_AC, op), c, 0);
      } else if (a.k == 2) {
        put(OP_LDS0 + a.slot, a.slot, 0, T(0));
        if (c.k == 0) put(bin_opcode(V_AX, op), 0, c.feat, T(0));
        else if (c.k == 1) putl(bin_opcode(V_AC, op), c, 0);
        else {
          put(OP_POP0 + c.slot, c.slot, 0, T(0));
          put(bin_opcode(V_AT, op), 0, 0, T(0));
        }
      } else {  // (X or immediate, slot)
        put(OP_LDS0 + c.slot, c.slot, 0, T(0));
        if (a.k == 0) put(bin_opcode(V_XA, op), 0, a.feat, T(0));
        else putl(bin_opcode(V_CA, op), a, 0);
      }
      return;
    }
    if (R.deg == 0) {
      emit_body(e, n.l, base, b);
      const Leaf c = leaf_of(R, b);
      if (c.k == 0) put(bin_opcode(V_AX, op), 0, c.feat, T(0));
      else if (c.k == 1) putl(bin_opcode(V_AC, op), c, 0);
      else {
        put(OP_POP0 + c.slot, c.slot, 0, T(0));
        put(bin_opcode(V_AT, op), 0, 0, T(0));
      }
      return;
    }
    if (L.deg == 0) {
      emit_body(e, n.r, base, b);
      const Leaf a = leaf_of(L, b);
      if (a.k == 0) put(bin_opcode(V_XA, op), 0, a.feat, T(0));
      else if (a.k == 1) putl(bin_opcode(V_CA, op), a, 0);
      else {
        put(OP_POP0 + a.slot, a.slot, 0, T(0));
        put(bin_opcode(V_TA, op), 0, 0, T(0));
      }
      return;
    }
    if (base >= kMaxSlots) throw Error(SRHIP_ERR_UNSUPPORTED, "tree needs more than 16 stack slots");
    const bool lf = L.need >= R.need;
    emit_body(e, lf ? n.l : n.r, base, b);
    put(OP_PUSH0 + base, base, 0, T(0));
    emit_body(e, lf ? n.r : n.l, base + 1, b);
    put(OP_POP0 + base, base, 0, T(0));
    put(bin_opcode(lf ? V_TA : V_AT, op), 0, 0, T(0));
  }

  // The expression-operator node i: its computed arguments into reserved slots
  // [base, ...), each checked (OP_MARK: the reference checks every child
  // array), then the body in line, flagged no-mark: nothing inside is checked.
  void emit_xop(int i, int base) {
    const HNode& x = nd[i];
    const int kid[2] = {x.l, x.deg == 2 ? x.r : -1};
    int order[2] = {0, 1};
    if (x.deg == 2 && !is_leaf(nd[x.l]) && !is_leaf(nd[x.r]) && nd[x.r].need > nd[x.l].need) std::swap(order[0], order[1]);
    Bind b[2] = {{nullptr, 0}, {nullptr, 0}};
    int nb = base;
    for (int k : order) {
      const int j = kid[k];
      if (j < 0) continue;
      if (is_leaf(nd[j])) {
        b[k].leaf = &nd[j];
        continue;
      }
      if (nb >= kMaxSlots) throw Error(SRHIP_ERR_UNSUPPORTED, "tree needs more than 16 stack slots");
      emit(j, nb);
      put(OP_MARK, 0, 0, T(0));
      put(OP_PUSH0 + nb, nb, 0, T(0));
      b[k].slot = nb++;
    }
    emitted_xop = true;
    body_flag = grad ? kNoMarkGrad : kNoMark;
    emit_body(*x.xop, (int)x.xop->nd.size() - 1, nb, b);
    body_flag = 0;
  }

  // Emit code leaving node i's value in acc; slots [base, ...) are free.
  void emit(int i, int base) {
    const HNode& x = nd[i];
    if (x.deg == 0) {
      if (x.feat >= 0) put(OP_LDX, 0, x.feat, T(0));
      else putc(OP_LDC, x, 0);
      return;
    }
    if (x.xop) {
      emit_xop(i, base);
      return;
    }
    if (x.deg == 1) {
      emit(x.l, base);
      put(OP_UN0 + x.op, 0, 0, T(0));
      return;
    }
    const HNode& L = nd[x.l];
    const HNode& R = nd[x.r];
    const int op = x.op;
    if (is_leaf(L) && is_leaf(R)) {
      if (L.feat >= 0 && R.feat >= 0) put_feat2(bin_opcode(V_XX, op), L.feat, R.feat);
      else if (L.feat >= 0) putc(bin_opcode(V_XC, op), R, L.feat);
      else if (R.feat >= 0) putc(bin_opcode(V_CX, op), L, R.feat);
      else {  // two constants: only without folding (gradient programs)
        putc(OP_LDC, L, 0);
        putc(bin_opcode(V_AC, op), R, 0);
      }
      return;
    }
    if (is_leaf(R)) {
      emit(x.l, base);
      if (R.feat >= 0) put(bin_opcode(V_AX, op), 0, R.feat, T(0));
      else putc(bin_opcode(V_AC, op), R, 0);
      return;
    }
    if (is_leaf(L)) {
      emit(x.r, base);
      if (L.feat >= 0) put(bin_opcode(V_XA, op), 0, L.feat, T(0));
      else putc(bin_opcode(V_CA, op), L, 0);
      return;
    }
    if (base >= kMaxSlots) throw Error(SRHIP_ERR_UNSUPPORTED, "tree needs more than 16 stack slots");
    if (L.need >= R.need) {
      emit(x.l, base);
      put(OP_PUSH0 + base, base, 0, T(0));
      emit(x.r, base + 1);
      put(OP_POP0 + base, base, 0, T(0));
      put(bin_opcode(V_TA, op), 0, 0, T(0));  // lhs = tmp (left), rhs = acc (right)
    } else {
      emit(x.r, base);
      put(OP_PUSH0 + base, base, 0, T(0));
      emit(x.l, base + 1);
      put(OP_POP0 + base, base, 0, T(0));
      put(bin_opcode(V_AT, op), 0, 0, T(0));  // lhs = acc (left), rhs = tmp (right)
    }
  }

  // slot-field value of a constant operand: its index (gradient programs)
  int ci(const HNode& x) const { return grad ? x.cidx : 0; }

  bool any_const_nonfinite(int i) const {
    const HNode& x = nd[i];
    if (x.deg == 0) return x.feat < 0 && !std::isfinite(x.val);
    if (any_const_nonfinite(x.l)) return true;
    return x.deg == 2 && any_const_nonfinite(x.r);
  }

  int cost(int i) const {
    const HNode& x = nd[i];
    if (x.deg == 0) return 1;
    if (x.deg == 1) return (x.xop ? x.xop->cost : uop_cost(x.op)) + cost(x.l);
    return (x.xop ? x.xop->cost : bop_cost(x.op)) + cost(x.l) + cost(x.r);
  }
};

}  // namespace

template <typename T>
CompiledBatch<T> compile_batch(const srhip_trees& trees, bool grad, bool keep_layout) {
  if (trees.ntrees < 0) throw Error(SRHIP_ERR_INVALID, "negative tree count");
  if (trees.ntrees > 0 && (!trees.node_off || !trees.kind || !trees.arg || !trees.const_off))
    throw Error(SRHIP_ERR_INVALID, "null tree arrays");
  CompiledBatch<T> cb;
  const int nt = trees.ntrees;
  cb.ntrees = nt;
  cb.tree_off.assign(nt, -1);
  cb.nodes.assign(nt, 0);
  cb.static_fail.assign(nt, 0);
  cb.fail_if_rows.assign(nt, 0);
  cb.need.assign(nt, 0);
  cb.len.assign(nt, 0);
  cb.cost.assign(nt, 0);
  cb.direct.assign(nt, 0);
  cb.expr.assign(nt, 0);
  const T* consts = static_cast<const T*>(trees.consts);
  TreeCompiler<T> tc;
  tc.out = &cb.code;
  tc.cmap = &cb.cmap;
  tc.folds = &cb.folds;
  tc.grad = grad;
  std::vector<int> stk;
  for (int t = 0; t < nt; ++t) {
    const int b = trees.node_off[t], e = trees.node_off[t + 1];
    const int cb0 = trees.const_off[t], ce = trees.const_off[t + 1];
    if (e <= b) throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + " is empty");
    if (ce < cb0) throw Error(SRHIP_ERR_INVALID, "bad const_off");
    tc.nd.assign(e - b, HNode{});
    tc.fold_fail = false;
    tc.emitted_xop = false;
    bool has_xop = false;
    int tree_max_feat = -1;
    tc.cbase = cb0;
    tc.nbase = b;
    stk.clear();
    int ci = cb0;
    for (int i = 0; i < e - b; ++i) {
      HNode& x = tc.nd[i];
      x.l = x.r = -1; x.op = 0; x.feat = -1; x.val = 0; x.need = 0; x.cidx = -1; x.xop = nullptr;
      x.cpre = ci - cb0;  // constants before this node (a subtree's first node is a leaf)
      const int kind = trees.kind[b + i];
      const int arg = trees.arg[b + i];
      switch (kind) {
        case SRHIP_NODE_CONST:
          if (ci >= ce) throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + ": more constant leaves than constants");
          x.cidx = ci - cb0;
          x.deg = 0; x.val = (double)consts[ci++]; x.has_feature = false; x.size = 1;
          break;
        case SRHIP_NODE_FEATURE:
          x.deg = 0; x.feat = arg; x.has_feature = true; x.size = 1;
          tc.max_feat = std::max(tc.max_feat, arg);
          tree_max_feat = std::max(tree_max_feat, arg);
          break;
        case SRHIP_NODE_UNARY:
          if (arg >= SRHIP_EXPR_OP_BEGIN) {
            x.xop = tc.xop_of(arg, 1);
            has_xop = true;
          } else if (arg >= SRHIP_NUM_UOPS) {
            throw Error(SRHIP_ERR_UNSUPPORTED, "unknown unary operator id " + std::to_string(arg));
          }
          if (stk.empty()) throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + ": stack underflow");
          x.deg = 1; x.op = arg; x.l = stk.back(); stk.pop_back();
          x.has_feature = tc.nd[x.l].has_feature;
          x.size = 1 + tc.nd[x.l].size;
          break;
        case SRHIP_NODE_BINARY:
          if (arg >= SRHIP_EXPR_OP_BEGIN) {
            x.xop = tc.xop_of(arg, 2);
            has_xop = true;
          } else if (arg >= SRHIP_NUM_BOPS) {
            throw Error(SRHIP_ERR_UNSUPPORTED, "unknown binary operator id " + std::to_string(arg));
          }
          if (stk.size() < 2) throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + ": stack underflow");
          x.deg = 2; x.op = arg;
          x.r = stk.back(); stk.pop_back();
          x.l = stk.back(); stk.pop_back();
          x.has_feature = tc.nd[x.l].has_feature || tc.nd[x.r].has_feature;
          x.size = 1 + tc.nd[x.l].size + tc.nd[x.r].size;
          break;
        default:
          throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + ": bad node kind " + std::to_string(kind));
      }
      stk.push_back(i);
    }
    if (stk.size() != 1) throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + ": postfix stream does not reduce to one root");
    if (ci != ce) throw Error(SRHIP_ERR_INVALID, "tree " + std::to_string(t) + ": constant count mismatch");
    // (the gradient programs' no-mark flag shares the feature field)
    if (has_xop && tree_max_feat >= 0x8000)
      throw Error(SRHIP_ERR_UNSUPPORTED, "expression operators support feature indices below 32768");
    const int root = stk[0];
    cb.nodes[t] = e - b;
    cb.total_nodes += e - b;
    cb.cost[t] = tc.cost(root);

    if (grad) {
      // gradient programs: no folding; a non-finite constant fails statically
      if (ce - cb0 > 255) throw Error(SRHIP_ERR_UNSUPPORTED, "gradients support at most 255 constants per tree");
      if (tc.any_const_nonfinite(root)) {
        cb.static_fail[t] = 1;
        if (!keep_layout) continue;
      }
      cb.need[t] = tc.compute_need(root);
      if (cb.need[t] > kMaxSlots) throw Error(SRHIP_ERR_UNSUPPORTED, "tree needs more than 16 stack slots");
      cb.tree_off[t] = (int32_t)cb.code.size();
      tc.emit(root, 0);
      tc.put(OP_END, 0, 0, T(0));
      cb.len[t] = (int32_t)cb.code.size() - cb.tree_off[t];
      cb.direct[t] = 1;
      cb.expr[t] = tc.emitted_xop ? 1 : 0;
      continue;
    }
    const bool root_is_leaf = tc.nd[root].deg == 0;
    tc.fold(root);
    // keep_layout (programs whose constants change: set_constants patches
    // them in place): a tree that fails statically keeps its code too — its
    // verdict decides its result — so that constants that make it finite
    // again are patched into that code instead of rebuilding the program
    if (tc.fold_fail) {
      cb.static_fail[t] = 1;
      if (!keep_layout) continue;
    } else if (root_is_leaf || tc.nd[root].deg == 0) {
      // a leaf (or folded) root: `deg0_eval` fill/copy + the final array check
      const HNode& r = tc.nd[root];
      if (r.feat < 0 && !std::isfinite(r.val)) {
        cb.fail_if_rows[t] = 1;
        if (!keep_layout) continue;
      }
    } else if (tc.nonroot_const_nonfinite(root)) {
      cb.static_fail[t] = 1;
      if (!keep_layout) continue;
    }
    cb.need[t] = tc.compute_need(root);
    if (cb.need[t] > kMaxSlots) throw Error(SRHIP_ERR_UNSUPPORTED, "tree needs more than 16 stack slots");
    cb.tree_off[t] = (int32_t)cb.code.size();
    tc.emit(root, 0);
    tc.put(OP_END, 0, 0, T(0));
    cb.len[t] = (int32_t)cb.code.size() - cb.tree_off[t];
    // folded values are in the map too (folds); set_constants decides the
    // verdict of a keep_layout tree from its patched immediates
    cb.direct[t] = 1;
    cb.expr[t] = tc.emitted_xop ? 1 : 0;
  }
  cb.max_feature = tc.max_feat;
  // trailing OP_ENDs: the kernels prefetch one instruction past each END and
  // the VGPR-resident-program variant loads kVProgMax + 1 instructions per tree
  for (int i = 0; i <= kVProgMax; ++i) tc.put(OP_END, 0, 0, T(0));
  return cb;
}

template <typename T>
CompiledBatch<T> compile_batch_par(const srhip_trees& trees, bool grad, bool keep_layout) {
  const int nt = trees.ntrees;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int cap = host_thread_cap();  // a device group's members share the 8
  const int nthr = (int)std::min<unsigned>(cap > 0 ? (unsigned)std::min(cap, 8) : 8u, hw);
  if (nt < 2048 || nthr < 2) return compile_batch<T>(trees, grad, keep_layout);
  const int nchunk = nthr;
  std::vector<CompiledBatch<T>> part(nchunk);
  std::vector<std::exception_ptr> err(nchunk);
  std::vector<std::thread> th;
  for (int k = 0; k < nchunk; ++k) {
    th.emplace_back([&, k] {
      try {
        const int t0 = (int)((int64_t)nt * k / nchunk), t1 = (int)((int64_t)nt * (k + 1) / nchunk);
        srhip_trees v = trees;  // a view of trees [t0, t1): the offsets index the shared arrays
        v.ntrees = t1 - t0;
        v.node_off = trees.node_off + t0;
        v.const_off = trees.const_off + t0;
        part[k] = compile_batch<T>(v, grad, keep_layout);
      } catch (...) {
        err[k] = std::current_exception();
      }
    });
  }
  for (auto& t : th) t.join();
  for (auto& e : err)
    if (e) std::rethrow_exception(e);
  // merge: each part ends in the kVProgMax + 1 trailing OP_ENDs, kept once at the end
  CompiledBatch<T> cb;
  cb.ntrees = nt;
  const size_t tail = (size_t)kVProgMax + 1;
  for (int k = 0; k < nchunk; ++k) {
    CompiledBatch<T>& p = part[k];
    const int32_t base = (int32_t)cb.code.size();
    cb.code.insert(cb.code.end(), p.code.begin(), p.code.end() - (k + 1 < nchunk ? (std::ptrdiff_t)tail : 0));
    const int32_t fbase = (int32_t)cb.folds.size();  // this part's fold references move up by fbase
    for (auto it = p.cmap.begin(); it != p.cmap.end() - (k + 1 < nchunk ? (std::ptrdiff_t)tail : 0); ++it)
      cb.cmap.push_back(*it <= -2 ? *it - fbase : *it);
    cb.folds.insert(cb.folds.end(), p.folds.begin(), p.folds.end());
    cb.direct.insert(cb.direct.end(), p.direct.begin(), p.direct.end());
    cb.expr.insert(cb.expr.end(), p.expr.begin(), p.expr.end());
    for (int32_t o : p.tree_off) cb.tree_off.push_back(o < 0 ? o : o + base);
    cb.nodes.insert(cb.nodes.end(), p.nodes.begin(), p.nodes.end());
    cb.static_fail.insert(cb.static_fail.end(), p.static_fail.begin(), p.static_fail.end());
    cb.fail_if_rows.insert(cb.fail_if_rows.end(), p.fail_if_rows.begin(), p.fail_if_rows.end());
    cb.need.insert(cb.need.end(), p.need.begin(), p.need.end());
    cb.len.insert(cb.len.end(), p.len.begin(), p.len.end());
    cb.cost.insert(cb.cost.end(), p.cost.begin(), p.cost.end());
    cb.max_feature = std::max(cb.max_feature, p.max_feature);
    cb.total_nodes += p.total_nodes;
  }
  return cb;
}

template <typename T>
bool eval_fold(const FoldRec& f, const srhip_trees& trees, T* out) {
  T stk[kMaxFoldDepth];
  int sp = 0;
  const T* c = static_cast<const T*>(trees.consts) + f.const_b;
  for (int i = f.node_b; i < f.node_e; ++i) {
    const int arg = trees.arg[i];
    switch (trees.kind[i]) {
      case SRHIP_NODE_CONST:
        if (sp == kMaxFoldDepth) return false;
        stk[sp++] = *c++;
        break;
      case SRHIP_NODE_UNARY:
        if (sp < 1) return false;
        stk[sp - 1] = arg >= SRHIP_EXPR_OP_BEGIN ? expr_op_eval<T>(*expr_op_find(arg, false), stk[sp - 1], T(0))
                                                 : host::unop<T>(arg, stk[sp - 1]);
        if (!std::isfinite(stk[sp - 1])) return false;
        break;
      case SRHIP_NODE_BINARY:
        if (sp < 2) return false;
        stk[sp - 2] = arg >= SRHIP_EXPR_OP_BEGIN
                          ? expr_op_eval<T>(*expr_op_find(arg, false), stk[sp - 2], stk[sp - 1])
                          : host::binop<T>(arg, stk[sp - 2], stk[sp - 1]);
        --sp;
        if (!std::isfinite(stk[sp - 1])) return false;
        break;
      default:
        return false;  // a feature: not a folded subtree
    }
  }
  if (sp != 1) return false;
  *out = stk[0];
  return true;
}

template CompiledBatch<float> compile_batch<float>(const srhip_trees&, bool, bool);
template CompiledBatch<double> compile_batch<double>(const srhip_trees&, bool, bool);
template CompiledBatch<float> compile_batch_par<float>(const srhip_trees&, bool, bool);
template CompiledBatch<double> compile_batch_par<double>(const srhip_trees&, bool, bool);
template bool eval_fold<float>(const FoldRec&, const srhip_trees&, float*);
template bool eval_fold<double>(const FoldRec&, const srhip_trees&, double*);

}  // namespace srhip
