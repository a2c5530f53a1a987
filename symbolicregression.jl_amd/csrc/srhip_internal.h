// srhip_internal.h — device program encoding shared by the host compiler
// (compile.cpp) and the HIP kernels (kernels.hip).
//
// A tree is compiled to an accumulator-machine program. Every instruction is
// wave-uniform: it is fetched with scalar loads and dispatched with a
// uniform branch, so the 64 lanes of a wave never diverge on the program.
// Each instruction operates on R rows per lane at once.
//
// Register model (all per lane, R rows each):
//   acc          the value being computed
//   tmp          the second operand popped from the stack
//   slot[0..D)   spilled partial results (Sethi–Ullman order keeps D small)
// Leaf operands are read directly: X[f] from the LDS row tile, constants
// from the instruction's immediate (an SGPR operand of the VALU op).
#pragma once
#include <stdint.h>

#include "../../include/srhip.h"

namespace srhip {

// ---- opcode layout ---------------------------------------------------------
constexpr int kMaxSlots = 16;
enum : int {
  OP_END = 0,
  OP_LDX = 1,                          // acc = X[f]
  OP_LDC = 2,                          // acc = imm
  OP_PUSH0 = 3,                        // slot[k] = acc
  OP_POP0 = OP_PUSH0 + kMaxSlots,      // tmp = slot[k]
  OP_UN0 = OP_POP0 + kMaxSlots,        // acc = u(acc)
  OP_BIN0 = OP_UN0 + SRHIP_NUM_UOPS,   // acc = b(lhs, rhs), see BinVariant
};

// Operand sources of a binary instruction (lhs, rhs):
enum BinVariant : int {
  V_AX = 0,  // (acc, X[f])
  V_XA,      // (X[f], acc)
  V_AC,      // (acc, imm)
  V_CA,      // (imm, acc)
  V_AT,      // (acc, tmp)
  V_TA,      // (tmp, acc)
  V_XX,      // (X[f], X[g]),  g = integer in imm
  V_XC,      // (X[f], imm)
  V_CX,      // (imm, X[f])
  NUM_VARIANTS
};
constexpr int kNumOpcodes = OP_BIN0 + NUM_VARIANTS * SRHIP_NUM_BOPS;
static_assert(kNumOpcodes <= 256, "opcode must fit in 8 bits");

constexpr int bin_opcode(int variant, int bop) {
  return OP_BIN0 + variant * SRHIP_NUM_BOPS + bop;
}

// Micro-instructions of expression operators (srhip.h "expression operators"),
// dispatched by the OPSET_EXPR kernel variants only: the body of such an
// operator is expanded in line, its computed arguments held in reserved slots.
enum : int {
  OP_LDS0 = kNumOpcodes,           // acc = slot[k] (an argument read by the body)
  OP_MARK = OP_LDS0 + kMaxSlots,   // chk = mark(acc): a computed argument is checked
  kNumOpcodesExpr = OP_MARK + 1,
};
static_assert(kNumOpcodesExpr <= 256, "opcode must fit in 8 bits");

// code word: [7:0] opcode, [15:8] slot index, [31:16] feature index.
// Evaluation programs set bit 15 (kNeedX) on instructions with an X[f]
// operand (LDX and the AX/XA/XX/XC/CX variants): the kernel reads X[f] from
// LDS ahead of the dispatch. Gradient programs use all 8 slot bits for
// constant indices and never set it.
constexpr uint32_t kNeedX = 1u << 15;
// Body instructions of an expression operator carry a no-mark flag: the marks
// of their lossy operands go to a throw-away marker (nothing inside a body is
// checked). Evaluation programs: bit 14 (slot indices stay below 16).
// Gradient programs: bit 31 (their feature index stays below 2^15), and a body
// constant carries kBodyConst in the slot field: the index of no tangent.
constexpr uint32_t kNoMark = 1u << 14;
constexpr uint32_t kNoMarkGrad = 1u << 31;
constexpr int kBodyConst = 255;
constexpr uint32_t make_code(int opc, int slot, int feat) {
  return (uint32_t)opc | ((uint32_t)slot << 8) | ((uint32_t)feat << 16);
}
constexpr bool variant_needs_x(int v) {
  return v == V_AX || v == V_XA || v == V_XX || v == V_XC || v == V_CX;
}
// Longest program (END included) of the VGPR-resident-program kernel
// variant: one instruction per lane, and the dispatch reads one ahead.
constexpr int kVProgMax = 63;

template <typename T>
struct Ins;
template <>
struct alignas(8) Ins<float> {
  uint32_t code;
  float imm;
};
template <>
struct alignas(16) Ins<double> {
  uint32_t code;
  uint32_t pad;
  double imm;
};

// ---- operator properties ------------------------------------------------------
// "lossy" operators can map a non-finite operand to a finite result
// (exp(-Inf) = 0, x/Inf = 0, greater(NaN, 1) = 0, ...). DynamicExpressions
// fails a tree when ANY node value is non-finite at any row (every child
// array is checked, InterfaceDynamicExpressions.jl:43-48). All other
// operators propagate non-finite values, so it is enough to check the
// computed operands of lossy operators plus the root value.
constexpr bool bop_lossy_lhs(int op) {
  return op == SRHIP_BOP_POW || op == SRHIP_BOP_GREATER ||
         op == SRHIP_BOP_LOGICAL_OR || op == SRHIP_BOP_LOGICAL_AND ||
         op == SRHIP_BOP_MAX || op == SRHIP_BOP_MIN;
}
constexpr bool bop_lossy_rhs(int op) {
  return op == SRHIP_BOP_DIV || op == SRHIP_BOP_POW || op == SRHIP_BOP_GREATER ||
         op == SRHIP_BOP_LOGICAL_OR || op == SRHIP_BOP_LOGICAL_AND ||
         op == SRHIP_BOP_MOD || op == SRHIP_BOP_MAX || op == SRHIP_BOP_MIN;
}
constexpr bool uop_lossy(int op) {
  return op == SRHIP_UOP_EXP || op == SRHIP_UOP_TANH || op == SRHIP_UOP_ATAN ||
         op == SRHIP_UOP_ERF || op == SRHIP_UOP_ERFC || op == SRHIP_UOP_SIGN ||
         op == SRHIP_UOP_INV;
}

// ---- operator sets -------------------------------------------------------------
// A kernel variant compiled only with the dispatch cases of a small operator
// set has a shallower dispatch branch tree. The host picks the smallest set
// that contains every operator of the batch.
// OPSET_EXPR: the full set plus the expression operators' micro-instructions
// and no-mark flag; deep kernel variants only.
enum OpSet : int { OPSET_BASIC = 0, OPSET_FULL = 1, OPSET_EXPR = 2 };
constexpr uint32_t kBasicBops = (1u << SRHIP_BOP_ADD) | (1u << SRHIP_BOP_SUB) | (1u << SRHIP_BOP_MUL) |
                                (1u << SRHIP_BOP_DIV);
constexpr uint32_t kBasicUops = (1u << SRHIP_UOP_NEG) | (1u << SRHIP_UOP_SQUARE) | (1u << SRHIP_UOP_CUBE) |
                                (1u << SRHIP_UOP_EXP) | (1u << SRHIP_UOP_ABS) | (1u << SRHIP_UOP_LOG) |
                                (1u << SRHIP_UOP_SQRT) | (1u << SRHIP_UOP_SIN) | (1u << SRHIP_UOP_COS);
constexpr bool opset_has_bop(int set, int op) { return set != OPSET_BASIC || ((kBasicBops >> op) & 1u); }
constexpr bool opset_has_uop(int set, int op) { return set != OPSET_BASIC || ((kBasicUops >> op) & 1u); }

// Stack slots of the ordinary kernel variant; trees needing more (rare:
// < 0.01 % of random trees at maxsize 30) run in the 16-slot variant.
constexpr int kShallowSlots = 2;

// Rough VALU cost per row of each operator (f32), used to balance trees over
// workgroups. Not a correctness input.
constexpr int bop_cost(int op) {
  return op == SRHIP_BOP_DIV ? 12 : op == SRHIP_BOP_POW ? 60 : op == SRHIP_BOP_MOD ? 30 : 2;
}
constexpr int uop_cost(int op) {
  return (op == SRHIP_UOP_NEG || op == SRHIP_UOP_ABS || op == SRHIP_UOP_SQUARE ||
          op == SRHIP_UOP_CUBE || op == SRHIP_UOP_RELU || op == SRHIP_UOP_ROUND ||
          op == SRHIP_UOP_FLOOR || op == SRHIP_UOP_CEIL || op == SRHIP_UOP_SIGN)
             ? 2
             : (op == SRHIP_UOP_EXP || op == SRHIP_UOP_SQRT || op == SRHIP_UOP_INV) ? 14 : 40;
}

// ---- expression-loss programs (srhip_loss_expr_create) ----------------------------
// The loss tree over (ŷ, y, w) compiled to its own small accumulator machine,
// run per row tile in the epilogue of the interpreter kernels (interp.h
// run_loss, grad_interp.h run_loss_dual). Registers, R rows per lane each:
//   acc, tmp, slot[0..kLossSlots)
// Leaves are never pushed: a leaf operand is read by the instruction that uses
// it, from the tile's ŷ / y / w registers or the immediate. A postfix stack of
// at most kLossMaxDepth values needs at most kLossMaxDepth - 1 slots.
constexpr int kLossMaxNodes = 64;
constexpr int kLossMaxDepth = 4;
constexpr int kLossSlots = kLossMaxDepth - 1;
enum : int {
  LOP_END = 0,
  LOP_LD = 1,                            // acc = leaf
  LOP_PUSH0 = 2,                         // slot[k] = acc
  LOP_POP0 = LOP_PUSH0 + kLossSlots,     // tmp = slot[k]
  LOP_UN0 = LOP_POP0 + kLossSlots,       // acc = u(acc)
  LOP_AX0 = LOP_UN0 + SRHIP_NUM_UOPS,    // acc = b(acc, leaf)
  LOP_XA0 = LOP_AX0 + SRHIP_NUM_BOPS,    // acc = b(leaf, acc)
  LOP_TA0 = LOP_XA0 + SRHIP_NUM_BOPS,    // acc = b(tmp, acc)
  kNumLossOpcodes = LOP_TA0 + SRHIP_NUM_BOPS,
};
// code word: [7:0] opcode, [17:16] leaf of LD / AX / XA
enum LossLeaf : int { LEAF_YHAT = 0, LEAF_Y = 1, LEAF_W = 2, LEAF_IMM = 3 };
constexpr uint32_t make_loss_code(int opc, int leaf) { return (uint32_t)opc | ((uint32_t)leaf << 16); }
// instructions of the longest program: one per node, a PUSH and a POP per binary
// node with two computed operands, END
constexpr int kLossMaxIns = kLossMaxNodes + 2 * (kLossMaxNodes / 2) + 1;

// ---- expression operators (srhip_op_expr_create) ----------------------------------
constexpr int kExprOpMaxNodes = 64;
constexpr int kExprOpMaxDepth = 4;

// The name of the main (evaluation) kernel the calling thread launched last:
// set at each launch site, read by srhip_last_kernel_name (bench.py ties a
// rocprofv3 PMC summary to the kernel that ran).
void note_kernel(const char* name);
const char* last_kernel();
// The geometry of the loss tree-code launch the calling thread made last
// (jit.cpp launch; srhip_last_loss_launch): nrg, ntg, tpb, grid, tbig, tsub.
void note_loss_launch(int nrg, int ntg, int tpb, unsigned grid, int tbig, int tsub);
const int* last_loss_launch();

// The most host threads a program build on the calling thread may start
// (0: no cap beyond each builder's own). The members of a device group build
// concurrently and share the builders' budget between them.
int& host_thread_cap();

}  // namespace srhip
