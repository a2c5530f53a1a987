/*
 * srhip.h — C ABI of libsrhip.so, the MI355X-native batched expression
 * evaluation engine behind SymbolicRegression.jl's scoring hot path.
 *
 * Every entry point below replaces (a batched form of) one reference
 * interface; the reference file:line is cited on each declaration
 * (paths relative to the SymbolicRegression.jl v0.15.0 repository).
 *
 * Conventions
 *  - Plain C: pointers + sizes, no C++ exceptions cross this boundary.
 *  - Status codes: SRHIP_OK (0) on success, < 0 on error; the message of the
 *    last error on the calling thread is returned by srhip_last_error().
 *  - SRHIP_ERR_UNSUPPORTED means "this call is outside the engine's
 *    coverage" (unknown operator, unsupported loss / dtype, non-finite X):
 *    the caller is expected to fall back to the reference CPU path.
 *  - All host buffers are owned by the caller. Calls are synchronous: the
 *    results are in the caller's buffers when the call returns.
 *  - A context serialises the calls made through it (one mutex, one stream).
 *    Use one context per host thread for concurrency. A program belongs to
 *    the context that created it, and an evaluation call runs on the
 *    PROGRAM's context: a dataset (read-only device memory once created) is
 *    shared by every context of its device, so threads create their programs
 *    in their own contexts and evaluate them concurrently on one dataset.
 *    A program and a dataset on different devices give SRHIP_ERR_INVALID.
 *    Destroy a dataset only when no call on it is in progress.
 *  - Trees cross the boundary as post-order (postfix) node streams: for a
 *    node, its left subtree, then its right subtree, then the node itself.
 *    Constants are listed separately, in the order of the constant leaves in
 *    that stream, which is DynamicExpressions' get_constants order (leaf
 *    order, left to right; test/test_derivatives.jl:126-150).
 *  - Feature counts: a feature index must fit srhip_trees.arg, so a dataset
 *    has at most 65536 features, and 32768 for trees with expression
 *    operators. The kernels keep a row tile of every feature in LDS; a dataset
 *    whose tile does not fit (from 79 features for the ordinary interpreter
 *    kernels, from 159 for every kernel) runs in the wide interpreter
 *    kernels, which read their feature operands from device memory, with no
 *    tree code unless the program was created with
 *    SRHIP_PROGRAM_WIDE_TREE_CODE (Float32 loss tree code that reads its
 *    features from device memory, below). SRHIP_WIDE (environment, read per call; for tests and
 *    measurements): 1 runs every interpreter pass in the wide kernels and
 *    uses no tree code, 0 answers SRHIP_ERR_UNSUPPORTED for such a dataset
 *    ("row tile of N features does not fit in LDS") as the engine did before
 *    it had them. srhip_last_kernel_name then holds "wide".
 */
#ifndef SRHIP_H
#define SRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRHIP_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------ */
#define SRHIP_OK 0
#define SRHIP_ERR_INVALID (-1)     /* malformed arguments / trees           */
#define SRHIP_ERR_UNSUPPORTED (-2) /* fall back to the reference CPU path  */
#define SRHIP_ERR_DEVICE (-3)      /* HIP runtime failure                  */
#define SRHIP_ERR_NOMEM (-4)       /* host or device allocation failed     */

/* ---- element types (Dataset{T}: src/Dataset.jl:24-34) ------------------ */
#define SRHIP_F32 0
#define SRHIP_F64 1

/* ---- X layouts ---------------------------------------------------------- */
/* Julia's Dataset.X is (nfeatures, n) column-major (src/ProgramConstants.jl:3-5):
 * element (f, i) at X[i*nfeat + f]. FEATURE_MAJOR is element (f, i) at X[f*n + i]. */
#define SRHIP_X_JULIA 0
#define SRHIP_X_FEATURE_MAJOR 1

/* ---- node kinds of the postfix stream ----------------------------------- */
#define SRHIP_NODE_CONST 0   /* Node(; val=c)                               */
#define SRHIP_NODE_FEATURE 1 /* Node(; feature=f); arg = f-1 (0-based)      */
#define SRHIP_NODE_UNARY 2   /* degree-1 node; arg = SRHIP_UOP_*            */
#define SRHIP_NODE_BINARY 3  /* degree-2 node; arg = SRHIP_BOP_*            */

/* ---- operator ids --------------------------------------------------------
 * Semantics follow src/Operators.jl:8-111 after the user-op → safe-op mapping
 * of src/Options.jl:86-120 (binopmap / unaopmap). The Julia shim maps
 * options.operators.binops[i] / unaops[i] to these ids once per Options
 * (srhip_op_lookup gives the id for a Julia function name).            */
#define SRHIP_BOP_ADD 0          /* +, plus            Operators.jl:23-25 */
#define SRHIP_BOP_SUB 1          /* -, sub             :26-28             */
#define SRHIP_BOP_MUL 2          /* *, mult            :29-31             */
#define SRHIP_BOP_DIV 3          /* /, div             :47-49             */
#define SRHIP_BOP_POW 4          /* ^, safe_pow        :38-46             */
#define SRHIP_BOP_GREATER 5      /* greater            :94-99             */
#define SRHIP_BOP_LOGICAL_OR 6   /* logical_or         :104-106           */
#define SRHIP_BOP_LOGICAL_AND 7  /* logical_and        :109-111           */
#define SRHIP_BOP_MOD 8          /* Base.mod (float)   :17                */
#define SRHIP_BOP_MAX 9          /* Base.max (float)                      */
#define SRHIP_BOP_MIN 10         /* Base.min (float)                      */
#define SRHIP_NUM_BOPS 11

#define SRHIP_UOP_NEG 0          /* neg                :90-92             */
#define SRHIP_UOP_SQUARE 1       /* square = x*x       :32-34             */
#define SRHIP_UOP_CUBE 2         /* cube = x*x*x       :35-37             */
#define SRHIP_UOP_EXP 3
#define SRHIP_UOP_ABS 4
#define SRHIP_UOP_LOG 5          /* safe_log           :50-53             */
#define SRHIP_UOP_LOG2 6         /* safe_log2          :54-57             */
#define SRHIP_UOP_LOG10 7        /* safe_log10         :58-61             */
#define SRHIP_UOP_LOG1P 8        /* safe_log1p         :62-65             */
#define SRHIP_UOP_SQRT 9         /* safe_sqrt          :70-73             */
#define SRHIP_UOP_SIN 10
#define SRHIP_UOP_COS 11
#define SRHIP_UOP_TAN 12
#define SRHIP_UOP_SINH 13
#define SRHIP_UOP_COSH 14
#define SRHIP_UOP_TANH 15
#define SRHIP_UOP_ATAN 16
#define SRHIP_UOP_ASINH 17
#define SRHIP_UOP_ACOSH 18       /* safe_acosh         :66-69             */
#define SRHIP_UOP_ATANH_CLIP 19  /* atanh_clip         :14                */
#define SRHIP_UOP_ERF 20
#define SRHIP_UOP_ERFC 21
#define SRHIP_UOP_GAMMA 22       /* gamma (Inf → NaN)  :8-12              */
#define SRHIP_UOP_RELU 23        /* (x+abs(x))/2       :100-102           */
#define SRHIP_UOP_ROUND 24       /* round, ties to even                   */
#define SRHIP_UOP_FLOOR 25
#define SRHIP_UOP_CEIL 26
#define SRHIP_UOP_SIGN 27
#define SRHIP_UOP_INV 28         /* inv(x) = 1/x                          */
#define SRHIP_NUM_UOPS 29

/* ---- elementwise losses (LossFunctions.jl distance losses; r = ŷ - y,
 * docs/src/losses.md:16-80; default L2DistLoss, src/Options.jl:429-431) -- */
#define SRHIP_LOSS_L2 0        /* r^2                                       */
#define SRHIP_LOSS_L1 1        /* |r|                                       */
#define SRHIP_LOSS_LP 2        /* |r|^p,        params[0] = p               */
#define SRHIP_LOSS_HUBER 3     /* |r|<=d ? r^2/2 : d(|r|-d/2), params[0]=d  */
#define SRHIP_LOSS_LOGCOSH 4   /* log(cosh(r)), as log1p(cosh(r) - 1): no cancellation near r = 0 */
#define SRHIP_LOSS_L1EPSINS 5  /* max(0, |r|-eps),  params[0] = eps         */
#define SRHIP_LOSS_L2EPSINS 6  /* max(0, |r|-eps)^2, params[0] = eps        */
#define SRHIP_LOSS_QUANTILE 7  /* r>=0 ? tau*r : (tau-1)*r,  params[0] = tau */
#define SRHIP_LOSS_PERIODIC 8  /* 1 - cos(2πr/c) = 2 sin²(πr/c), params[0] = c */
#define SRHIP_LOSS_LOGITDIST 9 /* -log(4 e^r / (1+e^r)^2)                   */
/* LPDistLoss{n} with an INTEGER n (LPDistLoss(3), not LPDistLoss(3.0)):
 * |r|^n by Julia's T^Integer — Float32 stays Float32 (|r|*|r|*|r| for n = 3,
 * else Float64 power by squaring rounded once), Float64 by compensated power
 * by squaring; params[0] = n, integral with |n| < 2^31 (else INVALID). */
#define SRHIP_LOSS_LPINT 10
/* ---- margin (classification) losses (LossFunctions.jl margin losses on the
 * agreement a = y·ŷ, docs/src/losses.md:226-520): out_loss_sum[t] =
 * Σ w_i·L(y_i·ŷ_i). y is used as given: the reference does not check that it
 * is ±1, and neither does the engine. a is computed in T; the nine losses
 * without a parameter are evaluated in T, the two parametric ones in Float64
 * and rounded once (as the parametric distance losses). The gradient seed is
 * dℓ/dŷ = y·L'(a), L' as LossFunctions.jl defines it. h = max(0, 1 - a). */
#define SRHIP_LOSS_ZEROONE 11         /* a < 0 ? 1 : 0 (-0.0 gives 0); L' = 0            */
#define SRHIP_LOSS_PERCEPTRON 12      /* max(0, -a)                                      */
#define SRHIP_LOSS_LOGITMARGIN 13     /* log1p(exp(-a)) (+Inf where exp overflows)       */
#define SRHIP_LOSS_L1HINGE 14         /* h                                               */
#define SRHIP_LOSS_L2HINGE 15         /* h^2                                             */
#define SRHIP_LOSS_SMOOTHEDL1HINGE 16 /* a >= 1-g ? (0.5/g) h^2 : 1 - g/2 - a, params[0] = g > 0 */
#define SRHIP_LOSS_MODHUBER 17        /* a >= -1 ? h^2 : -4a                             */
#define SRHIP_LOSS_L2MARGIN 18        /* (1 - a)^2                                       */
#define SRHIP_LOSS_EXP 19             /* exp(-a)                                         */
#define SRHIP_LOSS_SIGMOID 20         /* 1 - tanh(a)                                     */
/* a >= q/(q+1) ? 1 - a : (q^q / (q+1)^(q+1)) / a^q; params[0] = q > 0 (else
 * INVALID), integral and below 2^31 (else UNSUPPORTED: the reference raises a
 * DomainError for a negative agreement under a non-integer power, so that case
 * stays with the CPU path). */
#define SRHIP_LOSS_DWDMARGIN 21
#define SRHIP_NUM_LOSSES 22
/* ids from here on are margin losses (a = y·ŷ), below it distance losses (r = ŷ - y) */
#define SRHIP_MARGIN_LOSS_BEGIN 11

/* ---- expression losses: a custom elementwise_loss as an engine tree --------
 * The reference accepts any function as elementwise_loss
 * (src/LossFunctions.jl:17-19: sum(loss.(x, y)) / length(y); :27-31:
 * sum(loss.(x, y, w)) / sum(w)). An expression loss is such a function written
 * as a postfix tree in this header's node format (SRHIP_NODE_*, SRHIP_UOP_*,
 * SRHIP_BOP_*) whose feature leaves are 0: the prediction ŷ, 1: the target y,
 * 2: the weight w. It is registered once (process-wide, immutable, one handle
 * for both element types) and the handle it gets — a loss kind >=
 * SRHIP_EXPR_LOSS_BEGIN — is accepted wherever a loss_kind is taken
 * (srhip_eval_loss, _packed, _batch, _batch_ctx, _rowsets, _batch_rowsets_ctx,
 * srhip_eval_loss_grad, srhip_constopt_options.loss_kind); loss_params is
 * ignored there and may be NULL. For every tree t:
 *   out_ok[t]       = did_succeed of the candidate tree alone; values inside the
 *                     loss expression are never checked, a non-finite loss value
 *                     does not fail the tree (the sum is then non-finite, ok = 1)
 *   out_loss_sum[t] = Σ_i ℓ(ŷ_i, y_i, w_i): NO implicit weight, the reference's
 *                     loss.(x, y, w) contract; ℓ is computed in T with the
 *                     operators' semantics above (safe operators give NaN), its
 *                     constants rounded to T once
 *   out_weight_sum  = Σ w, or the row count when unweighted, as for every loss
 *   out_dloss[c]    = Σ_i (dℓ/dŷ)_i · ∂ŷ_i/∂c, dℓ/dŷ one forward-mode tangent
 *                     through the expression (1 on feature 0, 0 elsewhere) with
 *                     the derivative rules of the constant gradients
 * Limits: at most 64 nodes; at most 4 values live on the postfix stack; finite
 * constants; feature index <= 2; exactly one value left on the stack. A
 * malformed stream is SRHIP_ERR_INVALID; a well-formed one beyond the node or
 * stack limits, or with an operator id beyond the tables, is
 * SRHIP_ERR_UNSUPPORTED (the caller falls back to the CPU path).
 * Deviations from the reference: an expression that reads feature 2 on an
 * unweighted dataset is SRHIP_ERR_INVALID, and one that ignores feature 2 is
 * allowed on a weighted dataset (the reference would call a 2-argument function
 * with 3 arguments there); Julia promotes Float32 ^ 2.5 (a Float64 literal) to
 * Float64, the engine stays in T. These kinds always run in the interpreter
 * kernels (no tree code: srhip_last_tree_code gives 0, and the
 * srhip_jit_compile_loss hook answers SRHIP_ERR_UNSUPPORTED for them). */
#define SRHIP_EXPR_LOSS_BEGIN 1024 /* loss kinds from here on are handles of expression losses */
/* consts[nconsts]: the constant leaves in stream order (as srhip_trees). */
int32_t srhip_loss_expr_create(const uint8_t* kind, const uint16_t* arg, int32_t nnodes,
                               const double* consts, int32_t nconsts, int32_t* out_loss_kind);
/* A destroyed (or never registered) kind >= SRHIP_EXPR_LOSS_BEGIN is
 * SRHIP_ERR_INVALID everywhere; handles are not reused. */
int32_t srhip_loss_expr_destroy(int32_t loss_kind);
/* Host statement of the semantics, no device: out[i] = ℓ(yhat[i], y[i],
 * w ? w[i] : unused) in dtype T (arrays of T), with the host routines that
 * constant folding and srhip_op_eval use. w == NULL with an expression that
 * reads feature 2 is SRHIP_ERR_INVALID. */
int32_t srhip_loss_expr_eval(int32_t loss_kind, int32_t dtype, const void* yhat, const void* y,
                             const void* w, int64_t n, void* out);

/* ---- expression operators: a custom operator as an engine tree ---------------
 * The reference accepts any Julia function in binary_operators /
 * unary_operators (test/test_custom_operators.jl: op2(x, y) = x^2 + 1/(y^2 + 0.1),
 * op3(x) = sin(x) + cos(x)). An expression operator is such a function written
 * as a postfix tree in this header's node format over the operators above,
 * whose feature leaves are 0: the first argument, 1: the second. It is
 * registered once (process-wide, immutable, one handle for both element types);
 * the handle — an operator id >= SRHIP_EXPR_OP_BEGIN — goes in srhip_trees.arg
 * of a SRHIP_NODE_UNARY / SRHIP_NODE_BINARY node wherever an operator id goes,
 * and srhip_op_eval accepts it (the host statement of the semantics). These are
 * the reference's semantics for an opaque function:
 *   1. the value is the body evaluated in T with the operators' semantics above
 *      (safe operators give NaN), body constants rounded to T once;
 *   2. the arguments are checked: a non-finite argument value fails the tree, as
 *      the reference checks every child array;
 *   3. nothing inside the body is checked: inv(exp(x)) where exp overflows gives
 *      0 and the tree succeeds (the same tree written with primitives fails);
 *   4. a non-finite result fails the tree as any operator's does;
 *   5. the node counts as one node (srhip_program_info);
 *   6. in the static rules of the enclosing tree it is an ordinary operator of
 *      its arity: a feature-free subtree holding it is folded, the result
 *      checked once at the operator's output; the rules for non-finite constant
 *      leaves apply to its arguments.
 * Body constants are fixed: they are no constants of the tree (no entry in
 * consts, no gradient). Limits: at most 64 nodes; at most 4 values live on the
 * postfix stack; finite constants; feature index below the arity; primitives
 * only (no expression operator inside a body). A malformed stream, a non-finite
 * constant or a feature index beyond the arity is SRHIP_ERR_INVALID; a well-formed
 * stream beyond the node or stack limits or with an operator id beyond the tables
 * is SRHIP_ERR_UNSUPPORTED. In a tree, an operator id that was never handed out
 * is SRHIP_ERR_UNSUPPORTED, a destroyed handle SRHIP_ERR_INVALID, a handle of
 * the wrong arity for its node kind SRHIP_ERR_INVALID, and a tree whose expansion
 * needs more than 16 stack slots SRHIP_ERR_UNSUPPORTED. Feature indices of such
 * a tree stay below 32768. A program holds the definitions it uses: destroying a
 * handle does not disturb programs that exist. Deviation from the reference, as
 * for expression losses: a Float64 literal in a Julia body promotes a Float32
 * argument to Float64, the engine stays in T. Trees whose program holds such an
 * operator always run in the 16-slot interpreter kernels (no tree code: the
 * srhip_jit_compile* hooks leave them out); the other trees of the program keep
 * their kernels. */
#define SRHIP_EXPR_OP_BEGIN 1024 /* operator ids from here on are handles of expression operators */
/* arity 1 or 2; consts[nconsts]: the constant leaves in stream order. */
int32_t srhip_op_expr_create(int32_t arity, const uint8_t* kind, const uint16_t* arg, int32_t nnodes,
                             const double* consts, int32_t nconsts, int32_t* out_op_id);
/* Handles are not reused. */
int32_t srhip_op_expr_destroy(int32_t op_id);

typedef struct srhip_ctx srhip_ctx;
typedef struct srhip_dataset srhip_dataset;
typedef struct srhip_program srhip_program;

/* A batch of trees as postfix node streams (see header comment). */
typedef struct srhip_trees {
  int32_t ntrees;
  const int32_t* node_off;  /* [ntrees+1]: nodes of tree t are node_off[t] .. node_off[t+1]-1 */
  const uint8_t* kind;      /* [node_off[ntrees]] SRHIP_NODE_*                                  */
  const uint16_t* arg;      /* [node_off[ntrees]] feature (0-based) or operator id              */
  const int32_t* const_off; /* [ntrees+1]: constants of tree t                                   */
  const void* consts;       /* [const_off[ntrees]] of the program dtype                          */
} srhip_trees;

/* ---- library / context ------------------------------------------------- */
int32_t srhip_version(void);
const char* srhip_last_error(void);
int32_t srhip_device_count(int32_t* out_count);
int32_t srhip_open(int32_t device, srhip_ctx** out_ctx);
int32_t srhip_close(srhip_ctx* ctx);

/* Operator table: id and arity (1 or 2) for a Julia operator name
 * ("+", "*", "safe_log", "log", "cos", "^", ...), applying binopmap/unaopmap
 * (src/Options.jl:86-120). Unknown → SRHIP_ERR_UNSUPPORTED. */
int32_t srhip_op_lookup(const char* name, int32_t* out_arity, int32_t* out_id);

/* One operator on scalars of the program dtype (SRHIP_F32 / SRHIP_F64), with
 * the engine's semantics (the same host routines its compiler folds
 * constant subtrees with: Operators.jl:8-111, Float32 transcendentals
 * evaluated in double and rounded once). For the host callers that fold
 * constants themselves — DynamicExpressions' `simplify_tree` /
 * `combine_operators`, used by optimize_and_simplify_population
 * (src/SingleIteration.jl:73-74) and the :simplify mutation
 * (src/Mutate.jl:107-109). b is ignored for arity 1. No device work. */
int32_t srhip_op_eval(int32_t dtype, int32_t arity, int32_t id, double a, double b,
                      double* out);

/* The symbol name of the main evaluation kernel the calling thread launched
 * last ("sr_jit_eval_dlp", "eval_kernel<float>", "sr_jit_grad_dl", ...), as
 * rocprofv3 reports it: ties a profile to the kernel that ran (bench.py). */
int32_t srhip_last_kernel_name(char* buf, int32_t len);

/* The geometry of the loss tree-code launch the calling thread made last:
 * out6 = {row groups, tree groups, trees per group, workgroups launched, first
 * row group whose tree groups are split over several workgroups (= row groups:
 * none), workgroups per tree group there (1: none)}; zeros before any. */
int32_t srhip_last_loss_launch(int32_t* out6);

/* ---- dataset: Dataset(X, y; weights) src/Dataset.jl:43-64 ----------------
 * Uploads rows [row_begin, row_end) of X / y / w once (the row shard of this
 * device); X is transposed to feature-major on the device. w may be NULL
 * (unweighted). The dataset is immutable after creation. */
int32_t srhip_dataset_create(srhip_ctx* ctx, int32_t dtype, int32_t x_layout,
                             const void* X, const void* y, const void* w,
                             int64_t n, int32_t nfeat, int64_t row_begin,
                             int64_t row_end, srhip_dataset** out_ds);
int32_t srhip_dataset_destroy(srhip_dataset* ds);
/* rows of this shard, Σw (or the row count), Σ y·w (or Σ y) over the shard —
 * the pieces of avg_y (src/Dataset.jl:56-60) — and whether X is all-finite. */
int32_t srhip_dataset_info(const srhip_dataset* ds, int64_t* out_rows,
                           int32_t* out_nfeat, double* out_sum_w,
                           double* out_sum_yw, int32_t* out_x_finite);

/* ---- programs: a compiled, device-resident batch of trees ---------------
 * Flattens/compiles the postfix streams (register allocation, leaf fusion,
 * static constant checks) and uploads them once; evaluate any number of
 * times afterwards. */
int32_t srhip_program_create(srhip_ctx* ctx, int32_t dtype,
                             const srhip_trees* trees, srhip_program** out_prog);
/* srhip_program_create with flags. SRHIP_PROGRAM_VARYING_CONSTANTS: the
 * caller will set new constants (srhip_program_set_constants, the candidates
 * of `optimize_constants`, src/ConstantOptimization.jl:12-19): Float32 tree
 * code is built reading its constants from memory from the start, so no
 * constant set ever recompiles it (without the flag the first set does). */
#define SRHIP_PROGRAM_VARYING_CONSTANTS 1u
/* SRHIP_PROGRAM_INTERPRETED: build no loss / output tree code (the program is
 * scored only on per-tree row sets, srhip_eval_loss_rowsets, which run in the
 * interpreter: a large batch then skips the code generation and load). */
#define SRHIP_PROGRAM_INTERPRETED 2u
/* SRHIP_PROGRAM_WIDE_TREE_CODE (opt-in): Float32 literal-constant loss tree
 * code may read its features from X in device memory. When a tree-code
 * candidate of the program reads a feature index >= 63 (past the LDS tile's
 * reach) the program's loss code is built wide: its LDS tile holds y and w
 * only, so it runs on a dataset of any width, and with the flag a program's
 * tree code stays in use when an interpreter pass of the call has to run wide
 * (without it such a call runs wholly in the wide interpreter). Per-row
 * outputs, per-tree row sets and targets of a program with wide code run in
 * the interpreter, and so does the program after srhip_program_set_constants.
 * No effect on Float64 programs, with SRHIP_PROGRAM_INTERPRETED or with
 * SRHIP_PROGRAM_VARYING_CONSTANTS (memory-constant code is never wide). */
#define SRHIP_PROGRAM_WIDE_TREE_CODE 4u
int32_t srhip_program_create_ex(srhip_ctx* ctx, int32_t dtype, const srhip_trees* trees, uint32_t flags,
                                srhip_program** out_prog);
int32_t srhip_program_destroy(srhip_program* prog);
/* per-tree node counts (count_nodes, = compute_complexity without a custom
 * complexity mapping, src/Complexity.jl:13-19) */
int32_t srhip_program_info(const srhip_program* prog, int32_t* out_ntrees,
                           int64_t* out_total_nodes, int32_t* out_nodes /*[ntrees] or NULL*/);
/* Replace the constants of every tree (set_constants, in get_constants
 * order) without recompiling; used by batched constant optimisation
 * (src/ConstantOptimization.jl:12-19). consts has const_off[ntrees] entries. */
int32_t srhip_program_set_constants(srhip_program* prog, const void* consts);

/* ---- batched loss: eval_loss / _eval_loss src/LossFunctions.jl:34-67 ----
 * For every tree t:
 *   out_loss_sum[t] = Σ_i w_i · ℓ(ŷ_t,i, y_i) over the shard (fp64)
 *   out_ok[t]       = did_succeed of eval_tree_array (1/0)
 *   *out_weight_sum = Σ_i w_i (or the row count when unweighted)
 * The reference loss is out_loss_sum[t] / *out_weight_sum computed in T, and
 * T(Inf) when !out_ok[t] (src/LossFunctions.jl:36-38). row_idx (NULL = all
 * rows) selects rows with repetition, as score_func_batch does
 * (src/LossFunctions.jl:95-115); indices are 0-based within the shard.
 * Trees whose evaluation fails get out_loss_sum = NaN. */
int32_t srhip_eval_loss(srhip_dataset* ds, const srhip_program* prog,
                        int32_t loss_kind, const double* loss_params,
                        const int64_t* row_idx, int64_t nidx,
                        double* out_loss_sum, double* out_weight_sum,
                        uint8_t* out_ok);
/* Row shards (config #5, src/ConstantOptimization.jl:43 with the rows split
 * over GPUs): srhip_eval_loss's per-tree partials written to DEVICE memory
 * for a device-side all-reduce (RCCL), no host round trip:
 *   d_out[2t]      = Σ_i w_i ℓ(ŷ_t,i, y_i) over the shard (0 if t failed)
 *   d_out[2t + 1]  = 1 if t failed on the shard (did_succeed false), else 0
 *   d_out[2·ntrees] = Σ_i w_i (the row count when unweighted)
 * d_out holds 2·ntrees + 1 doubles on the context's device. Asynchronous:
 * enqueued on the context's stream; srhip_sync(ctx) before another stream
 * or the host reads d_out. Summed over shards: loss = ΣΣ/ΣΣw, did_succeed =
 * (Σ failed == 0). */
int32_t srhip_eval_loss_packed(srhip_dataset* ds, srhip_program* prog, int32_t loss_kind,
                               const double* loss_params, double* d_out);

/* Convenience: srhip_program_create + srhip_eval_loss + destroy (the program
 * in the dataset's context). */
int32_t srhip_eval_loss_batch(srhip_dataset* ds, const srhip_trees* trees,
                              int32_t loss_kind, const double* loss_params,
                              const int64_t* row_idx, int64_t nidx,
                              double* out_loss_sum, double* out_weight_sum,
                              uint8_t* out_ok);
/* The same with the program in `ctx` (a context of the dataset's device):
 * one context per host thread scores that thread's candidates concurrently
 * with the others on one shared dataset (SearchUtils.jl:33-45, one
 * Threads.@spawn per island). */
int32_t srhip_eval_loss_batch_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                  int32_t loss_kind, const double* loss_params,
                                  const int64_t* row_idx, int64_t nidx,
                                  double* out_loss_sum, double* out_weight_sum,
                                  uint8_t* out_ok);

/* ---- per-tree minibatches: score_func_batch src/LossFunctions.jl:95-115 ----
 * The reference draws a fresh sample of batch_size rows (with replacement,
 * :98) for EVERY call, i.e. for every candidate it scores (src/Mutate.jl:41-47
 * parents, :199-205 babies). This scores every tree of the program on its own
 * sample in ONE launch: row_idx is [ntrees][batch_size] (0-based within the
 * shard, repetition allowed), tree t evaluated on rows row_idx[t][0..bs).
 *   out_loss_sum[t]   = Σ_k w_{idx[t][k]} · ℓ(ŷ_t, y) over tree t's sample
 *   out_weight_sum[t] = Σ_k w_{idx[t][k]} (batch_size when unweighted)
 *   out_ok[t]         = did_succeed on that sample
 * The loss is out_loss_sum[t] / out_weight_sum[t] in T (Inf if !ok), as
 * srhip_eval_loss. Runs in the interpreter (one tree per workgroup over its
 * gathered sample). */
int32_t srhip_eval_loss_rowsets(srhip_dataset* ds, const srhip_program* prog,
                                int32_t loss_kind, const double* loss_params,
                                const int64_t* row_idx, int64_t batch_size,
                                double* out_loss_sum, double* out_weight_sum,
                                uint8_t* out_ok);
/* Convenience: program (SRHIP_PROGRAM_INTERPRETED) in ctx (NULL = the
 * dataset's context) + srhip_eval_loss_rowsets + destroy — Julia's batched
 * score_func_batch over a vector of candidates. */
int32_t srhip_eval_loss_batch_rowsets_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                          int32_t loss_kind, const double* loss_params,
                                          const int64_t* row_idx, int64_t batch_size,
                                          double* out_loss_sum, double* out_weight_sum,
                                          uint8_t* out_ok);

/* ---- multi-output datasets: one X, a target per tree --------------------------
 * EquationSearch(X, y::AbstractMatrix) builds nout Datasets over the same X
 * (src/SymbolicRegression.jl:304-315) and scores the candidates of all outputs
 * in one loop (:459-494). A multi-target dataset holds X once with ntargets
 * target columns, each with its own optional weight column. It is scored in two
 * ways:
 *   views      srhip_dataset_view(ds, k): target k as an ordinary single-target
 *              dataset on the parent's device memory (no copy). Every entry point
 *              takes a view and runs the kernels it runs on a dataset made of
 *              (X, Y[k], W[k]) by srhip_dataset_create, with the same results.
 *   fused      srhip_eval_loss_targets and its forms: the trees of one program each
 *              carry a target index and one launch scores every tree against its
 *              own column.
 * Rules:
 *   - ntargets outside 1..SRHIP_MAX_TARGETS, or a null Y, is SRHIP_ERR_INVALID,
 *     answered before any device work (and before ctx is looked at).
 *   - a target[t] outside 0..ntargets-1 is SRHIP_ERR_INVALID; nothing is written.
 *   - a dataset with ntargets > 1 passed to a single-target entry point (every
 *     entry point above and below that takes a srhip_dataset, the constant
 *     optimiser included) is SRHIP_ERR_INVALID; the message says to take a view.
 *   - with ntargets == 1 the dataset is an ordinary dataset everywhere.
 *   - the fused calls accept every table loss, distance and margin; an
 *     expression-loss handle is SRHIP_ERR_UNSUPPORTED there in this version
 *     (views take it).
 *   - out_ok and out_loss_sum mean what they mean for srhip_eval_loss with
 *     (y, w) = (Y[target[t]], W[target[t]]); a failed tree has a NaN sum.
 *   - srhip_dataset_info's x_finite, rows and nfeat refer to the shared X; the Σw
 *     and Σ y·w of target k come from srhip_dataset_target_info.
 *   - the fused calls always run in the interpreter kernels (variants of their
 *     own whose row tile holds every column; the wide variant when that tile does
 *     not fit in LDS): srhip_last_tree_code gives 0. Callers with large batches
 *     per target score them on views, which run tree code.
 * Not in this version: fused gradients and fused constant optimisation through
 * these scoring calls or the single-target entry points (srhip_eval_loss_grad and
 * srhip_optimize_constants_batch take views): see srhip_eval_loss_grad_targets and
 * srhip_optimize_constants_targets below, which carry a target per tree;
 * expression losses in the fused calls; multi-target group datasets (a device
 * group takes one srhip_group_dataset per target). */
#define SRHIP_MAX_TARGETS 16
/* Y: [ntargets][n] (target-major); W: NULL or [ntargets][n]. Rows [row_begin,row_end) as srhip_dataset_create. */
int32_t srhip_dataset_create_multi(srhip_ctx* ctx, int32_t dtype, int32_t x_layout, const void* X, const void* Y,
                                   const void* W, int64_t n, int32_t nfeat, int32_t ntargets,
                                   int64_t row_begin, int64_t row_end, srhip_dataset** out_ds);
int32_t srhip_dataset_targets(const srhip_dataset* ds, int32_t* out_ntargets); /* 1 for every other dataset */
int32_t srhip_dataset_target_info(const srhip_dataset* ds, int32_t k, double* out_sum_w, double* out_sum_yw);
/* single-target dataset on the parent's X / Y[k] / W[k]; no copy. Parent and views may be destroyed
 * (srhip_dataset_destroy) in any order: device memory goes with the last of them. */
int32_t srhip_dataset_view(srhip_dataset* ds, int32_t k, srhip_dataset** out_view);
/* srhip_eval_loss with tree t scored against column target[t]; out_weight_sum is [ntargets]. */
int32_t srhip_eval_loss_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                const double* loss_params, const int32_t* target, double* out_loss_sum,
                                double* out_weight_sum, uint8_t* out_ok);
/* srhip_program_create_ex(SRHIP_PROGRAM_INTERPRETED) + srhip_eval_loss_targets + destroy, the program in ctx
 * (NULL: the dataset's context). */
int32_t srhip_eval_loss_batch_targets_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                          int32_t loss_kind, const double* loss_params, const int32_t* target,
                                          double* out_loss_sum, double* out_weight_sum, uint8_t* out_ok);
/* srhip_eval_loss_rowsets with a target per tree (row_idx [ntrees][batch_size]; out_weight_sum [ntrees]). */
int32_t srhip_eval_loss_rowsets_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                        const double* loss_params, const int32_t* target, const int64_t* row_idx,
                                        int64_t batch_size, double* out_loss_sum, double* out_weight_sum,
                                        uint8_t* out_ok);

/* ---- per-row outputs: eval_tree_array src/InterfaceDynamicExpressions.jl:50-52
 * out is [ntrees][rows] of the dataset dtype (row-major per tree); rows of a
 * failed tree are unspecified (the reference returns an undef array). */
int32_t srhip_eval_tree_array(srhip_dataset* ds, const srhip_program* prog,
                              void* out, uint8_t* out_ok);

/* ---- constant gradients: eval_grad_tree_array(tree, X, options;
 * variable=false) src/InterfaceDynamicExpressions.jl:105-107, fused with the
 * loss: out_dloss[c] = Σ_i w_i ∂ℓ(ŷ_i, y_i)/∂c for every constant c of every
 * tree (laid out like consts, const_off order). Also returns the loss sums
 * and did_succeed like srhip_eval_loss.
 *
 * Derivative rules: the textbook ones for every operator (DESIGN.md §3.4 lists
 * them with the conventions at kinks, ties and poles), each pinned to an
 * independent high-precision reference (tests/golden/derivatives.npz). The
 * piecewise-constant operators (greater, logical_or, logical_and, round, floor,
 * ceil, sign) have derivative 0 everywhere.
 * DEVIATION from the reference: SRHIP_UOP_GAMMA's rule, Γ(x)·ψ(x), is not
 * provided (no device digamma): its derivative is taken as 0, so every
 * constant below a gamma node gets gradient 0 through it and a gradient-based
 * optimiser will not move it. Optimise such trees with Nelder-Mead
 * (srhip_constopt_options) or on the CPU. */
int32_t srhip_eval_loss_grad(srhip_dataset* ds, const srhip_program* prog,
                             int32_t loss_kind, const double* loss_params,
                             double* out_loss_sum, double* out_dloss,
                             double* out_weight_sum, uint8_t* out_ok);

/* ---- constant gradients on per-tree minibatches ------------------------------
 * srhip_eval_loss_grad with tree t on its own sample: row_idx [ntrees][batch_size], 0-based within the
 * shard, repetition allowed. out_weight_sum is [ntrees]. Rules as srhip_eval_loss_rowsets:
 *   out_loss_sum[t]   = Σ_k w_{idx[t][k]} · ℓ(ŷ_t, y) over tree t's sample (NaN if !ok)
 *   out_dloss[c]      = Σ_k w_{idx[t][k]} · ∂ℓ/∂c for every constant c of tree t (NaN if !ok)
 *   out_weight_sum[t] = Σ_k w_{idx[t][k]} (batch_size when unweighted)
 *   out_ok[t]         = did_succeed on that sample
 * Every loss kind srhip_eval_loss_grad takes is accepted, with the same rule for
 * expression losses that read w. Answered before any launch with
 * SRHIP_ERR_INVALID: a null row_idx with ntrees·batch_size > 0, an index outside
 * [0, rows), a negative batch_size, a dataset with several targets (take a view).
 * Runs in the forward-mode interpreter, one (tree, tangent group) per workgroup
 * over the tree's gathered sample, with the tiles, lane sums and row-group sum of
 * a dataset made of that sample: the results equal srhip_eval_loss_grad's on such
 * a dataset bit for bit. Gradient tree code is never used (srhip_last_tree_code
 * gives 0) and none is built for such a call; srhip_last_kernel_name gives
 * "grad_kernel_seg<float>" and its kin. */
int32_t srhip_eval_loss_grad_rowsets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                     const double* loss_params, const int64_t* row_idx, int64_t batch_size,
                                     double* out_loss_sum, double* out_dloss, double* out_weight_sum,
                                     uint8_t* out_ok);

/* ---- constant gradients with a target per tree --------------------------------
 * srhip_eval_loss_grad and srhip_eval_loss_grad_rowsets on a multi-target dataset
 * (srhip_dataset_create_multi), tree t against column target[t]:
 *   out_loss_sum[t], out_dloss[c], out_ok[t] mean what they mean for the plain call
 *     with (y, w) = (Y[target[t]], W[target[t]]); a failed tree has a NaN sum and
 *     NaN gradients;
 *   out_weight_sum is [ntargets] (Σ w of every column) for srhip_eval_loss_grad_targets
 *     and [ntrees] (Σ w of tree t's sample in its column) with row sets.
 * Rules, all answered before any launch and before anything is written: those of
 * srhip_eval_loss_targets (a null target with ntrees > 0 or a target outside
 * 0..ntargets-1 is SRHIP_ERR_INVALID; an expression-loss handle is
 * SRHIP_ERR_UNSUPPORTED: take a view) and, with row sets, those of
 * srhip_eval_loss_grad_rowsets. A single-target dataset is accepted; its targets
 * are all 0.
 * Always the forward-mode interpreter, never gradient tree code
 * (srhip_last_tree_code gives 0; none is built for such a call). Over all rows the
 * kernel variants are their own ("grad_kernel_targets<float>",
 * "grad_kernel_wide_targets<float>" and the double forms): the row tile holds every
 * column of Y (and of W), and the wide variant runs when that tile does not fit in
 * LDS. With one column an item's arithmetic is srhip_eval_loss_grad's in the
 * interpreter, bit for bit. With row sets the gather takes each tree's rows from
 * its own column and the launch is srhip_eval_loss_grad_rowsets' ("grad_kernel_seg<float>"
 * and its kin): the results equal that call's on a view of target[t], bit for bit.
 * Not in this version: expression losses; multi-target group datasets; staging
 * only the columns that a launch's work items use (every column is staged). */
int32_t srhip_eval_loss_grad_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                     const double* loss_params, const int32_t* target, double* out_loss_sum,
                                     double* out_dloss, double* out_weight_sum, uint8_t* out_ok);
int32_t srhip_eval_loss_grad_rowsets_targets(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                             const double* loss_params, const int32_t* target,
                                             const int64_t* row_idx, int64_t batch_size, double* out_loss_sum,
                                             double* out_dloss, double* out_weight_sum, uint8_t* out_ok);

/* ---- derivative objectives: fused losses on ŷ and ∂ŷ/∂x --------------------------
 * One table loss reduced on the prediction and on its derivatives with respect to
 * ndir features, for every tree of a program in one pass ("a loss that takes into
 * account derivatives", src/Options.jl:203-210; eval_diff_tree_array /
 * eval_grad_tree_array(...; variable=true) on the host).
 * ds is a dataset of srhip_dataset_create_multi with ntargets = 1 + ndir columns:
 * column 0 is y, column 1 + k the target of ∂ŷ/∂x_dir[k] (each with its own weight
 * column when the dataset is weighted). dir holds 0-based feature indices.
 *   out_loss_sum[t][0]     = Σ_i W[0][i] · ℓ(ŷ_t(x_i), Y[0][i])
 *   out_loss_sum[t][1 + k] = Σ_i W[1+k][i] · ℓ(∂ŷ_t/∂x_dir[k](x_i), Y[1+k][i])
 *   out_weight_sum[c]      = Σ_i W[c][i] (rows when unweighted), c < 1 + ndir
 *   out_ok[t]              = did_succeed of the tree's value evaluation
 * ℓ takes the derivative in the prediction's place. The engine's rule for the
 * flag is the one its eval_diff_tree_array follows: only the value evaluation is
 * checked, so a non-finite derivative gives a non-finite channel sum with ok = 1
 * (the expression losses' rule), and a failed tree's whole row is NaN. Parity with
 * DynamicExpressions' own completion flag for derivatives is unpinned.
 * Answered before any launch and before anything is written: a null dir with
 * ndir > 0, an ndir outside 1..15, ds->ntargets != 1 + ndir, a direction outside
 * 0..nfeat-1, a repeated direction and a margin loss (loss_kind >=
 * SRHIP_MARGIN_LOSS_BEGIN) are SRHIP_ERR_INVALID; an expression-loss handle and a
 * program that holds expression operators are SRHIP_ERR_UNSUPPORTED. The loss
 * kind and its parameter are checked as everywhere.
 * Always the forward-mode interpreter with tangents seeded at feature leaves, in
 * kernel variants of its own ("grad_kernel_deriv<float>",
 * "grad_kernel_wide_deriv<float>" and the double forms; the wide one when the row
 * tile of every feature and column does not fit in LDS). One work item per tree
 * when ndir <= 2, one per group of 4 directions otherwise. srhip_last_tree_code
 * gives 0 and no tree code is built for such a call (the one-shot form makes its
 * program with SRHIP_PROGRAM_INTERPRETED). srhip_last_loss_launch gives the row
 * groups, tree groups and items per group of the call's last launch.
 * The sums' gradients with respect to the constants and constant optimisation under
 * the objective are srhip_eval_loss_grad_deriv and srhip_optimize_constants_deriv below.
 * Not in this version: row sets; group datasets; expression losses and expression
 * operators; tree code. */
int32_t srhip_eval_loss_deriv(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                              const double* loss_params, const int32_t* dir, int32_t ndir,
                              double* out_loss_sum,   /* [ntrees][1 + ndir] */
                              double* out_weight_sum, /* [1 + ndir]: Σw of each column, or rows */
                              uint8_t* out_ok);
int32_t srhip_eval_loss_deriv_batch_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                        int32_t loss_kind, const double* loss_params, const int32_t* dir,
                                        int32_t ndir, double* out_loss_sum, double* out_weight_sum,
                                        uint8_t* out_ok);

/* ---- derivative objectives: constant gradients (∂²ŷ/∂c∂x) ------------------------
 * srhip_eval_loss_deriv's sums and their derivatives with respect to every constant,
 * one launch for every channel (ds, dir, ndir, loss as there):
 *   out_loss_sum[t][c]     as srhip_eval_loss_deriv gives it, bit for bit
 *   out_grad_sum[j][0]     = Σ_i W[0][i] · ℓ'(ŷ_t(x_i), Y[0][i]) · ∂ŷ_t/∂c_j(x_i)
 *   out_grad_sum[j][1 + k] = Σ_i W[1+k][i] · ℓ'(d_k(x_i), Y[1+k][i]) · ∂d_k/∂c_j(x_i)
 * with d_k = ∂ŷ_t/∂x_dir[k], j over the constants of all trees in order (tree t's are
 * const_off[t] .. const_off[t+1]-1) and ℓ' the loss's derivative in its first
 * argument. ∂d_k/∂c_j comes from second-order forward mode over the gradient
 * programs: every operator's second partials are the derivatives of its first-order
 * rules as written (so a piecewise-constant rule, and gamma's missing one, give 0;
 * safe_pow's ∂/∂y branch for x <= 0 gives fxy = fyy = 0).
 * The flag is srhip_eval_loss_deriv's: ok is did_succeed of the value evaluation; a
 * non-finite derivative or mixed partial gives non-finite sums with ok = 1; a failed
 * tree's rows of both outputs are NaN.
 * A work item is (tree, direction, group of constants) in two words: up to 2^24
 * trees, 256 constant groups of 1 or 2 constants per tree (more than a gradient
 * program's 254 constants), any ndir within srhip_eval_loss_deriv's 1..15.
 * Refusals are srhip_eval_loss_deriv's, before any launch with the outputs untouched,
 * and one more: there is no wide variant, so a dataset whose row tile of every
 * feature and column does not fit in LDS (or SRHIP_WIDE=1) is SRHIP_ERR_UNSUPPORTED.
 * Kernel variants of their own ("grad_kernel_deriv2<float>" / "<double>");
 * srhip_last_tree_code gives 0.
 * Not in this version: the wide variant; margin and expression losses; expression
 * operators; row sets; group datasets; tree code. */
int32_t srhip_eval_loss_grad_deriv(srhip_dataset* ds, const srhip_program* prog, int32_t loss_kind,
                                   const double* loss_params, const int32_t* dir, int32_t ndir,
                                   double* out_loss_sum,   /* [ntrees][1 + ndir] */
                                   double* out_grad_sum,   /* [const_off[ntrees]][1 + ndir] */
                                   double* out_weight_sum, /* [1 + ndir] */
                                   uint8_t* out_ok);
int32_t srhip_eval_loss_grad_deriv_batch_ctx(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                             int32_t loss_kind, const double* loss_params, const int32_t* dir,
                                             int32_t ndir, double* out_loss_sum, double* out_grad_sum,
                                             double* out_weight_sum, uint8_t* out_ok);
/* Per row, for few trees: out_deriv [ntrees][ndir][rows] = ∂ŷ/∂x_dir[k] and out_mixed
 * [const_off[ntrees]][ndir][rows] = ∂²ŷ/∂x_dir[k]∂c_j, of the dataset's dtype (the
 * companion of srhip_eval_grad_tree_array; "grad_kernel_deriv2_out<float>"). Any
 * dataset (no column is read); dir / ndir, expression operators and the missing wide
 * variant are answered as above. out_ok is 0 only for a tree the compiler refuses
 * (its rows are NaN): a tree that fails on some row shows it in that row. */
int32_t srhip_eval_mixed_tree_array(srhip_dataset* ds, const srhip_program* prog, const int32_t* dir, int32_t ndir,
                                    void* out_deriv, void* out_mixed, uint8_t* out_ok);

/* Per-row constant gradients for few trees: out_grad is
 * [total consts][rows] (∂ŷ_i/∂c), out_value [ntrees][rows]. */
int32_t srhip_eval_grad_tree_array(srhip_dataset* ds, const srhip_program* prog,
                                   void* out_value, void* out_grad,
                                   uint8_t* out_ok);

/* ---- batched constant optimisation ----------------------------------------
 * optimize_constants (src/ConstantOptimization.jl:22-65) for every tree of a
 * batch at once — the per-member loop of optimize_and_simplify_population
 * (src/SingleIteration.jl:63-82) in one call: every start (x0 and
 * `nrestarts` perturbed copies x0 .* (1 .+ randn/2), :46-54) of every tree
 * is a candidate, all advance in lockstep, and each phase of an iteration is
 * ONE evaluation of all candidates. BFGS (Newton for one constant, :32-33)
 * with LineSearches.BackTracking, or Nelder-Mead for trees of two or more
 * constants (:35-36); `iterations` = optimizer_iterations (Options.jl,
 * default 8). The best start of a tree is kept if it converged, else the
 * tree keeps x0 (:56-63). Gradients are analytic (srhip_eval_loss_grad), not
 * Optim's finite differences. */
#define SRHIP_OPT_BFGS 0
#define SRHIP_OPT_NELDERMEAD 1
typedef struct srhip_constopt_options {
  int32_t algorithm;          /* SRHIP_OPT_*                                              */
  int32_t iterations;         /* optimizer_iterations                                     */
  int32_t nrestarts;          /* optimizer_nrestarts                                      */
  int32_t loss_kind;          /* SRHIP_LOSS_* (srhip_optimize_constants_batch)            */
  const double* loss_params;  /* the loss parameter, or NULL                              */
  /* [nrestarts * const_off[ntrees]]: the standard normal draws of the
   * perturbed starts (Julia: randn(T, size(x0)) per restart), tree by tree,
   * restart by restart; NULL: drawn from an internal generator seeded with
   * `seed` */
  const double* start_noise;
  uint64_t seed;
} srhip_constopt_options;

/* On the engine: loss and ∂L/∂c of all candidates per launch on `ds` (the
 * programs in `ctx`, a context of the dataset's device; NULL = the dataset's
 * own context). Outputs (caller-owned): out_consts [const_off[ntrees]] of
 * the dtype — the constants to set_constants! (x0 where the run did not
 * converge); out_loss [ntrees] the loss at those constants in T (+Inf on
 * failure); out_converged [ntrees]; out_num_evals [ntrees] loss evaluations
 * (a member's num_evals increment). */
int32_t srhip_optimize_constants_batch(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                       const srhip_constopt_options* opts, void* out_consts, double* out_loss,
                                       uint8_t* out_converged, double* out_num_evals);
/* srhip_optimize_constants_batch with input tree t optimised on its own sample, the same rows for
 * all of its starts, iterations and the final evaluation. Outputs as srhip_optimize_constants_batch;
 * out_loss is the loss on the sample. row_idx is [ntrees][batch_size] as for
 * srhip_eval_loss_grad_rowsets, with the same rules, and batch_size < 1 is
 * SRHIP_ERR_INVALID. Every candidate is scored on the sample of its input tree:
 * loss-only phases as srhip_eval_loss_rowsets, gradient phases as
 * srhip_eval_loss_grad_rowsets; the samples of an evaluation set's candidates are
 * gathered once when the set is made. out_num_evals counts evaluations as
 * srhip_optimize_constants_batch does: a caller that follows the reference's
 * convention (src/Mutate.jl:43) scales it by batch_size / n.
 * Not in this version: group datasets (srhip_group_optimize_constants); a
 * target per tree through this call (a multi-target dataset is SRHIP_ERR_INVALID
 * here: take a view, or use srhip_optimize_constants_targets); one gather shared
 * among all sets through a segment indirection; row sets in
 * srhip_optimize_constants_cb, whose evaluator owns the rows. */
int32_t srhip_optimize_constants_rowsets(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                         const srhip_constopt_options* opts, const int64_t* row_idx,
                                         int64_t batch_size, void* out_consts, double* out_loss,
                                         uint8_t* out_converged, double* out_num_evals);
/* srhip_optimize_constants_batch (row_idx NULL) or srhip_optimize_constants_rowsets
 * (row_idx [ntrees][batch_size]) on a multi-target dataset, input tree t optimised
 * against column target[t]: the populations of all outputs in one lockstep run.
 * Every candidate of an evaluation set — straggler sets of a line search, the
 * Nelder-Mead simplex programs and the final evaluation included — is scored
 * against the column of its input tree: loss-only phases as srhip_eval_loss_targets /
 * srhip_eval_loss_rowsets_targets, gradient phases as srhip_eval_loss_grad_targets /
 * srhip_eval_loss_grad_rowsets_targets, and a candidate's loss and gradient are
 * divided by the Σ w of its own column (of its sample in that column with row
 * sets). The sets' programs are interpreted (no tree code). Outputs as
 * srhip_optimize_constants_batch; srhip_constopt_profile counts these calls as it
 * counts the others.
 * Rules, answered before any launch and before anything is written: a null dataset
 * or options, a null target with ntrees > 0, a target outside 0..ntargets-1, a
 * negative batch_size, and with row_idx a batch_size < 1 or an index outside
 * [0, rows) are SRHIP_ERR_INVALID; an expression-loss handle is
 * SRHIP_ERR_UNSUPPORTED (take views). A single-target dataset is accepted; its
 * targets are all 0.
 * Not in this version: expression losses; multi-target group datasets; targets in
 * srhip_optimize_constants_cb, whose evaluator owns the data; staging only the
 * columns that a launch's work items use. */
int32_t srhip_optimize_constants_targets(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                         const srhip_constopt_options* opts, const int32_t* target,
                                         const int64_t* row_idx /* NULL: all rows */, int64_t batch_size,
                                         void* out_consts, double* out_loss, uint8_t* out_converged,
                                         double* out_num_evals);
/* srhip_optimize_constants_batch under a derivative objective: a candidate's loss is
 *   f = Σ_c coef[c] · out_loss_sum[t][c] / out_weight_sum[c],  c = 0 .. ndir
 * added in channel order in float64 (+Inf when the tree failed or f is not finite),
 * and its gradient the same combination of out_grad_sum (NaN for a failed candidate).
 * ds, dir, ndir as srhip_eval_loss_deriv; the loss is opts->loss_kind / loss_params.
 * Loss-only phases run srhip_eval_loss_deriv, gradient phases
 * srhip_eval_loss_grad_deriv; BFGS, Newton for one constant and Nelder-Mead as in
 * srhip_optimize_constants_batch. The sets' programs are interpreted. Outputs as
 * srhip_optimize_constants_batch, except that out_loss is the float64 objective, not
 * rounded to the dtype. srhip_constopt_profile counts these calls as the others.
 * Refused before any launch with the outputs untouched: what srhip_eval_loss_grad_deriv
 * refuses, a null coef and a coefficient that is not finite (SRHIP_ERR_INVALID).
 * Not in this version: the wide variant; row sets; group datasets; margin and
 * expression losses; expression operators; tree code. */
int32_t srhip_optimize_constants_deriv(srhip_ctx* ctx, srhip_dataset* ds, const srhip_trees* trees,
                                       const srhip_constopt_options* opts, const int32_t* dir, int32_t ndir,
                                       const double* coef /* [1 + ndir] */, void* out_consts, double* out_loss,
                                       uint8_t* out_converged, double* out_num_evals);
/* Where the last srhip_optimize_constants_batch call of this thread spent
 * its time: out[0..8] = total, program builds, set_constants, loss calls,
 * gradient calls, the kernels inside those calls (HIP events) — seconds —
 * then the number of builds, loss calls, gradient calls and full program
 * rebuilds inside set_constants, then the builds' tree-code generation and
 * code-object load times (s), then (srhip_optimize_constants_rowsets) the
 * sets' sample gathers (s) and the number of evaluations run on row segments
 * (the first n of these 14 written). The rest of the total is the host
 * optimiser's own algebra. */
int32_t srhip_constopt_profile(double* out, int32_t n);
/* The same optimiser over any evaluator (row-sharded datasets whose partials
 * the caller all-reduces, custom losses on the CPU, tests): fn scores
 * ntasks candidates — tree_idx[k] is the input tree of candidate k, consts
 * their constants concatenated in that order (values of the dtype) —
 * writing out_f[ntasks] (the loss, +Inf on failure) and, when grad != 0,
 * out_g[constants] (∂L/∂c, NaN for failed candidates). A nonzero return
 * aborts the optimisation with SRHIP_ERR_INVALID. No device is used. */
typedef int32_t (*srhip_constopt_eval_fn)(void* user, int64_t ntasks, const int32_t* tree_idx, const double* consts,
                                          int32_t grad, double* out_f, double* out_g);
int32_t srhip_optimize_constants_cb(const srhip_trees* trees, int32_t dtype, const srhip_constopt_options* opts,
                                    srhip_constopt_eval_fn fn, void* user, void* out_consts, double* out_loss,
                                    uint8_t* out_converged, double* out_num_evals);

/* ---- device groups: one process, row shards over several GPUs ---------------
 * The reference spreads a search over its workers from one Julia process
 * (src/SymbolicRegression.jl:539-630 the per-island dispatch, :717-778 the main
 * loop that collects and migrates; src/SearchUtils.jl:33-45 one task per
 * island) and optimises constants against the whole dataset
 * (src/ConstantOptimization.jl:12-65). A group owns `ndev` members; member k
 * is a context of its own on devices[k] (what srhip_open makes) with one
 * persistent driver thread that does the member's hipSetDevice, host planning
 * and enqueues. The same device may be listed more than once: each entry is a
 * full member, which is also how a one-GPU machine runs every path. A group
 * dataset holds row shard k = srhip_group_shard_range(n, ndev, k) on member k;
 * a group program is one identical program per member. A group call
 *  - hands the call to every member; each evaluates its shard on its own stream
 *    and leaves its packed partials (the srhip_eval_loss_packed layout; for
 *    gradients [Σw·ℓ, failed] per tree, Σw·∂ℓ/∂c per constant, Σw) in slot k of
 *    a pinned host buffer that every device maps; an empty shard launches nothing;
 *  - member 0's stream waits for the other members' events and one combine
 *    kernel adds the slots elementwise in fp64 IN MEMBER ORDER k = 0 … ndev-1 —
 *    the result is the left-to-right sum of the shards' single-context results,
 *    bit for bit, whatever the timing — and finishes them: a tree that failed
 *    on ANY shard has a NaN sum, NaN for each of its constants and ok = 0;
 *  - returns after every member has finished its part, with one host wait on
 *    member 0's stream; reports the first error in member order (the message
 *    names the member) and then writes nothing into the caller's arrays.
 * No peer access is used. Group calls on one group are serialised (one mutex);
 * a context lent by srhip_group_ctx may be used with the single-device entry
 * points from any thread at any time: its own mutex serialises those calls with
 * the member's part of a group call. Destroy the group's datasets and programs
 * before srhip_group_close, and call neither while a call on them is running.
 * Not in this version: row_idx, per-tree row sets and per-row outputs over a
 * group (use the member contexts), tree shards (islands use srhip_group_ctx). */
typedef struct srhip_group srhip_group;
typedef struct srhip_group_dataset srhip_group_dataset;
typedef struct srhip_group_program srhip_group_program;

/* 1 <= ndev <= 16, devices non-NULL and non-negative (else SRHIP_ERR_INVALID);
 * an index beyond srhip_device_count is SRHIP_ERR_DEVICE, answered before any
 * context is made (so also on a machine without a device). */
int32_t srhip_group_open(const int32_t* devices, int32_t ndev, srhip_group** out_group);
int32_t srhip_group_close(srhip_group* group);
/* devices_out: [ndev] or NULL */
int32_t srhip_group_info(const srhip_group* group, int32_t* out_ndev, int32_t* devices_out);
/* Member k's context, lent: an island assigned to device k scores through the
 * single-device entry points (srhip_eval_loss_batch_ctx and the rest,
 * SearchUtils.jl:33-45). It stays the group's: do not srhip_close it. */
int32_t srhip_group_ctx(srhip_group* group, int32_t k, srhip_ctx** out_ctx);
/* Rows [begin, end) of member k of ndev over n rows: contiguous, sizes differ by
 * at most one, the first n % ndev shards the longer ones; a shard may be empty.
 * Host arithmetic only. n < 0, ndev outside 1..16 or k outside 0..ndev-1:
 * SRHIP_ERR_INVALID. */
int32_t srhip_group_shard_range(int64_t n, int32_t ndev, int32_t k, int64_t* begin, int64_t* end);

/* Dataset(X, y; weights) (src/Dataset.jl:43-64) with the rows sharded: every
 * member uploads its shard (srhip_dataset_create's arguments and checks), all
 * members at once. */
int32_t srhip_group_dataset_create(srhip_group* group, int32_t dtype, int32_t x_layout, const void* X,
                                   const void* y, const void* w, int64_t n, int32_t nfeat,
                                   srhip_group_dataset** out_gds);
int32_t srhip_group_dataset_destroy(srhip_group_dataset* gds);
/* all rows, nfeat, Σw and Σ y·w added over the members in member order, and
 * whether every shard's X is finite */
int32_t srhip_group_dataset_info(const srhip_group_dataset* gds, int64_t* out_rows, int32_t* out_nfeat,
                                 double* out_sum_w, double* out_sum_yw, int32_t* out_x_finite);

/* srhip_program_create_ex on every member with the same trees and flags, built
 * at once; the builds share the host threads one build would use (8 / ndev
 * each, so together they stay within 16). */
int32_t srhip_group_program_create(srhip_group* group, int32_t dtype, const srhip_trees* trees, uint32_t flags,
                                   srhip_group_program** out_gp);
int32_t srhip_group_program_destroy(srhip_group_program* gp);
/* srhip_program_set_constants on every member (ConstantOptimization.jl:12-19) */
int32_t srhip_group_program_set_constants(srhip_group_program* gp, const void* consts);

/* srhip_eval_loss over all rows of all shards (src/LossFunctions.jl:34-67):
 * the same outputs with the same meaning, every loss kind (margin losses and
 * expression-loss handles included). A program of another group than the
 * dataset's is SRHIP_ERR_INVALID. */
int32_t srhip_group_eval_loss(srhip_group_dataset* gds, srhip_group_program* gp, int32_t loss_kind,
                              const double* loss_params, double* out_loss_sum, double* out_weight_sum,
                              uint8_t* out_ok);
/* srhip_eval_loss_grad over all rows of all shards
 * (src/ConstantOptimization.jl:12-19, :43 with the rows split over GPUs). */
int32_t srhip_group_eval_loss_grad(srhip_group_dataset* gds, srhip_group_program* gp, int32_t loss_kind,
                                   const double* loss_params, double* out_loss_sum, double* out_dloss,
                                   double* out_weight_sum, uint8_t* out_ok);
/* srhip_optimize_constants_batch with the rows sharded
 * (src/ConstantOptimization.jl:22-65): the same optimiser, its evaluation sets
 * group programs (SRHIP_PROGRAM_VARYING_CONSTANTS) scored by the two calls
 * above. Outputs as srhip_optimize_constants_batch. */
int32_t srhip_group_optimize_constants(srhip_group_dataset* gds, const srhip_trees* trees,
                                       const srhip_constopt_options* opts, void* out_consts, double* out_loss,
                                       uint8_t* out_converged, double* out_num_evals);

/* ---- tree compiler ---------------------------------------------------------
 * Large programs are compiled to machine code, one block per tree
 * (symbolicregression.jl_amd/csrc/jit.cpp for Float32, jit64.cpp for
 * Float64; SRHIP_JIT=0 turns it off, =1 on for every size; SRHIP_WIDE and
 * wide datasets, which run without tree code: the conventions above). Tree code
 * computes exactly what the interpreter computes: eval_loss with L2 and with
 * every elementwise loss (Float32 Periodic: a tile whose |r·2π/c| leaves
 * its routine's Cody-Waite range hands the tree back to the interpreter),
 * and the per-row outputs of eval_tree_array. This reports:
 * trees compiled, of which with a guarded Float32-transcendental path, code
 * bytes, host code generation and code-object load times (ms). All zero for
 * an interpreted program. */
int32_t srhip_program_jit_info(const srhip_program* prog, int32_t* out_ntrees, int32_t* out_nfast,
                               int64_t* out_code_bytes, double* out_ms_codegen, double* out_ms_load);
/* How srhip_program_set_constants applied new constants so far: in place
 * (the device programs' immediates overwritten, same buffers; tree code built
 * with its constants in memory reads them from there) or by a full rebuild
 * (folding or a static verdict changed, or the first new constant set of a
 * tree-code program whose constants were compiled into its code: rebuilt once
 * as memory-constant tree code). */
int32_t srhip_program_update_stats(const srhip_program* prog, int64_t* out_inplace, int64_t* out_rebuilt);
/* Gradient tree code of this program (reverse-mode ∂L/∂c for
 * srhip_eval_loss_grad, built on the first gradient call; Float32: L2 and the
 * losses with a dℓ/dr routine — all but Periodic; Float64 (jit64.cpp): all
 * but LP, the non-integer LPDistLoss; LPINT has its routines in both; the
 * margin losses have none in either, their gradients run in the forward-mode
 * interpreter):
 * trees compiled, trees left to the forward-mode interpreter, code bytes,
 * codegen and load times (ms). All zero before the first gradient call. */
int32_t srhip_program_grad_jit_info(const srhip_program* prog, int32_t* out_ntrees, int32_t* out_nrejected,
                                    int64_t* out_code_bytes, double* out_ms_codegen, double* out_ms_load);
/* Which kernel passes this program's trees go to (read-only, for tests that
 * pin a batch to one interpreter variant; NULL outputs are skipped).
 * out_eval[4]: trees in the shallow list (at most 2 stack slots and 63
 * instructions; its leading trees are the tree code's), trees in the deep list,
 * trees of the shallow list compiled as tree code, operator set of the shallow
 * pass (0: the basic operators only, 1: all).
 * out_grad_items[4]: gradient work items (one per tree and group of up to 4
 * constants) of the passes with 1, 2 and 4 tangents and of the deep pass (more
 * than 4 stack slots); out_grad_rest[4]: the same counts over the trees left to
 * the interpreter when gradient tree code exists; out_grad_opset: operator set
 * of the shallow gradient passes. The gradient fields are all zero before the
 * first gradient call. */
int32_t srhip_program_pass_info(const srhip_program* prog, int32_t* out_eval, int32_t* out_grad_items,
                                int32_t* out_grad_rest, int32_t* out_grad_opset);
/* Trees of the last eval on this context whose tree code handed a tile back
 * (a sin/cos argument beyond the fast reduction) and were re-evaluated, and
 * tiles that tree code redid with the Float64-evaluated routines (a FAST-path
 * guard fired or the tile failed; out_redone may be NULL). */
int32_t srhip_last_bailed(const srhip_ctx* ctx, int32_t* out_ntrees, int64_t* out_redone);
/* Trees the last eval or gradient on this context ran as tree code (0: all
 * interpreted; srhip_eval_loss_grad: L2 and, compiled at their first use,
 * the other losses with a dℓ/dr routine, Float32 and Float64). */
int32_t srhip_last_tree_code(const srhip_ctx* ctx, int32_t* out_ntrees);
/* Shared-subtree columns. Float32 loss tree code reads the constant-free
 * subtrees that several trees of its batch contain from columns of device
 * memory. A context numbers them (canonical subtree text -> slot, at most
 * SRHIP_COLUMN_SLOTS = 64 slots, least recently used replaced) and a dataset
 * keeps the columns derived over its own rows, so a call — of the same
 * program or of another program of the dataset's context — derives only the
 * columns the dataset does not hold under the program's slots. Calls on
 * gathered rows, programs of another context, a pool beyond
 * SRHIP_COLUMN_CACHE_MB (1024) and SRHIP_COLUMN_CACHE=0 derive every column
 * at every call. Results do not depend on any of this.
 * Counters of a context since srhip_open (NULL outputs are skipped): columns
 * derived, columns that calls found in a dataset's pool, derive programs
 * built, and the registry's slot count. */
int32_t srhip_column_cache_info(const srhip_ctx* ctx, int64_t* out_derived, int64_t* out_reused,
                                int64_t* out_programs, int32_t* out_nslot);
/* The shared-subtree columns of the program's L2 loss tree code, one line
 * "<slot> <canonical text>\n" each (no device needed beyond the program's
 * own). inout_n: capacity on entry, size (without the final NUL) on return;
 * SRHIP_ERR_INVALID if too small. */
int32_t srhip_program_shared_columns(const srhip_program* prog, char* out_text, int64_t* inout_n);
/* Testing hook (no device needed): compile Float32 trees with the tree
 * compiler (fast: bit 0 the guarded FAST path, bit 1 memory-constant code,
 * bit 2 the per-row output code of srhip_eval_tree_array; bit 3: the trees
 * are Float64 (consts double) and go through the Float64 tree compiler; bit
 * 4: no assembly text — the multi-threaded code generation of the product
 * path, whose bytes must equal the text path's; bit 5: wide loss code, whose
 * features come from X in device memory (SRHIP_PROGRAM_WIDE_TREE_CODE;
 * ignored with bits 1, 2 and 3)).
 * Returns the code bytes, their assembly text ('\n'-separated lines)
 * and, per compiled tree, (tree id, byte offset). Each inout_n* holds the
 * capacity on entry and the size on return; SRHIP_ERR_INVALID if too small. */
int32_t srhip_jit_compile(const srhip_trees* trees, int32_t fast, uint8_t* out_bytes, int64_t* inout_nbytes,
                          char* out_text, int64_t* inout_ntext, int32_t* out_offsets,
                          int64_t* inout_noffsets);
/* Testing hook, same contract: the gradient tree code (reverse-mode ∂L/∂c,
 * the fast path of srhip_eval_loss_grad) of Float32 trees. */
int32_t srhip_jit_compile_grad(const srhip_trees* trees, uint8_t* out_bytes, int64_t* inout_nbytes,
                               char* out_text, int64_t* inout_ntext, int32_t* out_offsets,
                               int64_t* inout_noffsets);
/* Testing hook, same contract: the loss tree code (grad = 0; fast: its
 * guarded FAST path) or the gradient tree code (grad = 1) of Float32 trees
 * for the elementwise loss `loss` (SRHIP_LOSS_*) with its parameter; fast
 * bit 3: Float64 trees through the Float64 tree compiler with that loss's
 * routine in the tile tail, or with grad = 1 their gradient tree code; fast
 * bit 5 (grad = 0, Float32): wide loss code. SRHIP_ERR_UNSUPPORTED when Float32 tree code has no routine for that
 * loss (a Float64 tree without one is not compiled). The margin losses have
 * Float32 loss tree code only: grad = 1 or fast bit 3 with one of them is
 * SRHIP_ERR_UNSUPPORTED, and those calls run in the interpreter. */
int32_t srhip_jit_compile_loss(const srhip_trees* trees, int32_t grad, int32_t fast, int32_t loss, double loss_param,
                               uint8_t* out_bytes, int64_t* inout_nbytes, char* out_text, int64_t* inout_ntext,
                               int32_t* out_offsets, int64_t* inout_noffsets);
/* Testing hook (no device needed): the host side of
 * srhip_program_set_constants. Compiles the trees (dtype F32/F64), writes
 * new_consts through the programs' constant map (loss programs, grad = 0, or
 * gradient programs, grad = 1) and compares every tree with a fresh compile
 * of the new constants: out_mismatch = trees whose instruction stream or
 * static verdict differs (0 is correct), out_recompiled = trees the update
 * compiled again, out_relayout = 1 when it needed a rebuild instead.
 * grad | 2: the images of a program whose constants change (VARYING_CONSTANTS
 * or after its first set: a tree that fails statically keeps its code). */
int32_t srhip_debug_constant_map(const srhip_trees* trees, int32_t dtype, int32_t grad, const void* new_consts,
                                 int64_t* out_mismatch, int64_t* out_recompiled, int32_t* out_relayout);

/* ---- instrumentation ----------------------------------------------------
 * Device time (ms, HIP events on the context's stream) of the evaluation
 * kernel(s) of the last eval call on this context, and the number of kernel
 * launches it made. */
int32_t srhip_last_kernel_time(const srhip_ctx* ctx, double* out_ms,
                               int32_t* out_launches);
/* Synchronise the context's stream. */
int32_t srhip_sync(srhip_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* SRHIP_H */
