# SRHip.jl — the Julia side of the drop-in boundary (ccall into libsrhip.so).
#
# This is the binding a SymbolicRegression.jl maintainer would add (INTEGRATION.md
# shows where it plugs in). UNTESTED AS JULIA: the build image has no Julia, so
# this file has never been executed. What is tested (tests/test_julia_binding.py,
# CPU): every `ccall((:srhip_*, libsrhip), R, (A...), ...)` below names a symbol
# that include/srhip.h declares and libsrhip.so exports, with the declared number
# of arguments and compatible argument / return types; and every loss type maps
# to a SRHIP_LOSS_* code. The C ABI itself is exercised from Python through the
# same entry points (tests/test_abi.py, tests/test_gpu_parity.py, ...).
module SRHip

using DynamicExpressions: Node, count_nodes, set_constants
import DynamicExpressions  # DynamicExpressions.eval_tree_array: the CPU path of ExprLoss
import LossFunctions  # LossFunctions.value: the CPU definition of DerivativeObjective
using LossFunctions: L2DistLoss, L1DistLoss, LPDistLoss, HuberLoss, LogCoshLoss, L1EpsilonInsLoss,
    L2EpsilonInsLoss, QuantileLoss, PeriodicLoss, LogitDistLoss,
    ZeroOneLoss, PerceptronLoss, LogitMarginLoss, L1HingeLoss, L2HingeLoss, SmoothedL1HingeLoss,
    ModifiedHuberLoss, L2MarginLoss, ExpLoss, SigmoidLoss, DWDMarginLoss
import ..CoreModule: Options, Dataset

const libsrhip = get(ENV, "SRHIP_LIB", joinpath(@__DIR__, "..", "lib", "libsrhip.so"))

# include/srhip.h
const SRHIP_OK = Int32(0)
const SRHIP_ERR_UNSUPPORTED = Int32(-2)
const NODE_CONST, NODE_FEATURE, NODE_UNARY, NODE_BINARY = UInt8(0), UInt8(1), UInt8(2), UInt8(3)
const X_JULIA = Int32(0)
const LOSS_L2, LOSS_L1, LOSS_LP, LOSS_HUBER, LOSS_LOGCOSH = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)
const LOSS_L1EPSINS, LOSS_L2EPSINS, LOSS_QUANTILE, LOSS_PERIODIC, LOSS_LOGITDIST, LOSS_LPINT =
    Int32(5), Int32(6), Int32(7), Int32(8), Int32(9), Int32(10)
# margin losses (a = y·ŷ)
const LOSS_ZEROONE, LOSS_PERCEPTRON, LOSS_LOGITMARGIN, LOSS_L1HINGE, LOSS_L2HINGE, LOSS_SMOOTHEDL1HINGE =
    Int32(11), Int32(12), Int32(13), Int32(14), Int32(15), Int32(16)
const LOSS_MODHUBER, LOSS_L2MARGIN, LOSS_EXP, LOSS_SIGMOID, LOSS_DWDMARGIN =
    Int32(17), Int32(18), Int32(19), Int32(20), Int32(21)

struct SrhipTrees              # include/srhip.h: srhip_trees
    ntrees::Int32
    node_off::Ptr{Int32}
    kind::Ptr{UInt8}
    arg::Ptr{UInt16}
    const_off::Ptr{Int32}
    consts::Ptr{Cvoid}
end

"""Raised for anything outside the engine's coverage: the caller falls back to
the reference CPU path (srhip.h: SRHIP_ERR_UNSUPPORTED)."""
struct Unsupported <: Exception
    msg::String
end

last_error() = unsafe_string(ccall((:srhip_last_error, libsrhip), Cstring, ()))
const SRHIP_ERR_INVALID = Int32(-1)
function check(rc::Int32)
    rc == SRHIP_OK && return nothing
    rc == SRHIP_ERR_UNSUPPORTED && throw(Unsupported(last_error()))
    # malformed input, e.g. a program and a dataset on different devices
    rc == SRHIP_ERR_INVALID && throw(ArgumentError("srhip: $(last_error())"))
    error("srhip: $(last_error())")
end

dtype_code(::Type{Float32}) = Int32(0)
dtype_code(::Type{Float64}) = Int32(1)
dtype_code(::Type) = throw(Unsupported("only Float32/Float64 run on the GPU"))

# ---- elementwise losses -> SRHIP_LOSS_* (LossFunctions.jl distance and margin losses,
# src/Options.jl:429-431 default L2DistLoss; docs/src/losses.md) ----------------
loss_code(::L2DistLoss) = (LOSS_L2, 0.0)
loss_code(::L1DistLoss) = (LOSS_L1, 0.0)
# LPDistLoss{P} with an Int P keeps Julia's T^Integer rules (srhip.h SRHIP_LOSS_LPINT)
loss_code(::LPDistLoss{P}) where {P} = (P isa Integer ? LOSS_LPINT : LOSS_LP, Float64(P))
loss_code(l::HuberLoss) = (LOSS_HUBER, Float64(l.d))
loss_code(::LogCoshLoss) = (LOSS_LOGCOSH, 0.0)
loss_code(l::L1EpsilonInsLoss) = (LOSS_L1EPSINS, Float64(l.ε))
loss_code(l::L2EpsilonInsLoss) = (LOSS_L2EPSINS, Float64(l.ε))
loss_code(l::QuantileLoss) = (LOSS_QUANTILE, Float64(l.τ))
# PeriodicLoss stores k = 2π/circumference; the engine takes the circumference
loss_code(l::PeriodicLoss) = (LOSS_PERIODIC, 2π / Float64(l.k))
loss_code(::LogitDistLoss) = (LOSS_LOGITDIST, 0.0)
# margin losses (docs/src/losses.md:226-520; HingeLoss is L1HingeLoss). The engine checks
# the parameters: γ > 0, q > 0, and a q that is not integral is Unsupported (CPU path).
loss_code(::ZeroOneLoss) = (LOSS_ZEROONE, 0.0)
loss_code(::PerceptronLoss) = (LOSS_PERCEPTRON, 0.0)
loss_code(::LogitMarginLoss) = (LOSS_LOGITMARGIN, 0.0)
loss_code(::L1HingeLoss) = (LOSS_L1HINGE, 0.0)
loss_code(::L2HingeLoss) = (LOSS_L2HINGE, 0.0)
loss_code(l::SmoothedL1HingeLoss) = (LOSS_SMOOTHEDL1HINGE, Float64(l.gamma))
loss_code(::ModifiedHuberLoss) = (LOSS_MODHUBER, 0.0)
loss_code(::L2MarginLoss) = (LOSS_L2MARGIN, 0.0)
loss_code(::ExpLoss) = (LOSS_EXP, 0.0)
loss_code(::SigmoidLoss) = (LOSS_SIGMOID, 0.0)
loss_code(l::DWDMarginLoss) = (LOSS_DWDMARGIN, Float64(l.q))
loss_code(l) = throw(Unsupported("elementwise loss $(typeof(l)) is not in the engine's table"))

# ---- contexts: one per (thread, device); calls through a context are serialised.
# An evaluation runs on its PROGRAM's context (srhip.h): programs are created
# in the calling thread's context, datasets are uploaded once per device and
# shared by every thread's context, so threads (one island each,
# src/SearchUtils.jl:33-45) score concurrently. A task that migrates between
# threads keeps using the context its program was created in, which is safe
# (the context's mutex serialises it with that thread's calls).
const CTX = Dict{Tuple{Int,Int},Ptr{Cvoid}}()
const CTX_LOCK = ReentrantLock()
function context(device::Int=0)
    key = (Threads.threadid(), device)
    lock(CTX_LOCK) do
        get!(CTX, key) do
            h = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:srhip_open, libsrhip), Int32, (Int32, Ptr{Ptr{Cvoid}}), device, h))
            h[]
        end
    end
end

function device_available()
    n = Ref{Int32}(0)
    try
        ccall((:srhip_device_count, libsrhip), Int32, (Ptr{Int32},), n) == SRHIP_OK && n[] > 0
    catch
        false  # library missing or not loadable
    end
end

# ---- operator ids (srhip_op_lookup applies binopmap/unaopmap names) ------------
# Expression operators (srhip.h "expression operators"): Julia functions that
# register_operator! gave a body tree; flatten maps them to their handles.
const SRHIP_EXPR_OP_BEGIN = Int32(1024)  # operator ids from here on are handles of expression operators
mutable struct ExprOpHandle
    id::Int32
    arity::Int
end
const EXPR_OPS = IdDict{Any,ExprOpHandle}()

function op_id(op, arity)
    h = lock(CTX_LOCK) do
        get(EXPR_OPS, op, nothing)
    end
    if h !== nothing
        h.arity == arity || throw(Unsupported("operator $(op) has arity $(h.arity)"))
        return UInt16(h.id)
    end
    a = Ref{Int32}(0); i = Ref{Int32}(0)
    check(ccall((:srhip_op_lookup, libsrhip), Int32, (Cstring, Ptr{Int32}, Ptr{Int32}),
                string(nameof(op)), a, i))
    a[] == arity || throw(Unsupported("operator $(op) has arity $(a[])"))
    return UInt16(i[])
end
const OPS_CACHE = IdDict{Any,Any}()
operator_ids(options::Options) = lock(CTX_LOCK) do
    get!(OPS_CACHE, options) do
        ([op_id(op, 2) for op in options.operators.binops], [op_id(op, 1) for op in options.operators.unaops])
    end
end

"""
    register_operator!(f, tree::Node{T}, operators; arity)

Give the custom operator `f` (a Julia function in `binary_operators` /
`unary_operators`) its definition as a tree over x1 = the first argument and
x2 = the second, built with `operators` (an `OperatorEnum` of engine
primitives). The engine registers the body once; `flatten` then maps `f` to the
handle (>= SRHIP_EXPR_OP_BEGIN) instead of asking `srhip_op_lookup`, so a
search whose operator list holds `f` runs on the engine. The handle is destroyed
by the finaliser of the returned object, which the registry keeps alive.
Nothing inside the body is checked for non-finite values, as for an opaque
Julia function; `f` itself stays the CPU path's definition.
"""
function register_operator!(f, tree::Node{T}, operators; arity::Int) where {T}
    bin = [op_id(op, 2) for op in operators.binops]
    una = [op_id(op, 1) for op in operators.unaops]
    kind = UInt8[]; arg = UInt16[]; consts = Float64[]
    function visit(t::Node{T})
        if t.degree == 0
            if t.constant
                push!(kind, NODE_CONST); push!(arg, 0); push!(consts, Float64(t.val::T))
            else
                push!(kind, NODE_FEATURE); push!(arg, UInt16(t.feature - 1))
            end
        elseif t.degree == 1
            visit(t.l); push!(kind, NODE_UNARY); push!(arg, una[t.op])
        else
            visit(t.l); visit(t.r); push!(kind, NODE_BINARY); push!(arg, bin[t.op])
        end
    end
    visit(tree)
    h = Ref{Int32}(0)
    check(ccall((:srhip_op_expr_create, libsrhip), Int32,
                (Int32, Ptr{UInt8}, Ptr{UInt16}, Int32, Ptr{Float64}, Int32, Ptr{Int32}),
                Int32(arity), kind, arg, Int32(length(kind)), consts, Int32(length(consts)), h))
    x = ExprOpHandle(h[], arity)
    finalizer(x) do y
        ccall((:srhip_op_expr_destroy, libsrhip), Int32, (Int32,), y.id)
    end
    lock(CTX_LOCK) do
        EXPR_OPS[f] = x
        empty!(OPS_CACHE)  # operator ids resolved before the registration are stale
    end
    return x
end

"""
    enabled(options) -> Bool

Whether `options` can run on the engine: a device is visible, `loss_function`
is not set (arbitrary Julia stays on the CPU, src/LossFunctions.jl:60-67) or is
a `DerivativeObjective` (scored by the fused call `eval_loss_deriv`), the
elementwise loss and every operator are in the engine's table. Set
ENV["SRHIP_DISABLE"] = "1" to force the reference path.
"""
function enabled(options::Options)
    get(ENV, "SRHIP_DISABLE", "0") == "1" && return false
    # the recorder's genealogy (src/Recorder.jl, Options.jl:597-599) is written by
    # the reference's per-candidate loops: with it on, the search stays there
    options.recorder && return false
    (options.loss_function === nothing || options.loss_function isa DerivativeObjective) || return false
    device_available() || return false
    try
        loss_code(options.elementwise_loss)
        operator_ids(options)
        return true
    catch e
        e isa Unsupported || rethrow()
        return false
    end
end

# ---- flattening: post-order node streams, constants in get_constants order ----
function flatten(trees::AbstractVector{Node{T}}, options::Options) where {T}
    bin, una = operator_ids(options)
    kind = UInt8[]; arg = UInt16[]; consts = T[]
    node_off = Int32[0]; const_off = Int32[0]
    function visit(t::Node{T})
        if t.degree == 0
            if t.constant
                push!(kind, NODE_CONST); push!(arg, 0); push!(consts, t.val::T)
            else
                push!(kind, NODE_FEATURE); push!(arg, UInt16(t.feature - 1))
            end
        elseif t.degree == 1
            visit(t.l); push!(kind, NODE_UNARY); push!(arg, una[t.op])
        else
            visit(t.l); visit(t.r); push!(kind, NODE_BINARY); push!(arg, bin[t.op])
        end
    end
    for t in trees
        visit(t)
        push!(node_off, length(kind)); push!(const_off, length(consts))
    end
    return node_off, kind, arg, const_off, consts
end

# ---- expression losses: a custom elementwise_loss written as a tree (srhip.h
# "expression losses") ----------------------------------------------------------
const SRHIP_EXPR_LOSS_BEGIN = Int32(1024)  # loss kinds from here on are handles of expression losses

"""
    ExprLoss(tree::Node{T}, operators)

A custom `elementwise_loss` as a tree over x1 = the prediction, x2 = the target
and x3 = the weight, built with `operators` (an `OperatorEnum`, e.g.
`options.operators`). It is registered with the engine once (`kind` is the
handle, >= SRHIP_EXPR_LOSS_BEGIN, destroyed by the finaliser) and is itself a
function `(x, y)` / `(x, y, w)`, so the reference's CPU path
(src/LossFunctions.jl:17-31) evaluates the same tree. The engine sums the loss
values as they are: a weighted loss multiplies by x3 itself, and a tree that
reads x3 needs a weighted dataset.
"""
mutable struct ExprLoss{T,O} <: Function
    tree::Node{T}
    operators::O
    kind::Int32
end

function ExprLoss(tree::Node{T}, operators) where {T}
    bin = [op_id(op, 2) for op in operators.binops]
    una = [op_id(op, 1) for op in operators.unaops]
    kind = UInt8[]; arg = UInt16[]; consts = Float64[]
    function visit(t::Node{T})
        if t.degree == 0
            if t.constant
                push!(kind, NODE_CONST); push!(arg, 0); push!(consts, Float64(t.val::T))
            else
                push!(kind, NODE_FEATURE); push!(arg, UInt16(t.feature - 1))
            end
        elseif t.degree == 1
            visit(t.l); push!(kind, NODE_UNARY); push!(arg, una[t.op])
        else
            visit(t.l); visit(t.r); push!(kind, NODE_BINARY); push!(arg, bin[t.op])
        end
    end
    visit(tree)
    h = Ref{Int32}(0)
    check(ccall((:srhip_loss_expr_create, libsrhip), Int32,
                (Ptr{UInt8}, Ptr{UInt16}, Int32, Ptr{Float64}, Int32, Ptr{Int32}),
                kind, arg, Int32(length(kind)), consts, Int32(length(consts)), h))
    l = ExprLoss{T,typeof(operators)}(tree, operators, h[])
    finalizer(l) do x
        ccall((:srhip_loss_expr_destroy, libsrhip), Int32, (Int32,), x.kind)
    end
    return l
end

# the CPU path: the same tree on one (prediction, target, weight) triple
function (l::ExprLoss{T})(x, y, w=zero(T)) where {T}
    out, _ = DynamicExpressions.eval_tree_array(l.tree, reshape(T[x, y, w], 3, 1), l.operators)
    return out[1]
end

loss_code(l::ExprLoss) = (l.kind, 0.0)

# A compiled, device-resident batch of trees (srhip_program_create); destroyed
# by the caller (`destroy`) or by the finaliser.
mutable struct Program
    h::Ptr{Cvoid}
    ntrees::Int
    const_off::Vector{Int32}
    device::Int   # its datasets are this device's (srhip.h: a call runs on the program's context)
end
function destroy(p::Program)
    p.h == C_NULL && return nothing
    ccall((:srhip_program_destroy, libsrhip), Int32, (Ptr{Cvoid},), p.h)
    p.h = C_NULL
    return nothing
end
# varying_constants: the caller will set_constants! (the candidates of
# optimize_constants), so Float32 tree code reads its constants from memory
# from the start (SRHIP_PROGRAM_VARYING_CONSTANTS: no recompile on a new set)
const PROGRAM_VARYING_CONSTANTS = UInt32(1)
const PROGRAM_INTERPRETED = UInt32(2)  # no loss / output tree code (per-tree row sets, per-tree targets)
# wide_tree_code (opt-in): Float32 literal-constant loss tree code may read its
# features from X in device memory (SRHIP_PROGRAM_WIDE_TREE_CODE), so trees that
# read features from index 63 on and datasets too wide for LDS keep tree code
const PROGRAM_WIDE_TREE_CODE = UInt32(4)
function Program(trees::AbstractVector{Node{T}}, options::Options, device::Int=0;
                 varying_constants::Bool=false, wide_tree_code::Bool=false) where {T}
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    flags = (varying_constants ? PROGRAM_VARYING_CONSTANTS : UInt32(0)) |
            (wide_tree_code ? PROGRAM_WIDE_TREE_CODE : UInt32(0))
    GC.@preserve node_off kind arg const_off consts begin
        tr = Ref(SrhipTrees(Int32(length(trees)), pointer(node_off), pointer(kind), pointer(arg),
                            pointer(const_off), Ptr{Cvoid}(pointer(consts))))
        check(ccall((:srhip_program_create_ex, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Ref{SrhipTrees}, UInt32, Ptr{Ptr{Cvoid}}),
                    context(device), dtype_code(T), tr, flags, h))
    end
    p = Program(h[], length(trees), const_off, device)
    finalizer(destroy, p)
    return p
end

function set_constants!(p::Program, consts::Vector{T}) where {T}
    length(consts) == p.const_off[end] || throw(ArgumentError("expected $(p.const_off[end]) constants"))
    GC.@preserve consts check(ccall((:srhip_program_set_constants, libsrhip), Int32,
                                    (Ptr{Cvoid}, Ptr{Cvoid}), p.h, consts))
    return p
end

# ---- device datasets ----------------------------------------------------------
function upload(X::AbstractMatrix{T}, y::AbstractVector{T}, w, device::Int) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    Xc = Matrix{T}(X); yc = Vector{T}(y)
    wc = w === nothing ? nothing : Vector{T}(w)
    nfeat, n = size(Xc)
    GC.@preserve Xc yc wc begin
        check(ccall((:srhip_dataset_create, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Int64, Int32, Int64, Int64,
                     Ptr{Ptr{Cvoid}}),
                    context(device), dtype_code(T), X_JULIA, Xc, yc,
                    wc === nothing ? Ptr{T}(C_NULL) : wc, n, nfeat, 0, n, h))
    end
    return h[]
end
destroy_dataset(h::Ptr{Cvoid}) = ccall((:srhip_dataset_destroy, libsrhip), Int32, (Ptr{Cvoid},), h)

# one device copy per (Dataset, device) (src/Dataset.jl:24-64), uploaded once
# and shared by the contexts of all threads. The table holds its Datasets
# weakly (Dataset is a mutable struct): when a Dataset is collected its entry
# goes, and the DeviceCopy's finaliser frees the device memory. Guarded by
# CTX_LOCK.
mutable struct DeviceCopy
    h::Ptr{Cvoid}
end
function free!(d::DeviceCopy)
    d.h == C_NULL && return nothing
    destroy_dataset(d.h)
    d.h = C_NULL
    return nothing
end
const DEVICE_DATASETS = WeakKeyDict{Dataset,Dict{Int,DeviceCopy}}()
function device_dataset(dataset::Dataset{T}, device::Int=0) where {T}
    lock(CTX_LOCK) do
        # an output of a multi-output search (MultiCopy below): its view of the shared upload
        e = covering(dataset, device)
        e !== nothing && e[1].h != C_NULL && return e[1].views[e[2]]
        copies = get!(() -> Dict{Int,DeviceCopy}(), DEVICE_DATASETS, dataset)
        d = get(copies, device, nothing)
        d !== nothing && d.h != C_NULL && return d.h
        d = DeviceCopy(upload(dataset.X, dataset.y, dataset.weighted ? dataset.weights : nothing, device))
        finalizer(free!, d)
        copies[device] = d
        return d.h
    end
end
"""Free the device copies of `dataset` now (they are also freed when the
Dataset is garbage-collected)."""
function release_dataset!(dataset::Dataset)
    lock(CTX_LOCK) do
        copies = pop!(DEVICE_DATASETS, dataset, nothing)
        copies === nothing || foreach(free!, values(copies))
    end
    return nothing
end

# ---- multi-output datasets (srhip.h "multi-output datasets") ------------------------
# EquationSearch(X, y::AbstractMatrix) builds nout Datasets over the SAME X object
# (src/SymbolicRegression.jl:304-315). A MultiCopy is one upload for all of them:
# X once, the targets and weights as columns (srhip_dataset_create_multi), and one
# view per output (srhip_dataset_view), which device_dataset(datasets[j]) then
# returns, so an nout-output search holds one X on the device. Each covered
# Dataset is held weakly (MULTI_DATASETS); the MultiCopy is freed by its finaliser
# once no Dataset refers to it, or at once by free!. Guarded by CTX_LOCK.
const SRHIP_MAX_TARGETS = Int32(16)
mutable struct MultiCopy
    h::Ptr{Cvoid}               # the multi-target dataset
    views::Vector{Ptr{Cvoid}}   # views[j]: output j as a single-target dataset
    device::Int
end
function free!(m::MultiCopy)
    m.h == C_NULL && return nothing
    foreach(destroy_dataset, m.views)   # parent and views in any order: memory goes with the last
    destroy_dataset(m.h)
    empty!(m.views)
    m.h = C_NULL
    return nothing
end
const MULTI_DATASETS = WeakKeyDict{Dataset,Dict{Int,Tuple{MultiCopy,Int}}}()
# the (MultiCopy, output index) that covers `dataset` on `device`, or nothing (under CTX_LOCK)
function covering(dataset::Dataset, device::Int)
    mv = get(MULTI_DATASETS, dataset, nothing)
    return mv === nothing ? nothing : get(mv, device, nothing)
end
"""
    MultiCopy(datasets, device=0) -> MultiCopy

One device upload for the `nout` Datasets of a multi-output search, whose `X` must be the
same object (`datasets[j].X === datasets[1].X`) and which are all weighted or all
unweighted. Returns the existing one when these Datasets are already covered.
"""
function MultiCopy(datasets::AbstractVector{<:Dataset{T}}, device::Int=0) where {T}
    K = length(datasets)
    1 <= K <= SRHIP_MAX_TARGETS || throw(ArgumentError("1 to $(SRHIP_MAX_TARGETS) outputs"))
    d1 = datasets[1]
    for d in datasets
        d.X === d1.X || throw(ArgumentError("the datasets of a MultiCopy share one X object"))
        d.weighted == d1.weighted || throw(ArgumentError("all outputs weighted, or none"))
    end
    lock(CTX_LOCK) do
        m1 = covering(d1, device)
        if m1 !== nothing && m1[1].h != C_NULL && length(m1[1].views) == K &&
           all(j -> covering(datasets[j], device) == (m1[1], j), 1:K)
            return m1[1]
        end
        nfeat, n = size(d1.X)
        Xc = Matrix{T}(d1.X)
        Yc = Matrix{T}(undef, n, K)          # column j = target j: [ntargets][n] in C
        Wc = d1.weighted ? Matrix{T}(undef, n, K) : nothing
        for j in 1:K
            Yc[:, j] .= datasets[j].y
            Wc === nothing || (Wc[:, j] .= datasets[j].weights)
        end
        h = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve Xc Yc Wc begin
            check(ccall((:srhip_dataset_create_multi, libsrhip), Int32,
                        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Int64, Int32, Int32, Int64, Int64,
                         Ptr{Ptr{Cvoid}}),
                        context(device), dtype_code(T), X_JULIA, Xc, Yc,
                        Wc === nothing ? Ptr{T}(C_NULL) : Wc, n, nfeat, K, 0, n, h))
        end
        m = MultiCopy(h[], Ptr{Cvoid}[], device)
        finalizer(free!, m)
        for j in 1:K
            v = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:srhip_dataset_view, libsrhip), Int32, (Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}),
                        m.h, j - 1, v))
            push!(m.views, v[])
        end
        for j in 1:K
            get!(() -> Dict{Int,Tuple{MultiCopy,Int}}(), MULTI_DATASETS, datasets[j])[device] = (m, j)
        end
        return m
    end
end

"""
    eval_loss_batch_targets(trees, js, datasets, options; device=0) -> Vector{T}

`eval_loss` of `trees[i]` against `datasets[js[i]]` (the outputs of one MultiCopy) for the
candidates of several outputs in ONE launch (srhip_eval_loss_batch_targets_ctx); T(Inf)
where evaluation fails. Expression losses are `Unsupported` here (the callers fall back).
"""
function eval_loss_batch_targets(trees::AbstractVector{Node{T}}, js::AbstractVector{<:Integer},
                                 datasets::AbstractVector{<:Dataset{T}}, options::Options;
                                 device::Int=0) where {T}
    nt = length(trees)
    length(js) == nt || throw(ArgumentError("one output index per tree"))
    m = MultiCopy(datasets, device)
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt)
    wsum = Vector{Float64}(undef, length(datasets))
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    target = Int32.(js .- 1)
    GC.@preserve node_off kind arg const_off consts sums ok wsum params target m datasets begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        check(ccall((:srhip_eval_loss_batch_targets_ctx, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64},
                     Ptr{Float64}, Ptr{UInt8}),
                    context(device), m.h, tr, kindcode, params, target, sums, wsum, ok))
    end
    return [ok[i] == 1 ? T(sums[i] / wsum[js[i]]) : T(Inf) for i in 1:nt]
end

"""
    eval_loss_batch_targets_rowsets(trees, js, datasets, options, idx) -> Vector{T}

The per-tree minibatch form: `trees[i]` on its own row sample `idx[:, i]` (1-based, with
repetition) against `datasets[js[i]]`, one launch (srhip_eval_loss_rowsets_targets).
"""
function eval_loss_batch_targets_rowsets(trees::AbstractVector{Node{T}}, js::AbstractVector{<:Integer},
                                         datasets::AbstractVector{<:Dataset{T}}, options::Options,
                                         idx::AbstractMatrix{<:Integer}; device::Int=0) where {T}
    nt = length(trees)
    length(js) == nt || throw(ArgumentError("one output index per tree"))
    size(idx, 2) == nt || throw(ArgumentError("one row sample (column of idx) per tree"))
    m = MultiCopy(datasets, device)
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Vector{Float64}(undef, nt)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    target = Int32.(js .- 1)
    rows = Matrix{Int64}(idx .- 1)  # column-major: tree t's sample is contiguous ([ntrees][bs] in C)
    prog = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve node_off kind arg const_off consts sums ok wsum params target rows m datasets begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        # row sets run in the interpreter: no tree code to build
        check(ccall((:srhip_program_create_ex, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Ref{SrhipTrees}, UInt32, Ptr{Ptr{Cvoid}}),
                    context(device), dtype_code(T), tr, PROGRAM_INTERPRETED, prog))
        try
            check(ccall((:srhip_eval_loss_rowsets_targets, libsrhip), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}, Int64, Ptr{Float64},
                         Ptr{Float64}, Ptr{UInt8}),
                        m.h, prog[], kindcode, params, target, rows, size(rows, 1), sums, wsum, ok))
        finally
            ccall((:srhip_program_destroy, libsrhip), Int32, (Ptr{Cvoid},), prog[])
        end
    end
    return [ok[i] == 1 ? T(sums[i] / wsum[i]) : T(Inf) for i in 1:nt]
end
# ---- eval_loss (src/LossFunctions.jl:34-67), batched ------------------------------
"""
    eval_loss_batch(trees, dataset, options; idx=nothing) -> Vector{T}

Batched `eval_loss` (src/LossFunctions.jl:60-67): one device launch for all
trees; T(Inf) where evaluation fails. `idx` (1-based, with repetition) is
score_func_batch's row sample (src/LossFunctions.jl:95-115).
"""
function eval_loss_batch(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options;
                         idx=nothing, device::Int=0) where {T}
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    nt = length(trees)
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Ref{Float64}(0)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    rows = idx === nothing ? Int64[] : Int64.(idx .- 1)
    GC.@preserve node_off kind arg const_off consts sums ok params rows begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        # the program lives in this thread's context, the dataset is shared
        check(ccall((:srhip_eval_loss_batch_ctx, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Int32, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64},
                     Ref{Float64}, Ptr{UInt8}),
                    context(device), device_dataset(dataset, device), tr, kindcode, params,
                    idx === nothing ? Ptr{Int64}(C_NULL) : pointer(rows), length(rows), sums, wsum, ok))
    end
    return [ok[i] == 1 ? T(sums[i] / wsum[]) : T(Inf) for i in 1:nt]
end

"""
    eval_loss_batch_rowsets(trees, dataset, options, idx::Matrix{Int}) -> Vector{T}

score_func_batch's loss (src/LossFunctions.jl:95-115) for every tree on its OWN
row sample: idx is (batch_size, ntrees), column t the 1-based rows (with
repetition) of trees[t] — one `StatsBase.sample(1:n, batch_size;
replace=true)` per candidate, as the reference draws per call (:98). One
launch (srhip_eval_loss_batch_rowsets_ctx); T(Inf) where evaluation fails.
"""
function eval_loss_batch_rowsets(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options,
                                 idx::AbstractMatrix{<:Integer}; device::Int=0) where {T}
    nt = length(trees)
    size(idx, 2) == nt || throw(ArgumentError("one row sample (column of idx) per tree"))
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Vector{Float64}(undef, nt)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    rows = Matrix{Int64}(idx .- 1)  # column-major: tree t's sample is contiguous ([ntrees][bs] in C)
    GC.@preserve node_off kind arg const_off consts sums ok wsum params rows begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        check(ccall((:srhip_eval_loss_batch_rowsets_ctx, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Int32, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64},
                     Ptr{Float64}, Ptr{UInt8}),
                    context(device), device_dataset(dataset, device), tr, kindcode, params, rows,
                    size(rows, 1), sums, wsum, ok))
    end
    return [ok[i] == 1 ? T(sums[i] / wsum[i]) : T(Inf) for i in 1:nt]
end

"""
    eval_loss_grad_batch(p::Program, dataset, options) -> (losses, grads, ok)

Loss and ∂loss/∂c of every constant of every tree of `p` in one launch
(`srhip_eval_loss_grad`), for batched constant optimisation
(src/ConstantOptimization.jl:12-65). grads[t] is in get_constants order.
"""
function eval_loss_grad_batch(p::Program, dataset::Dataset{T}, options::Options) where {T}
    nt = p.ntrees
    ncon = Int(p.const_off[end])
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Ref{Float64}(0)
    dloss = Vector{Float64}(undef, ncon)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    GC.@preserve sums ok dloss params begin
        check(ccall((:srhip_eval_loss_grad, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64},
                     Ptr{UInt8}),
                    device_dataset(dataset, p.device), p.h, kindcode, params, sums, dloss, wsum, ok))
    end
    losses = [ok[i] == 1 ? T(sums[i] / wsum[]) : T(Inf) for i in 1:nt]
    grads = [dloss[(p.const_off[i] + 1):p.const_off[i + 1]] ./ wsum[] for i in 1:nt]
    return losses, grads, ok .== 1
end

"""
    eval_loss_grad_rowsets(p::Program, dataset, options, idx::Matrix{Int}) -> (losses, grads, ok)

eval_loss_grad_batch with every tree on its OWN row sample (`srhip_eval_loss_grad_rowsets`): idx is
(batch_size, ntrees), column t the 1-based rows (with repetition) of tree t, as
eval_loss_batch_rowsets takes them. Loss and gradient are divided by the sample's Σw.
"""
function eval_loss_grad_rowsets(p::Program, dataset::Dataset{T}, options::Options,
                                idx::AbstractMatrix{<:Integer}) where {T}
    nt = p.ntrees
    size(idx, 2) == nt || throw(ArgumentError("one row sample (column of idx) per tree"))
    ncon = Int(p.const_off[end])
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Vector{Float64}(undef, nt)
    dloss = Vector{Float64}(undef, ncon)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    rows = Matrix{Int64}(idx .- 1)  # column-major: tree t's sample is contiguous ([ntrees][bs] in C)
    GC.@preserve sums ok dloss wsum params rows begin
        check(ccall((:srhip_eval_loss_grad_rowsets, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{UInt8}),
                    device_dataset(dataset, p.device), p.h, kindcode, params, rows, size(rows, 1), sums, dloss,
                    wsum, ok))
    end
    losses = [ok[i] == 1 ? T(sums[i] / wsum[i]) : T(Inf) for i in 1:nt]
    grads = [dloss[(p.const_off[i] + 1):p.const_off[i + 1]] ./ wsum[i] for i in 1:nt]
    return losses, grads, ok .== 1
end

# ---- batched constant optimisation (src/ConstantOptimization.jl:22-65) ----------------
struct ConstOptOptions         # include/srhip.h: srhip_constopt_options
    algorithm::Int32
    iterations::Int32
    nrestarts::Int32
    loss_kind::Int32
    loss_params::Ptr{Float64}
    start_noise::Ptr{Float64}
    seed::UInt64
end
const OPT_BFGS, OPT_NELDERMEAD = Int32(0), Int32(1)

"""
    optimize_constants_batch!(trees, dataset, options) -> (losses, converged, num_evals)

optimize_constants (src/ConstantOptimization.jl:22-65) for every tree at once
(srhip_optimize_constants_batch): all starts of all trees in lockstep on the
engine, one launch per phase. The perturbed starts draw `randn(T, nconst)`
per restart, tree by tree, where the reference does (:47). Trees whose run
converged get the best start's constants (set_constants); the others keep
x0 (:56-63). losses[i] is the loss of trees[i] at its final constants;
num_evals[i] counts its loss evaluations (+1 for the re-score of a converged
member, :58-59).

`row_idx` (batch_size, ntrees), column t the 1-based rows (with repetition) of trees[t]: every tree
is optimised on its own sample (srhip_optimize_constants_rowsets), the same rows for all of its
starts, iterations and the final evaluation; losses are then those on the samples, and num_evals
still counts evaluations (the caller scales by batch_size / n, src/Mutate.jl:43).
"""
function optimize_constants_batch!(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options;
                                   device::Int=0,
                                   row_idx::Union{Nothing,AbstractMatrix{<:Integer}}=nothing) where {T}
    algo = options.optimizer_algorithm == "BFGS" ? OPT_BFGS :
           options.optimizer_algorithm == "NelderMead" ? OPT_NELDERMEAD :
           error("Optimization function not implemented.")
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    nt = length(trees)
    nr = options.optimizer_nrestarts
    noise = Float64[]
    for i in 1:nt
        nc = Int(const_off[i + 1] - const_off[i])
        nc == 0 && continue
        for _ in 1:nr
            append!(noise, Float64.(randn(T, nc)))
        end
    end
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    out_c = similar(consts); out_l = Vector{Float64}(undef, nt)
    out_k = Vector{UInt8}(undef, nt); out_n = Vector{Float64}(undef, nt)
    if row_idx !== nothing
        size(row_idx, 2) == nt || throw(ArgumentError("one row sample (column of row_idx) per tree"))
    end
    # column-major: tree t's sample is contiguous ([ntrees][bs] in C), 0-based
    rows = row_idx === nothing ? Matrix{Int64}(undef, 0, 0) : Matrix{Int64}(row_idx .- 1)
    GC.@preserve node_off kind arg const_off consts noise params out_c out_l out_k out_n rows begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        opts = Ref(ConstOptOptions(algo, Int32(options.optimizer_options.iterations), Int32(nr), kindcode,
                                   pointer(params), pointer(noise), UInt64(0)))
        if row_idx === nothing
            check(ccall((:srhip_optimize_constants_batch, libsrhip), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Ref{ConstOptOptions}, Ptr{Cvoid}, Ptr{Float64},
                         Ptr{UInt8}, Ptr{Float64}),
                        context(device), device_dataset(dataset, device), tr, opts, out_c, out_l, out_k, out_n))
        else
            check(ccall((:srhip_optimize_constants_rowsets, libsrhip), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Ref{ConstOptOptions}, Ptr{Int64}, Int64, Ptr{Cvoid},
                         Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}),
                        context(device), device_dataset(dataset, device), tr, opts, rows, size(rows, 1), out_c,
                        out_l, out_k, out_n))
        end
    end
    converged = out_k .== 1
    for i in 1:nt
        converged[i] && set_constants(trees[i], out_c[(const_off[i] + 1):const_off[i + 1]])
    end
    return T.(out_l), converged, out_n
end

# ---- gradients and constant optimisation with an output per tree --------------------
"""
    eval_loss_grad_targets(trees, js, datasets, options; device=0, idx=nothing) -> (losses, grads, ok)

Loss and ∂loss/∂c of `trees[i]` against `datasets[js[i]]` (the outputs of one MultiCopy) for the
members of several outputs in one call (srhip_eval_loss_grad_targets), each divided by the Σw of
its own output. `idx` (batch_size, ntrees), column t the 1-based rows of trees[t]: every tree on
its own sample (srhip_eval_loss_grad_rowsets_targets), divided by the sample's Σw. Expression
losses are `Unsupported` here (the callers fall back to one call per output).
"""
function eval_loss_grad_targets(trees::AbstractVector{Node{T}}, js::AbstractVector{<:Integer},
                                datasets::AbstractVector{<:Dataset{T}}, options::Options;
                                device::Int=0,
                                idx::Union{Nothing,AbstractMatrix{<:Integer}}=nothing) where {T}
    nt = length(trees)
    length(js) == nt || throw(ArgumentError("one output index per tree"))
    idx === nothing || size(idx, 2) == nt || throw(ArgumentError("one row sample (column of idx) per tree"))
    m = MultiCopy(datasets, device)
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    ncon = Int(const_off[end])
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt)
    wsum = Vector{Float64}(undef, idx === nothing ? length(datasets) : nt)
    dloss = Vector{Float64}(undef, ncon)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    target = Int32.(js .- 1)
    rows = idx === nothing ? Matrix{Int64}(undef, 0, 0) : Matrix{Int64}(idx .- 1)
    prog = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve node_off kind arg const_off consts sums ok wsum dloss params target rows m datasets begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        # the fused calls run in the interpreter: no tree code to build
        check(ccall((:srhip_program_create_ex, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Ref{SrhipTrees}, UInt32, Ptr{Ptr{Cvoid}}),
                    context(device), dtype_code(T), tr, PROGRAM_INTERPRETED, prog))
        try
            if idx === nothing
                check(ccall((:srhip_eval_loss_grad_targets, libsrhip), Int32,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                             Ptr{Float64}, Ptr{UInt8}),
                            m.h, prog[], kindcode, params, target, sums, dloss, wsum, ok))
            else
                check(ccall((:srhip_eval_loss_grad_rowsets_targets, libsrhip), Int32,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}, Int64,
                             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                            m.h, prog[], kindcode, params, target, rows, size(rows, 1), sums, dloss, wsum, ok))
            end
        finally
            ccall((:srhip_program_destroy, libsrhip), Int32, (Ptr{Cvoid},), prog[])
        end
    end
    ws = [idx === nothing ? wsum[js[i]] : wsum[i] for i in 1:nt]
    losses = [ok[i] == 1 ? T(sums[i] / ws[i]) : T(Inf) for i in 1:nt]
    grads = [dloss[(const_off[i] + 1):const_off[i + 1]] ./ ws[i] for i in 1:nt]
    return losses, grads, ok .== 1
end

"""
    optimize_constants_targets!(trees, js, datasets, options; device=0, row_idx=nothing)
        -> (losses, converged, num_evals)

optimize_constants_batch! for the members of several outputs in ONE lockstep run
(srhip_optimize_constants_targets): `trees[i]` is optimised against `datasets[js[i]]` (the outputs
of one MultiCopy). The start noise is drawn tree by tree, restart by restart, as
optimize_constants_batch! draws it. `row_idx` as there. Expression losses are `Unsupported`.
"""
function optimize_constants_targets!(trees::AbstractVector{Node{T}}, js::AbstractVector{<:Integer},
                                     datasets::AbstractVector{<:Dataset{T}}, options::Options;
                                     device::Int=0,
                                     row_idx::Union{Nothing,AbstractMatrix{<:Integer}}=nothing) where {T}
    algo = options.optimizer_algorithm == "BFGS" ? OPT_BFGS :
           options.optimizer_algorithm == "NelderMead" ? OPT_NELDERMEAD :
           error("Optimization function not implemented.")
    nt = length(trees)
    length(js) == nt || throw(ArgumentError("one output index per tree"))
    m = MultiCopy(datasets, device)
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    nr = options.optimizer_nrestarts
    noise = Float64[]
    for i in 1:nt
        nc = Int(const_off[i + 1] - const_off[i])
        nc == 0 && continue
        for _ in 1:nr
            append!(noise, Float64.(randn(T, nc)))
        end
    end
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    target = Int32.(js .- 1)
    out_c = similar(consts); out_l = Vector{Float64}(undef, nt)
    out_k = Vector{UInt8}(undef, nt); out_n = Vector{Float64}(undef, nt)
    if row_idx !== nothing
        size(row_idx, 2) == nt || throw(ArgumentError("one row sample (column of row_idx) per tree"))
    end
    rows = row_idx === nothing ? Matrix{Int64}(undef, 0, 0) : Matrix{Int64}(row_idx .- 1)
    GC.@preserve node_off kind arg const_off consts noise params target out_c out_l out_k out_n rows m datasets begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        opts = Ref(ConstOptOptions(algo, Int32(options.optimizer_options.iterations), Int32(nr), kindcode,
                                   pointer(params), pointer(noise), UInt64(0)))
        check(ccall((:srhip_optimize_constants_targets, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Ref{ConstOptOptions}, Ptr{Int32}, Ptr{Int64}, Int64,
                     Ptr{Cvoid}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}),
                    context(device), m.h, tr, opts, target,
                    row_idx === nothing ? Ptr{Int64}(C_NULL) : pointer(rows), size(rows, 1), out_c, out_l,
                    out_k, out_n))
    end
    converged = out_k .== 1
    for i in 1:nt
        converged[i] && set_constants(trees[i], out_c[(const_off[i] + 1):const_off[i + 1]])
    end
    return T.(out_l), converged, out_n
end

# ---- eval_tree_array (src/InterfaceDynamicExpressions.jl:50-52) -------------------
"""
    eval_tree_array(tree, X, options) -> (output, did_succeed)

Per-row outputs of one tree on the engine. X is (nfeatures, n); it is uploaded
for this call. On failure the output contents are unspecified, as in the
reference (an undef array).
"""
function eval_tree_array(tree::Node{T}, X::AbstractMatrix{T}, options::Options; device::Int=0) where {T}
    out, ok = eval_tree_array_batch([tree], X, options; device=device)
    return out[:, 1], ok[1]
end

"""
    eval_tree_array_batch(trees, X, options) -> (outputs::Matrix (n, ntrees), did_succeed::Vector{Bool})

Per-row outputs of many trees in one launch; X is uploaded for this call (it
may have changed since any earlier upload, as the reference re-reads it).
"""
function eval_tree_array_batch(trees::AbstractVector{Node{T}}, X::AbstractMatrix{T}, options::Options;
                               device::Int=0) where {T}
    n = size(X, 2)
    ds = upload(X, zeros(T, n), nothing, device)
    try
        return eval_tree_array_on(trees, ds, n, options, device)
    finally
        destroy_dataset(ds)
    end
end

"""
    eval_tree_array_batch(trees, dataset::Dataset, options) -> (outputs, did_succeed)

The same on a Dataset's X through its device copy (device_dataset, uploaded
once; a Dataset is not modified after construction). `dataset` and its
DeviceCopy are rooted across the call, so neither the WeakKeyDict entry nor
the device memory can be freed while the kernel reads it.
"""
function eval_tree_array_batch(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options;
                               device::Int=0) where {T}
    h = device_dataset(dataset, device)
    dcopy = lock(() -> DEVICE_DATASETS[dataset][device], CTX_LOCK)
    GC.@preserve dataset dcopy begin
        return eval_tree_array_on(trees, h, dataset.n, options, device)
    end
end

function eval_tree_array_on(trees::AbstractVector{Node{T}}, ds::Ptr{Cvoid}, n::Int, options::Options,
                            device::Int) where {T}
    nt = length(trees)
    p = Program(trees, options, device)
    out = Matrix{T}(undef, n, nt); ok = Vector{UInt8}(undef, nt)
    try
        GC.@preserve out ok check(ccall((:srhip_eval_tree_array, libsrhip), Int32,
                                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}), ds, p.h, out, ok))
    finally
        destroy(p)
    end
    return out, ok .== 1
end

# ---- eval_grad_tree_array (src/InterfaceDynamicExpressions.jl:83-107) -------------
"""
    eval_grad_tree_array(tree, X, options; variable=false) -> (output, gradient, did_succeed)

variable=false: gradient[k, i] = ∂ŷ_i/∂c_k for the constants in get_constants
order (srhip_eval_grad_tree_array). variable=true: gradient[f, i] = ∂ŷ_i/∂x_f,
computed by seeding each feature leaf x_f as (x_f + c) with c = -0.0 (x + -0.0
== x bit for bit, so values and did_succeed are unchanged) and summing the
seeds' tangents per feature; needs `+` among the binary operators, else
Unsupported.
"""
function eval_grad_tree_array(tree::Node{T}, X::AbstractMatrix{T}, options::Options;
                              variable::Bool=false, device::Int=0) where {T}
    nfeat, n = size(X)
    if !variable
        value, G, ok = _const_grads(tree, X, options, device)
        return value, permutedims(G), ok
    end
    plus = findfirst(op -> op === (+), options.operators.binops)
    plus === nothing && throw(Unsupported("variable=true needs + among the binary operators"))
    seeds = Int[]
    function seed(t::Node{T})
        if t.degree == 0
            t.constant && (push!(seeds, 0); return Node(T; val=t.val))
            push!(seeds, t.feature)
            return Node(plus, Node(T; feature=t.feature), Node(T; val=T(-0.0)))
        elseif t.degree == 1
            return Node(t.op, seed(t.l))
        else
            l = seed(t.l)
            return Node(t.op, l, seed(t.r))
        end
    end
    aug = seed(tree)
    value, G, ok = _const_grads(aug, X, options, device)
    grad = zeros(T, nfeat, n)
    for (k, f) in enumerate(seeds)
        f > 0 && (grad[f, :] .+= view(G, :, k))
    end
    return value, grad, ok
end

function _const_grads(tree::Node{T}, X::AbstractMatrix{T}, options::Options, device::Int) where {T}
    n = size(X, 2)
    ds = upload(X, zeros(T, n), nothing, device)
    p = Program([tree], options, device)
    ncon = Int(p.const_off[end])
    value = Vector{T}(undef, n); G = Matrix{T}(undef, n, ncon); ok = Ref{UInt8}(0)
    try
        GC.@preserve value G check(ccall((:srhip_eval_grad_tree_array, libsrhip), Int32,
                                         (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{UInt8}),
                                         ds, p.h, value, G, ok))
    finally
        destroy(p)
        destroy_dataset(ds)
    end
    return value, G, ok[] == 1
end

# ---- device groups (srhip.h "device groups"): one process, row shards over several GPUs ----
# A group owns one context and one driver thread per entry of `devices` (a device
# may be listed more than once). Its datasets hold one row shard per member, its
# programs one identical program per member, and an evaluation combines the
# shards on the device in member order. The search's islands do not go through
# the group calls: island k runs on device devices[k % ndev] through the
# single-device functions above (`device=`), see BatchedCallers.s_r_cycle_devices.
"""
    DeviceGroup(devices)

Open a device group (srhip_group_open) on `devices` (0-based device indices, 1
to 16 of them). Closed by `close!` or by the finaliser; the group datasets and
programs made through it are destroyed first.
"""
mutable struct DeviceGroup
    h::Ptr{Cvoid}
    devices::Vector{Int32}
    children::Vector{WeakRef}   # live GroupCopy / GroupProgram objects, destroyed before the group
end
function DeviceGroup(devices::AbstractVector{<:Integer})
    devs = Vector{Int32}(devices)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve devs check(ccall((:srhip_group_open, libsrhip), Int32, (Ptr{Int32}, Int32, Ptr{Ptr{Cvoid}}),
                                  devs, Int32(length(devs)), h))
    g = DeviceGroup(h[], devs, WeakRef[])
    finalizer(close!, g)
    return g
end
function close!(g::DeviceGroup)
    g.h == C_NULL && return nothing
    for r in g.children
        r.value === nothing || free!(r.value)
    end
    empty!(g.children)
    ccall((:srhip_group_close, libsrhip), Int32, (Ptr{Cvoid},), g.h)
    g.h = C_NULL
    return nothing
end
ndevices(g::DeviceGroup) = length(g.devices)

"""Member k's (0-based) context, lent (srhip_group_ctx): the group owns it."""
function group_context(g::DeviceGroup, k::Int)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:srhip_group_ctx, libsrhip), Int32, (Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}), g.h, Int32(k), h))
    return h[]
end

"""Rows (0-based, half-open) of member k of ndev over n rows (srhip_group_shard_range)."""
function shard_range(n::Integer, ndev::Integer, k::Integer)
    b = Ref{Int64}(0); e = Ref{Int64}(0)
    check(ccall((:srhip_group_shard_range, libsrhip), Int32, (Int64, Int32, Int32, Ptr{Int64}, Ptr{Int64}),
                Int64(n), Int32(ndev), Int32(k), b, e))
    return b[], e[]
end

# one sharded copy per (Dataset, group), uploaded once; held weakly like DEVICE_DATASETS
mutable struct GroupCopy
    h::Ptr{Cvoid}
    group::DeviceGroup
end
function free!(d::GroupCopy)
    (d.h == C_NULL || d.group.h == C_NULL) && (d.h = C_NULL; return nothing)
    ccall((:srhip_group_dataset_destroy, libsrhip), Int32, (Ptr{Cvoid},), d.h)
    d.h = C_NULL
    return nothing
end
const GROUP_DATASETS = WeakKeyDict{Dataset,IdDict{DeviceGroup,GroupCopy}}()
function group_dataset(dataset::Dataset{T}, group::DeviceGroup) where {T}
    lock(CTX_LOCK) do
        copies = get!(() -> IdDict{DeviceGroup,GroupCopy}(), GROUP_DATASETS, dataset)
        d = get(copies, group, nothing)
        d !== nothing && d.h != C_NULL && return d.h
        h = Ref{Ptr{Cvoid}}(C_NULL)
        Xc = Matrix{T}(dataset.X); yc = Vector{T}(dataset.y)
        wc = dataset.weighted ? Vector{T}(dataset.weights) : nothing
        nfeat, n = size(Xc)
        GC.@preserve Xc yc wc begin
            check(ccall((:srhip_group_dataset_create, libsrhip), Int32,
                        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Int64, Int32, Ptr{Ptr{Cvoid}}),
                        group.h, dtype_code(T), X_JULIA, Xc, yc, wc === nothing ? Ptr{T}(C_NULL) : wc, n, nfeat, h))
        end
        d = GroupCopy(h[], group)
        finalizer(free!, d)
        push!(group.children, WeakRef(d))
        copies[group] = d
        return d.h
    end
end

# one identical program per member (srhip_group_program_create)
mutable struct GroupProgram
    h::Ptr{Cvoid}
    ntrees::Int
    const_off::Vector{Int32}
    group::DeviceGroup
end
function free!(p::GroupProgram)
    (p.h == C_NULL || p.group.h == C_NULL) && (p.h = C_NULL; return nothing)
    ccall((:srhip_group_program_destroy, libsrhip), Int32, (Ptr{Cvoid},), p.h)
    p.h = C_NULL
    return nothing
end
destroy(p::GroupProgram) = free!(p)
function GroupProgram(trees::AbstractVector{Node{T}}, options::Options, group::DeviceGroup;
                      varying_constants::Bool=false, wide_tree_code::Bool=false) where {T}
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    flags = (varying_constants ? PROGRAM_VARYING_CONSTANTS : UInt32(0)) |
            (wide_tree_code ? PROGRAM_WIDE_TREE_CODE : UInt32(0))
    GC.@preserve node_off kind arg const_off consts begin
        tr = Ref(SrhipTrees(Int32(length(trees)), pointer(node_off), pointer(kind), pointer(arg),
                            pointer(const_off), Ptr{Cvoid}(pointer(consts))))
        check(ccall((:srhip_group_program_create, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Ref{SrhipTrees}, UInt32, Ptr{Ptr{Cvoid}}),
                    group.h, dtype_code(T), tr, flags, h))
    end
    p = GroupProgram(h[], length(trees), const_off, group)
    finalizer(free!, p)
    lock(() -> push!(group.children, WeakRef(p)), CTX_LOCK)
    return p
end
function set_constants!(p::GroupProgram, consts::Vector{T}) where {T}
    length(consts) == p.const_off[end] || throw(ArgumentError("expected $(p.const_off[end]) constants"))
    GC.@preserve consts check(ccall((:srhip_group_program_set_constants, libsrhip), Int32,
                                    (Ptr{Cvoid}, Ptr{Cvoid}), p.h, consts))
    return p
end

"""
    eval_loss_batch(trees, dataset, options, group::DeviceGroup) -> Vector{T}

`eval_loss_batch` with the dataset's rows sharded over `group` (all rows: no `idx`).
"""
function eval_loss_batch(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options,
                         group::DeviceGroup) where {T}
    nt = length(trees)
    p = GroupProgram(trees, options, group)
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Ref{Float64}(0)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    try
        GC.@preserve sums ok params check(ccall((:srhip_group_eval_loss, libsrhip), Int32,
                                                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64},
                                                 Ref{Float64}, Ptr{UInt8}),
                                                group_dataset(dataset, group), p.h, kindcode, params, sums, wsum, ok))
    finally
        destroy(p)
    end
    return [ok[i] == 1 ? T(sums[i] / wsum[]) : T(Inf) for i in 1:nt]
end

"""
    eval_loss_grad(p::GroupProgram, dataset, options) -> (losses, grads, ok)

`eval_loss_grad_batch` over the group of `p` (srhip_group_eval_loss_grad).
"""
function eval_loss_grad(p::GroupProgram, dataset::Dataset{T}, options::Options) where {T}
    nt = p.ntrees
    ncon = Int(p.const_off[end])
    sums = Vector{Float64}(undef, nt); ok = Vector{UInt8}(undef, nt); wsum = Ref{Float64}(0)
    dloss = Vector{Float64}(undef, ncon)
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    GC.@preserve sums ok dloss params begin
        check(ccall((:srhip_group_eval_loss_grad, libsrhip), Int32,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64},
                     Ptr{UInt8}),
                    group_dataset(dataset, p.group), p.h, kindcode, params, sums, dloss, wsum, ok))
    end
    losses = [ok[i] == 1 ? T(sums[i] / wsum[]) : T(Inf) for i in 1:nt]
    grads = [dloss[(p.const_off[i] + 1):p.const_off[i + 1]] ./ wsum[] for i in 1:nt]
    return losses, grads, ok .== 1
end

"""
    optimize_constants_batch!(trees, dataset, options, group::DeviceGroup) -> (losses, converged, num_evals)

`optimize_constants_batch!` with the dataset's rows sharded over `group`
(srhip_group_optimize_constants): the same optimiser and start noise.
"""
function optimize_constants_batch!(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options,
                                   group::DeviceGroup) where {T}
    algo = options.optimizer_algorithm == "BFGS" ? OPT_BFGS :
           options.optimizer_algorithm == "NelderMead" ? OPT_NELDERMEAD :
           error("Optimization function not implemented.")
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    nt = length(trees)
    nr = options.optimizer_nrestarts
    noise = Float64[]
    for i in 1:nt
        nc = Int(const_off[i + 1] - const_off[i])
        nc == 0 && continue
        for _ in 1:nr
            append!(noise, Float64.(randn(T, nc)))
        end
    end
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    out_c = similar(consts); out_l = Vector{Float64}(undef, nt)
    out_k = Vector{UInt8}(undef, nt); out_n = Vector{Float64}(undef, nt)
    GC.@preserve node_off kind arg const_off consts noise params out_c out_l out_k out_n begin
        tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                            Ptr{Cvoid}(pointer(consts))))
        opts = Ref(ConstOptOptions(algo, Int32(options.optimizer_options.iterations), Int32(nr), kindcode,
                                   pointer(params), pointer(noise), UInt64(0)))
        check(ccall((:srhip_group_optimize_constants, libsrhip), Int32,
                    (Ptr{Cvoid}, Ref{SrhipTrees}, Ref{ConstOptOptions}, Ptr{Cvoid}, Ptr{Float64}, Ptr{UInt8},
                     Ptr{Float64}),
                    group_dataset(dataset, group), tr, opts, out_c, out_l, out_k, out_n))
    end
    converged = out_k .== 1
    for i in 1:nt
        converged[i] && set_constants(trees[i], out_c[(const_off[i] + 1):const_off[i + 1]])
    end
    return T.(out_l), converged, out_n
end

# ---- derivative objectives (srhip.h "derivative objectives") -------------------------
"""
    DerivativeObjective(coefficients, directions, dydx; weights=nothing)

A `loss_function` that scores the prediction and its derivatives with respect to features
("a loss that takes into account derivatives", src/Options.jl:203-210):
`Σ_k coefficients[k] · mean_k`, where `mean_1` is the (weighted) mean of
`options.elementwise_loss` on `(ŷ, dataset.y)` and `mean_{1+j}` that of the same loss on
`(∂ŷ/∂x_d, dydx[j, :])` along `d = directions[j]` (1-based features, as
`eval_diff_tree_array`'s `direction`). `weights` is `nothing` (the dataset's own weights, if
any, on every channel) or `(1 + ndir, n)`, one row per channel. `T(Inf)` when an evaluation
does not complete or the result is not finite.

The method `(f)(tree, dataset, options)` is the CPU definition, built from
DynamicExpressions' `eval_tree_array` / `eval_diff_tree_array`, so the struct is a legal
`loss_function` on its own; `enabled(options)` accepts it and `eval_loss_deriv` /
`BatchedCallers.score_batch` score whole batches with one engine call
(srhip_eval_loss_deriv); `optimize_constants_deriv` fits the constants under it
(srhip_optimize_constants_deriv). Not covered there (the CPU definition runs): row samples
(`options.batching`), expression losses and operators.
"""
struct DerivativeObjective{T} <: Function
    coefficients::Vector{Float64}
    directions::Vector{Int}
    dydx::Matrix{T}                      # (ndir, n)
    weights::Union{Nothing,Matrix{T}}    # (1 + ndir, n) or nothing
    function DerivativeObjective(coefficients::AbstractVector{<:Real}, directions::AbstractVector{<:Integer},
                                 dydx::AbstractMatrix{T};
                                 weights::Union{Nothing,AbstractMatrix{T}}=nothing) where {T}
        nd = length(directions)
        1 <= nd <= 15 || throw(ArgumentError("1 to 15 directions"))
        allunique(directions) || throw(ArgumentError("directions must not repeat"))
        all(>=(1), directions) || throw(ArgumentError("directions are 1-based feature indices"))
        length(coefficients) == 1 + nd || throw(ArgumentError("one coefficient per channel: y, then one per direction"))
        size(dydx, 1) == nd || throw(ArgumentError("dydx must be (ndir, n)"))
        weights === nothing || size(weights) == (1 + nd, size(dydx, 2)) ||
            throw(ArgumentError("weights must be (1 + ndir, n)"))
        return new{T}(Float64.(coefficients), Int.(directions), Matrix{T}(dydx),
                      weights === nothing ? nothing : Matrix{T}(weights))
    end
end

# the weights of channel k (1 = y), or nothing
function channel_weights(f::DerivativeObjective{T}, dataset::Dataset{T}, k::Int) where {T}
    f.weights !== nothing && return f.weights[k, :]
    return dataset.weighted ? dataset.weights : nothing
end

function channel_mean(loss, pred::AbstractVector{T}, target::AbstractVector{T}, w) where {T}
    w === nothing && return Float64(LossFunctions.value(loss, target, pred, LossFunctions.AggMode.Mean()))
    return Float64(LossFunctions.value(loss, target, pred, LossFunctions.AggMode.WeightedMean(w)))
end

function (f::DerivativeObjective{T})(tree::Node{T}, dataset::Dataset{T}, options::Options)::T where {T}
    size(f.dydx, 2) == dataset.n || throw(ArgumentError("dydx has $(size(f.dydx, 2)) rows, the dataset $(dataset.n)"))
    all(<=(size(dataset.X, 1)), f.directions) || throw(ArgumentError("direction outside the dataset's features"))
    loss = options.elementwise_loss
    pred, complete = DynamicExpressions.eval_tree_array(tree, dataset.X, options.operators)
    complete || return T(Inf)
    total = f.coefficients[1] * channel_mean(loss, pred, dataset.y, channel_weights(f, dataset, 1))
    for (j, d) in enumerate(f.directions)
        _, g, complete = DynamicExpressions.eval_diff_tree_array(tree, dataset.X, options.operators, d)
        complete || return T(Inf)
        total += f.coefficients[1 + j] * channel_mean(loss, g, f.dydx[j, :], channel_weights(f, dataset, 1 + j))
    end
    return isfinite(total) ? T(total) : T(Inf)
end

"""
    eval_loss_deriv(trees, dataset, options; device=0) -> (losses, means, ok)

The derivative objective `options.loss_function::DerivativeObjective` for every tree in one
engine call (srhip_eval_loss_deriv): `losses[i] = T(Σ_k coefficients[k] · means[i, k])`,
`T(Inf)` where the tree fails or the result is not finite; `means` is (ntrees, 1 + ndir) in
Float64. The columns `[y; dydx]` go up once per call next to `dataset.X`
(srhip_dataset_create_multi). `Unsupported` for expression losses and expression operators
(the callers fall back to the CPU definition).
"""
function eval_loss_deriv(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options;
                         device::Int=0) where {T}
    f = options.loss_function::DerivativeObjective{T}
    nt = length(trees)
    nd = length(f.directions)
    nfeat, n = size(dataset.X)
    size(f.dydx, 2) == n || throw(ArgumentError("dydx has $(size(f.dydx, 2)) rows, the dataset $(n)"))
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    Xc = Matrix{T}(dataset.X)
    Yc = Matrix{T}(undef, n, 1 + nd)     # column k = channel k: [1 + ndir][n] in C
    Yc[:, 1] .= dataset.y
    for j in 1:nd
        Yc[:, 1 + j] .= f.dydx[j, :]
    end
    weighted = f.weights !== nothing || dataset.weighted
    Wc = weighted ? Matrix{T}(undef, n, 1 + nd) : nothing
    if weighted
        for k in 1:(1 + nd)
            Wc[:, k] .= channel_weights(f, dataset, k)
        end
    end
    dir = Int32.(f.directions .- 1)
    sums = Matrix{Float64}(undef, 1 + nd, nt)   # [ntrees][1 + ndir] in C
    wsum = Vector{Float64}(undef, 1 + nd)
    ok = Vector{UInt8}(undef, nt)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve node_off kind arg const_off consts Xc Yc Wc dir sums wsum ok params begin
        check(ccall((:srhip_dataset_create_multi, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Int64, Int32, Int32, Int64, Int64,
                     Ptr{Ptr{Cvoid}}),
                    context(device), dtype_code(T), X_JULIA, Xc, Yc,
                    Wc === nothing ? Ptr{T}(C_NULL) : Wc, n, nfeat, 1 + nd, 0, n, h))
        try
            tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                                Ptr{Cvoid}(pointer(consts))))
            check(ccall((:srhip_eval_loss_deriv_batch_ctx, libsrhip), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Int32, Ptr{Float64}, Ptr{Int32}, Int32,
                         Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                        context(device), h[], tr, kindcode, params, dir, Int32(nd), sums, wsum, ok))
        finally
            destroy_dataset(h[])
        end
    end
    means = permutedims(sums ./ wsum)
    losses = Vector{T}(undef, nt)
    for i in 1:nt
        v = sum(f.coefficients[k] * means[i, k] for k in 1:(1 + nd))
        losses[i] = (ok[i] == 1 && isfinite(v)) ? T(v) : T(Inf)
    end
    return losses, means, ok .== 1
end

"""
    optimize_constants_deriv(trees, dataset, options; device=0) -> (losses, converged, num_evals)

`optimize_constants_batch!` under `options.loss_function::DerivativeObjective`
(srhip_optimize_constants_deriv): every start of every tree in one lockstep run, the loss of a
candidate `Σ_k coefficients[k] · mean_k` over y and every derivative channel, its gradient
from second-order forward mode (∂²ŷ/∂c∂x). Trees that converged get their constants set.
`losses` are the objective values in `T`. `Unsupported` for expression losses, expression
operators and datasets whose row tile does not fit in LDS (the callers fall back to the
reference's optimiser).
"""
function optimize_constants_deriv(trees::AbstractVector{Node{T}}, dataset::Dataset{T}, options::Options;
                                  device::Int=0) where {T}
    f = options.loss_function::DerivativeObjective{T}
    algo = options.optimizer_algorithm == "BFGS" ? OPT_BFGS :
           options.optimizer_algorithm == "NelderMead" ? OPT_NELDERMEAD :
           error("Optimization function not implemented.")
    nt = length(trees)
    nd = length(f.directions)
    nfeat, n = size(dataset.X)
    size(f.dydx, 2) == n || throw(ArgumentError("dydx has $(size(f.dydx, 2)) rows, the dataset $(n)"))
    node_off, kind, arg, const_off, consts = flatten(trees, options)
    nr = options.optimizer_nrestarts
    noise = Float64[]
    for i in 1:nt
        nc = Int(const_off[i + 1] - const_off[i])
        nc == 0 && continue
        for _ in 1:nr
            append!(noise, Float64.(randn(T, nc)))
        end
    end
    kindcode, param = loss_code(options.elementwise_loss)
    params = Float64[param]
    Xc = Matrix{T}(dataset.X)
    Yc = Matrix{T}(undef, n, 1 + nd)
    Yc[:, 1] .= dataset.y
    for j in 1:nd
        Yc[:, 1 + j] .= f.dydx[j, :]
    end
    weighted = f.weights !== nothing || dataset.weighted
    Wc = weighted ? Matrix{T}(undef, n, 1 + nd) : nothing
    if weighted
        for k in 1:(1 + nd)
            Wc[:, k] .= channel_weights(f, dataset, k)
        end
    end
    dir = Int32.(f.directions .- 1)
    coef = Float64.(f.coefficients)
    out_c = similar(consts); out_l = Vector{Float64}(undef, nt)
    out_k = Vector{UInt8}(undef, nt); out_n = Vector{Float64}(undef, nt)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve node_off kind arg const_off consts noise params Xc Yc Wc dir coef out_c out_l out_k out_n begin
        check(ccall((:srhip_dataset_create_multi, libsrhip), Int32,
                    (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Int64, Int32, Int32, Int64, Int64,
                     Ptr{Ptr{Cvoid}}),
                    context(device), dtype_code(T), X_JULIA, Xc, Yc,
                    Wc === nothing ? Ptr{T}(C_NULL) : Wc, n, nfeat, 1 + nd, 0, n, h))
        try
            tr = Ref(SrhipTrees(Int32(nt), pointer(node_off), pointer(kind), pointer(arg), pointer(const_off),
                                Ptr{Cvoid}(pointer(consts))))
            opts = Ref(ConstOptOptions(algo, Int32(options.optimizer_options.iterations), Int32(nr), kindcode,
                                       pointer(params), pointer(noise), UInt64(0)))
            check(ccall((:srhip_optimize_constants_deriv, libsrhip), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ref{SrhipTrees}, Ref{ConstOptOptions}, Ptr{Int32}, Int32,
                         Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}),
                        context(device), h[], tr, opts, dir, Int32(nd), coef, out_c, out_l, out_k, out_n))
        finally
            destroy_dataset(h[])
        end
    end
    converged = out_k .== 1
    for i in 1:nt
        converged[i] && set_constants(trees[i], out_c[(const_off[i] + 1):const_off[i + 1]])
    end
    return T.(out_l), converged, out_n
end

end # module
