# BatchedCallers.jl — the hot path's callers, batched (SURVEY.md §8 a10 / f1).
#
# The reference scores one candidate at a time: next_generation
# (src/Mutate.jl:26-255) calls score_func per mutated tree inside
# reg_evol_cycle (src/RegularizedEvolution.jl:13-155), Population(...)
# (src/Population.jl:31-46) and finalize_scores (:134-148) score member by
# member. This module keeps those algorithms and moves the scoring out of the
# per-candidate loop, so that one SRHip.eval_loss_batch launch scores every
# candidate of a step:
#
#   * `population_batched`      — Population(dataset; npop, nlength, options, nfeatures)
#   * `finalize_scores_batched` — finalize_scores(dataset, pop, options)
#   * `reg_evol_cycle_lockstep` — reg_evol_cycle with the reference's DEFAULT
#     semantics (fast_cycle = false: best_of_sample, next_generation or
#     crossover_generation, replace-oldest, step by step per island), every
#     island's candidates of a step — both crossover children included — in
#     one launch; `s_r_cycle_lockstep` runs a whole s_r_cycle that way.
#   * `reg_evol_cycle_batched`  — reg_evol_cycle with fast_cycle semantics
#     (one baby per tournament_selection_n-member subsample, replace-oldest),
#     for several islands in lockstep: every island's babies in one launch,
#     and every `:optimize` mutation of the cycle in one batched optimiser call.
#   * `optimize_constants_batched` — optimize_constants (src/ConstantOptimization.jl:22-65)
#     for many members: SRHip.optimize_constants_batch! (srhip_optimize_constants_batch,
#     all starts of all members in lockstep, one launch per phase).
#   * `optimize_and_simplify_population_batched` — optimize_and_simplify_population
#     (src/SingleIteration.jl:63-123): the members drawn for optimisation go
#     through one batched optimiser call instead of one Optim run each.
#   * every function above that ends in an SRHip call takes `device::Int=0` and passes
#     it down; `s_r_cycle_devices` runs the islands with (k - 1) % ndev == d on the
#     d-th device of an SRHip.DeviceGroup, one task per device (INTEGRATION.md §4).
#
# next_generation is split into `propose` (mutation choice, attempts,
# check_constraints — everything before score_func, calling the reference's
# own mutation functions) and `accept` (the NaN rejection and the
# annealing / adaptive-parsimony acceptance rule after it). A candidate whose
# mutation needs no score (simplify, optimize, do_nothing, a failed
# constraint check) is decided in `propose`, as in the reference.
#
# UNTESTED AS JULIA (no Julia in the build image). The Python mirrors of the
# same lockstep loops (symbolicregression.jl_amd/srhip/evolution.py for the
# default path, srhip/search.py for fast_cycle) run in the test suite; tests/test_julia_binding.py checks this file's references to
# the reference's functions and to SRHip statically.
module BatchedCallers

import DynamicExpressions: Node, copy_node, count_constants, count_depth, simplify_tree, combine_operators
import ..CoreModule: Options, Dataset, RecordType, sample_mutation
import ..ComplexityModule: compute_complexity
import ..LossFunctionsModule: score_func, score_func_batch, loss_to_score
import ..CheckConstraintsModule: check_constraints
import ..AdaptiveParsimonyModule: RunningSearchStatistics
import ..PopMemberModule: PopMember, copy_pop_member
import ..PopulationModule: Population, best_of_sample
import ..HallOfFameModule: HallOfFame
import ..MutationFunctionsModule:
    gen_random_tree, gen_random_tree_fixed_size, mutate_constant, mutate_operator, append_random_op,
    prepend_random_op, insert_random_op, delete_random_op, crossover_trees
import ..ConstantOptimizationModule: optimize_constants
import ..UtilsModule: get_birth_order
import ..PopMemberModule: generate_reference
import ..RecorderModule: @recorder
import ..SingleIterationModule: s_r_cycle
import DynamicExpressions: string_tree
import ..SRHip

"""
    score_batch(dataset, trees, options) -> (scores, losses)

score_func (src/LossFunctions.jl:86-92) for every tree: one SRHip launch when
the engine covers the options (a `loss_function` that is a
SRHip.DerivativeObjective included: SRHip.eval_loss_deriv), else the reference,
tree by tree.
"""
function score_batch(dataset::Dataset{T}, trees::AbstractVector{Node{T}}, options::Options;
                     device::Int=0) where {T}
    if !isempty(trees) && SRHip.enabled(options)
        try
            # a derivative objective: every channel of every tree in one fused call
            if options.loss_function isa SRHip.DerivativeObjective
                losses = SRHip.eval_loss_deriv(trees, dataset, options; device=device)[1]
            else
                losses = SRHip.eval_loss_batch(trees, dataset, options; device=device)
            end
            scores = [loss_to_score(l, dataset.baseline_loss, t, options) for (l, t) in zip(losses, trees)]
            return scores, losses
        catch e
            e isa SRHip.Unsupported || rethrow()
        end
    end
    pairs = [score_func(dataset, t, options) for t in trees]
    return T[p[1] for p in pairs], T[p[2] for p in pairs]
end

"""
    score_batch_minibatch(dataset, trees, options) -> (scores, losses)

score_func_batch (src/LossFunctions.jl:95-115) for every tree: each tree on
its OWN sample of batch_size rows drawn with replacement, as the reference
draws one per call (:98), all trees in one launch
(SRHip.eval_loss_batch_rowsets); a failed evaluation scores (0, Inf) as in
the reference.
"""
function score_batch_minibatch(dataset::Dataset{T}, trees::AbstractVector{Node{T}}, options::Options;
                               device::Int=0) where {T}
    # (a loss_function, a DerivativeObjective included, is scored on all rows only)
    if !isempty(trees) && SRHip.enabled(options) && options.loss_function === nothing
        try
            idx = rand(1:(dataset.n), options.batch_size, length(trees))  # column t: tree t's sample
            losses = SRHip.eval_loss_batch_rowsets(trees, dataset, options, idx; device=device)
            scores = [isfinite(l) ? loss_to_score(l, dataset.baseline_loss, t, options) : zero(T)
                      for (l, t) in zip(losses, trees)]
            return scores, losses
        catch e
            e isa SRHip.Unsupported || rethrow()
        end
    end
    pairs = [score_func_batch(dataset, t, options) for t in trees]
    return T[p[1] for p in pairs], T[p[2] for p in pairs]
end

"""
    score_batch_multi(datasets, js, trees, options) -> (scores, losses)

One step's candidates from several outputs of a multi-output search in ONE call:
`trees[i]` belongs to output `js[i]` and is scored against `datasets[js[i]]`, the
Datasets EquationSearch builds over one shared `X` (src/SymbolicRegression.jl:304-315),
uploaded once (SRHip.MultiCopy). With `options.batching` every tree gets its own row
sample, as score_batch_minibatch. Outside the engine's coverage (`Unsupported`, or
datasets that do not share their X): score_batch / score_batch_minibatch per output.
"""
function score_batch_multi(datasets::AbstractVector{<:Dataset{T}}, js::AbstractVector{<:Integer},
                           trees::AbstractVector{Node{T}}, options::Options; device::Int=0) where {T}
    length(js) == length(trees) || throw(ArgumentError("one output index per tree"))
    shared = all(d -> d.X === datasets[1].X && d.weighted == datasets[1].weighted, datasets)
    if !isempty(trees) && shared && SRHip.enabled(options) && options.loss_function === nothing
        try
            if options.batching
                idx = rand(1:(datasets[1].n), options.batch_size, length(trees))  # column t: tree t's sample
                losses = SRHip.eval_loss_batch_targets_rowsets(trees, js, datasets, options, idx; device=device)
                scores = [isfinite(l) ? loss_to_score(l, datasets[j].baseline_loss, t, options) : zero(T)
                          for (l, t, j) in zip(losses, trees, js)]
            else
                losses = SRHip.eval_loss_batch_targets(trees, js, datasets, options; device=device)
                scores = [loss_to_score(l, datasets[j].baseline_loss, t, options)
                          for (l, t, j) in zip(losses, trees, js)]
            end
            return scores, losses
        catch e
            e isa SRHip.Unsupported || rethrow()
        end
    end
    scores = Vector{T}(undef, length(trees)); losses = Vector{T}(undef, length(trees))
    for j in unique(js)   # regroup by output, score, scatter back
        sel = findall(==(j), js)
        sub = Node{T}[trees[i] for i in sel]
        sc, lo = options.batching ? score_batch_minibatch(datasets[j], sub, options; device=device) :
                 score_batch(datasets[j], sub, options; device=device)
        scores[sel] .= sc
        losses[sel] .= lo
    end
    return scores, losses
end

# ---- Population / finalize_scores ---------------------------------------------------

"""Population(dataset; npop, nlength, options, nfeatures) with one launch."""
function population_batched(dataset::Dataset{T}; npop::Int, nlength::Int=3, options::Options,
                            nfeatures::Int, device::Int=0) where {T}
    trees = [gen_random_tree(nlength, options, nfeatures, T) for _ in 1:npop]
    scores, losses = score_batch(dataset, trees, options; device=device)
    members = [PopMember(trees[i], scores[i], losses[i]; parent=-1, deterministic=options.deterministic)
               for i in 1:npop]
    return Population{T}(members, npop)
end

"""finalize_scores (src/Population.jl:134-148): with batching, every member is
re-scored on the full dataset — one launch for the population."""
function finalize_scores_batched(dataset::Dataset{T}, pop::Population, options::Options;
                                 device::Int=0) where {T}
    options.batching || return (pop, 0.0)
    scores, losses = score_batch(dataset, [m.tree for m in pop.members], options; device=device)
    for (m, s, l) in zip(pop.members, scores, losses)
        m.score = s
        m.loss = l
    end
    return (pop, pop.n * (options.batch_size / dataset.n))
end

# ---- constant optimisation ---------------------------------------------------------------

"""
    optimize_constants_batched(dataset, members, options) -> num_evals::Vector{Float64}

optimize_constants (src/ConstantOptimization.jl:22-65) for every member at once,
updated in place: a converged member gets the optimised constants, its
score_func re-score (:58) and a new birth (:60); the others keep x0 (:62).
One SRHip call when the engine covers the options, else the reference member
by member.

`minibatch` (default false: the reference's v0.15.0 behaviour, which optimises on
the full dataset even with options.batching, src/ConstantOptimization.jl:16): with
`minibatch && options.batching` every member is optimised on its own sample of
options.batch_size rows drawn with replacement, where and how score_func_batch
draws them (src/LossFunctions.jl:98), the same rows for all of its starts and
iterations; a converged member's loss is the one on its sample, and num_evals is
scaled by batch_size / dataset.n (src/Mutate.jl:43). The CPU fall-back is the
reference's full-data optimiser either way.
"""
function optimize_constants_batched(dataset::Dataset{T}, members::AbstractVector{<:PopMember{T}},
                                    options::Options; device::Int=0, minibatch::Bool=false) where {T}
    isempty(members) && return Float64[]
    # a derivative objective: every member on all rows in one lockstep run (srhip_optimize_constants_deriv)
    if SRHip.enabled(options) && options.loss_function isa SRHip.DerivativeObjective
        try
            trees = Node{T}[m.tree for m in members]
            losses, converged, num_evals = SRHip.optimize_constants_deriv(trees, dataset, options; device=device)
            for (m, l, c) in zip(members, losses, converged)
                c || continue
                m.score = loss_to_score(l, dataset.baseline_loss, m.tree, options)
                m.loss = l
                m.birth = get_birth_order(; deterministic=options.deterministic)
            end
            return num_evals
        catch e
            e isa SRHip.Unsupported || rethrow()
        end
    end
    if SRHip.enabled(options) && options.loss_function === nothing
        try
            trees = Node{T}[m.tree for m in members]
            sampled = minibatch && options.batching
            # column t: member t's sample
            row_idx = sampled ? rand(1:(dataset.n), options.batch_size, length(trees)) : nothing
            losses, converged, num_evals = SRHip.optimize_constants_batch!(trees, dataset, options; device=device,
                                                                           row_idx=row_idx)
            sampled && (num_evals = num_evals .* (options.batch_size / dataset.n))
            for (m, l, c) in zip(members, losses, converged)
                c || continue
                m.score = loss_to_score(l, dataset.baseline_loss, m.tree, options)
                m.loss = l
                m.birth = get_birth_order(; deterministic=options.deterministic)
            end
            return num_evals
        catch e
            e isa SRHip.Unsupported || rethrow()
        end
    end
    evals = zeros(Float64, length(members))
    for (j, m) in enumerate(members)
        _, evals[j] = optimize_constants(dataset, m, options)
    end
    return evals
end

# Members per call up to which optimize_constants_batched_multi runs the fused optimiser
# by default (DESIGN.md §3.17, profiles/grad_targets_timing.json): the largest measured batch
# at which all three fused medians lie below those of one call per output (4 × 256 members on
# 100k rows: 274 ms against 362 ms); nothing larger was measured (`fused=true` forces it).
const FUSED_CONSTOPT_MAX_MEMBERS = 1024

"""
    optimize_constants_batched_multi(datasets, js, members, options) -> num_evals::Vector{Float64}

optimize_constants_batched for the members of several outputs of a multi-output search in ONE
lockstep run: `members[i]` belongs to output `js[i]` and is optimised against `datasets[js[i]]`,
the Datasets EquationSearch builds over one shared `X` (src/SymbolicRegression.jl:304-315,
:459-494), uploaded once (SRHip.MultiCopy). A converged member's score uses
`datasets[js[i]].baseline_loss`. `minibatch` as optimize_constants_batched. `fused` (default: up
to FUSED_CONSTOPT_MAX_MEMBERS members) forces the fused run or the per-output calls. Outside the
engine's coverage (`Unsupported`, or datasets that do not share their X):
optimize_constants_batched per output.
"""
function optimize_constants_batched_multi(datasets::AbstractVector{<:Dataset{T}}, js::AbstractVector{<:Integer},
                                          members::AbstractVector{<:PopMember{T}}, options::Options;
                                          device::Int=0, minibatch::Bool=false,
                                          fused::Union{Nothing,Bool}=nothing) where {T}
    length(js) == length(members) || throw(ArgumentError("one output index per member"))
    isempty(members) && return Float64[]
    shared = all(d -> d.X === datasets[1].X && d.weighted == datasets[1].weighted, datasets)
    use_fused = fused === nothing ? length(members) <= FUSED_CONSTOPT_MAX_MEMBERS : fused
    if use_fused && shared && SRHip.enabled(options) && options.loss_function === nothing
        try
            trees = Node{T}[m.tree for m in members]
            sampled = minibatch && options.batching
            n = datasets[1].n
            row_idx = sampled ? rand(1:n, options.batch_size, length(trees)) : nothing  # column t: member t's sample
            losses, converged, num_evals = SRHip.optimize_constants_targets!(trees, js, datasets, options;
                                                                             device=device, row_idx=row_idx)
            sampled && (num_evals = num_evals .* (options.batch_size / n))
            for (m, l, c, j) in zip(members, losses, converged, js)
                c || continue
                m.score = loss_to_score(l, datasets[j].baseline_loss, m.tree, options)
                m.loss = l
                m.birth = get_birth_order(; deterministic=options.deterministic)
            end
            return num_evals
        catch e
            e isa SRHip.Unsupported || rethrow()
        end
    end
    evals = zeros(Float64, length(members))
    for j in unique(js)   # regroup by output, optimise, scatter back
        sel = findall(==(j), js)
        evals[sel] .= optimize_constants_batched(datasets[j], members[sel], options; device=device,
                                                 minibatch=minibatch)
    end
    return evals
end

"""
    optimize_and_simplify_population_batched(dataset, pop, options, curmaxsize, record) -> (pop, num_evals)

optimize_and_simplify_population (src/SingleIteration.jl:63-123) with the
members drawn for optimisation (rand(pop.n) .< optimizer_probability)
optimised in one batched call and finalize_scores as one launch; the
simplification, the new references and the record are the reference's.
"""
function optimize_and_simplify_population_batched(dataset::Dataset{T}, pop::Population, options::Options,
                                                  curmaxsize::Int, record::RecordType; device::Int=0,
                                                  minibatch::Bool=false) where {T}
    do_optimization = rand(pop.n) .< options.optimizer_probability
    for j in 1:(pop.n)
        pop.members[j].tree = simplify_tree(pop.members[j].tree, options.operators)
        pop.members[j].tree = combine_operators(pop.members[j].tree, options.operators)
    end
    chosen = options.should_optimize_constants ? findall(do_optimization) : Int[]
    num_evals = sum(optimize_constants_batched(dataset, pop.members[chosen], options; device=device,
                                               minibatch=minibatch); init=0.0)
    pop, tmp_num_evals = finalize_scores_batched(dataset, pop, options; device=device)
    num_evals += tmp_num_evals
    for j in 1:(pop.n)
        old_ref = pop.members[j].ref
        new_ref = generate_reference()
        pop.members[j].parent = old_ref
        pop.members[j].ref = new_ref
        @recorder begin
            @assert haskey(record, "mutations")
            member = pop.members[j]
            if !haskey(record["mutations"], "$(member.ref)")
                record["mutations"]["$(member.ref)"] = RecordType(
                    "events" => Vector{RecordType}(), "tree" => string_tree(member.tree, options.operators),
                    "score" => member.score, "loss" => member.loss, "parent" => member.parent)
            end
            kind = (do_optimization[j] && options.should_optimize_constants) ? "simplification_and_optimization" :
                   "simplification"
            push!(record["mutations"]["$(old_ref)"]["events"],
                  RecordType("type" => "tuning", "time" => time(), "child" => new_ref,
                             "mutation" => RecordType("type" => kind)))
            push!(record["mutations"]["$(old_ref)"]["events"], RecordType("type" => "death", "time" => time()))
        end
    end
    return (pop, num_evals)
end

# ---- next_generation, split around its score_func call ---------------------------------

# A proposal: either decided (`member` set: no score needed) or a tree to score.
struct Proposal{T}
    parent::PopMember{T}
    tree::Union{Node{T},Nothing}
    member::Union{PopMember{T},Nothing}
    accepted::Bool
    num_evals::Float64
    # beforeScore / beforeLoss (src/Mutate.jl:41-47): the parent's own, or with
    # options.batching its re-score on a fresh minibatch
    before_score::T
    before_loss::T
    # an `:optimize` mutation (src/Mutate.jl:147-152): `member` holds the copy to
    # optimise; reg_evol_cycle_batched optimises all of them in one batched call
    optimize::Bool
end
Proposal{T}(parent, tree, member, accepted, num_evals, bs, bl) where {T} =
    Proposal{T}(parent, tree, member, accepted, num_evals, bs, bl, false)

# the tree-producing mutations of next_generation (src/Mutate.jl:79-115,132-139),
# through the reference's own mutation functions
function mutate_tree(choice::Symbol, tree::Node{T}, temperature, curmaxsize::Int, options::Options,
                     nfeatures::Int) where {T}
    choice == :mutate_constant && return mutate_constant(tree, temperature, options)
    choice == :mutate_operator && return mutate_operator(tree, options)
    choice == :add_node && return rand() < 0.5 ? append_random_op(tree, options, nfeatures) :
                                                 prepend_random_op(tree, options, nfeatures)
    choice == :insert_node && return insert_random_op(tree, options, nfeatures)
    choice == :delete_node && return delete_random_op(tree, options, nfeatures)
    choice == :randomize && return gen_random_tree_fixed_size(rand(1:curmaxsize), options, nfeatures, T)
    error("Unknown mutation choice: $choice")
end

"""Everything of next_generation before score_func (src/Mutate.jl:26-193);
`before` = (beforeScore, beforeLoss), already re-scored on a minibatch by the
caller when options.batching (:41-47)."""
function propose(dataset::Dataset{T}, member::PopMember{T}, before::Tuple{T,T}, temperature,
                 curmaxsize::Int, options::Options) where {T}
    prev = member.tree
    bs, bl = before
    keep(tree, accepted, evals=0.0) = Proposal{T}(member, nothing,
        PopMember(tree, bs, bl; parent=member.ref, deterministic=options.deterministic),
        accepted, evals, bs, bl)
    weights = copy(options.mutation_weights)
    weights.mutate_constant *= min(8, count_constants(prev)) / 8.0
    if compute_complexity(prev, options) >= curmaxsize || count_depth(prev) >= options.maxdepth
        weights.add_node = 0.0
        weights.insert_node = 0.0
    end
    choice = sample_mutation(weights)
    choice == :do_nothing && return keep(prev, true)
    if choice == :simplify
        return keep(combine_operators(simplify_tree(copy_node(prev), options.operators), options.operators), true)
    end
    if choice == :optimize  # optimised with the cycle's other :optimize proposals (reg_evol_cycle_batched)
        m = PopMember(copy_node(prev), bs, bl; parent=member.ref, deterministic=options.deterministic)
        return Proposal{T}(member, nothing, m, true, 0.0, bs, bl, true)
    end
    for _ in 1:10  # max_attempts
        tree = mutate_tree(choice, copy_node(prev), temperature, curmaxsize, options, dataset.nfeatures)
        check_constraints(tree, options, curmaxsize) &&
            return Proposal{T}(member, tree, nothing, false, 0.0, bs, bl)
    end
    return keep(copy_node(prev), false)  # failed constraint check: rejected
end

"""Everything of next_generation after score_func (src/Mutate.jl:207-255)."""
function accept(p::Proposal{T}, score::T, loss::T, temperature, stats::RunningSearchStatistics,
                options::Options) where {T}
    member = p.parent
    reject() = (PopMember(copy_node(member.tree), p.before_score, p.before_loss; parent=member.ref,
                          deterministic=options.deterministic), false)
    isnan(score) && return reject()
    prob = 1.0
    if options.annealing
        prob *= exp(-(score - p.before_score) / (temperature * options.alpha))
    end
    if options.use_frequency
        freq(c) = 0 < c <= options.maxsize ? stats.normalized_frequencies[c] : 1e-6
        prob *= freq(compute_complexity(member.tree, options)) / freq(compute_complexity(p.tree, options))
    end
    prob < rand() && return reject()
    return (PopMember(p.tree, score, loss; parent=member.ref, deterministic=options.deterministic), true)
end

# ---- reg_evol_cycle, fast_cycle semantics, islands in lockstep ------------------------

"""
    reg_evol_cycle_batched(dataset, pops, temperature, curmaxsize, stats, options) -> (pops, num_evals)

One fast_cycle pass (src/RegularizedEvolution.jl:33-79) over every island
of `pops` at once: shuffle each population, take the best of every
tournament_selection_n-member subsample, propose one baby each, score ALL
islands' babies in one launch, then accept and replace the oldest member
per island, in the reference's order.
"""
function reg_evol_cycle_batched(dataset::Dataset{T}, pops::AbstractVector{<:Population}, temperature,
                                curmaxsize::Int, stats::AbstractVector{RunningSearchStatistics},
                                options::Options; device::Int=0, minibatch::Bool=false) where {T}
    # this cycle's scoring and optimiser calls, on its device (minibatch: the :optimize mutations
    # optimise on per-member row samples, optimize_constants_batched)
    score_batch(ds, ts, o) = BatchedCallers.score_batch(ds, ts, o; device=device)
    score_batch_minibatch(ds, ts, o) = BatchedCallers.score_batch_minibatch(ds, ts, o; device=device)
    optimize_constants_batched(ds, ms, o) = BatchedCallers.optimize_constants_batched(ds, ms, o; device=device)
    optimize_sampled(ds, ms, o) = BatchedCallers.optimize_constants_batched(ds, ms, o; device=device, minibatch=true)
    proposals = Vector{Vector{Proposal{T}}}(undef, length(pops))
    allstars = Vector{Vector{PopMember{T}}}(undef, length(pops))
    for (k, pop) in enumerate(pops)
        shuffle!(pop.members)
        ncyc = round(Int, pop.n / options.tournament_selection_n)
        allstars[k] = [begin
                           sub = (1 + (i - 1) * options.tournament_selection_n):(i * options.tournament_selection_n)
                           pop.members[sub[argmin([pop.members[j].score for j in sub])]]
                       end for i in 1:ncyc]
    end
    # with options.batching, every next_generation first re-scores its parent
    # on a minibatch (src/Mutate.jl:41-47): one launch for all islands' parents
    parents = PopMember{T}[m for as in allstars for m in as]
    num_evals = 0.0
    before = if options.batching
        ps, pl = score_batch_minibatch(dataset, Node{T}[m.tree for m in parents], options)
        num_evals += length(parents) * (options.batch_size / dataset.n)
        collect(zip(ps, pl))
    else
        [(m.score, m.loss) for m in parents]
    end
    q = 0
    for (k, as) in enumerate(allstars)
        props = Vector{Proposal{T}}(undef, length(as))
        off = q
        Threads.@threads for i in eachindex(as)
            props[i] = propose(dataset, as[i], before[off + i], temperature, curmaxsize, options)
        end
        q += length(as)
        proposals[k] = props
    end
    # every :optimize mutation of every island in one batched optimiser call
    to_opt = PopMember{T}[p.member for props in proposals for p in props if p.optimize]
    opt_evals = minibatch ? optimize_sampled(dataset, to_opt, options) :
                optimize_constants_batched(dataset, to_opt, options)
    num_evals += sum(opt_evals; init=0.0)
    # one launch for every island's babies
    trees = Node{T}[p.tree for props in proposals for p in props if p.member === nothing]
    scores, losses = options.batching ? score_batch_minibatch(dataset, trees, options) :
                     score_batch(dataset, trees, options)
    num_evals += length(trees) * (options.batching ? options.batch_size / dataset.n : 1.0)
    j = 0
    for (k, pop) in enumerate(pops)
        for p in proposals[k]
            num_evals += p.num_evals
            baby, accepted = if p.member === nothing
                j += 1
                accept(p, scores[j], losses[j], temperature, stats[k], options)
            else
                (p.member, p.accepted)
            end
            oldest = argmin([m.birth for m in pop.members])
            (accepted || !options.skip_mutation_failures) && (pop.members[oldest] = baby)
        end
    end
    return pops, num_evals
end

shuffle!(v) = (for i in length(v):-1:2; j = rand(1:i); v[i], v[j] = v[j], v[i]; end; v)

# ---- reg_evol_cycle, DEFAULT semantics (fast_cycle = false), islands in lockstep ----------

# One island's step in flight: a mutation (Proposal) or a crossover pair.
struct Step{T}
    crossover::Bool
    prop::Union{Proposal{T},Nothing}        # mutation: next_generation's proposal
    parents::Tuple{Vararg{PopMember{T}}}     # crossover: (allstar1, allstar2)
    children::Union{Tuple{Node{T},Node{T}},Nothing}  # crossover children; nothing = failed constraints
end

"""
    crossover_children(m1, m2, curmaxsize, options) -> (child1, child2) or nothing

crossover_generation (src/Mutate.jl:285-313) up to its score_func calls:
crossover_trees until both children pass check_constraints, at most 11 tries.
"""
function crossover_children(m1::PopMember{T}, m2::PopMember{T}, curmaxsize::Int, options::Options) where {T}
    c1, c2 = crossover_trees(m1.tree, m2.tree)
    num_tries = 1
    while !(check_constraints(c1, options, curmaxsize) && check_constraints(c2, options, curmaxsize))
        num_tries > 10 && return nothing
        c1, c2 = crossover_trees(m1.tree, m2.tree)
        num_tries += 1
    end
    return (c1, c2)
end

"""
    reg_evol_cycle_lockstep(dataset, pops, temperature, curmaxsize, stats, options) -> (pops, num_evals)

reg_evol_cycle with the reference's DEFAULT semantics (src/RegularizedEvolution.jl:81-155:
`fast_cycle = false`, crossover with probability `crossover_probability`,
`best_of_sample` tournaments with `tournament_selection_p`) for every island
of `pops` in lockstep. Each of the round(npop / tournament_selection_n) steps
is taken by every island together: its own `rand() > crossover_probability`
draw, `best_of_sample` (once, or twice for crossover), the mutation proposal
or the crossover children; then ALL islands' candidates — every mutated tree
and both children of every crossover — are scored in ONE launch, and each
island accepts and replaces its oldest member(s) in the reference's order.
Within an island the steps stay sequential (step i+1's tournament sees step
i's replacement), so each island runs the reference's algorithm unchanged;
`stats[k]` is island k's RunningSearchStatistics (the copy its worker holds).
The Python mirror (srhip/evolution.py) is tested to give, over the oracle,
exactly the serial per-island result.
"""
function reg_evol_cycle_lockstep(dataset::Dataset{T}, pops::AbstractVector{<:Population}, temperature,
                                 curmaxsize::Int, stats::AbstractVector{RunningSearchStatistics},
                                 options::Options; device::Int=0, minibatch::Bool=false) where {T}
    # this cycle's scoring and optimiser calls, on its device (minibatch: the :optimize mutations
    # optimise on per-member row samples, optimize_constants_batched)
    score_batch(ds, ts, o) = BatchedCallers.score_batch(ds, ts, o; device=device)
    score_batch_minibatch(ds, ts, o) = BatchedCallers.score_batch_minibatch(ds, ts, o; device=device)
    optimize_constants_batched(ds, ms, o) = BatchedCallers.optimize_constants_batched(ds, ms, o; device=device)
    optimize_sampled(ds, ms, o) = BatchedCallers.optimize_constants_batched(ds, ms, o; device=device, minibatch=true)
    num_evals = 0.0
    nsteps = round(Int, pops[1].n / options.tournament_selection_n)
    for _ in 1:nsteps
        steps = Vector{Step{T}}(undef, length(pops))
        # tournaments first: each island's crossover draw and best_of_sample
        allstars = Vector{Union{PopMember{T},Nothing}}(nothing, length(pops))
        for (k, pop) in enumerate(pops)
            if rand() > options.crossover_probability
                allstars[k] = best_of_sample(pop, stats[k], options)
            else
                a1 = best_of_sample(pop, stats[k], options)
                a2 = best_of_sample(pop, stats[k], options)
                steps[k] = Step{T}(true, nothing, (a1, a2), crossover_children(a1, a2, curmaxsize, options))
            end
        end
        # with options.batching every next_generation re-scores its parent on a
        # fresh minibatch (src/Mutate.jl:41-47): all islands' parents in ONE launch,
        # each on its own sample
        mut = findall(a -> a !== nothing, allstars)
        before = if options.batching && !isempty(mut)
            ps, pl = score_batch_minibatch(dataset, Node{T}[allstars[k].tree for k in mut], options)
            num_evals += length(mut) * (options.batch_size / dataset.n)
            Dict(k => (ps[i], pl[i]) for (i, k) in enumerate(mut))
        else
            Dict(k => (allstars[k].score, allstars[k].loss) for k in mut)
        end
        for k in mut
            allstar = allstars[k]
            steps[k] = Step{T}(false, propose(dataset, allstar, before[k], temperature, curmaxsize, options),
                               (allstar,), nothing)
        end
        # every :optimize proposal of this step, all islands, in one optimiser call
        to_opt = PopMember{T}[s.prop.member for s in steps if !s.crossover && s.prop.optimize]
        opt_evals = minibatch ? optimize_sampled(dataset, to_opt, options) :
                    optimize_constants_batched(dataset, to_opt, options)
        num_evals += sum(opt_evals; init=0.0)
        # ONE launch: mutated trees and both crossover children of every island
        trees = Node{T}[]
        for s in steps
            if s.crossover
                s.children === nothing || append!(trees, s.children)
            elseif s.prop.member === nothing
                push!(trees, s.prop.tree)
            end
        end
        scores, losses = options.batching ? score_batch_minibatch(dataset, trees, options) :
                         score_batch(dataset, trees, options)
        j = 0
        for (k, pop) in enumerate(pops)
            s = steps[k]
            if !s.crossover
                p = s.prop
                num_evals += p.num_evals
                baby, accepted = if p.member === nothing
                    j += 1
                    num_evals += options.batching ? options.batch_size / dataset.n : 1.0
                    accept(p, scores[j], losses[j], temperature, stats[k], options)
                else
                    (p.member, p.accepted)
                end
                (!accepted && options.skip_mutation_failures) && continue
                pop.members[argmin([m.birth for m in pop.members])] = baby
            else
                a1, a2 = s.parents
                if s.children === nothing
                    options.skip_mutation_failures && continue
                    b1, b2 = a1, a2  # a failed crossover returns member1, member2 (src/Mutate.jl:309)
                else
                    b1 = PopMember(s.children[1], scores[j + 1], losses[j + 1]; parent=a1.ref,
                                   deterministic=options.deterministic)
                    b2 = PopMember(s.children[2], scores[j + 2], losses[j + 2]; parent=a2.ref,
                                   deterministic=options.deterministic)
                    j += 2
                    # src/Mutate.jl:314-322: 2·batch_size/n with batching, batch_size/n without
                    num_evals += options.batching ? 2 * (options.batch_size / dataset.n) :
                                 options.batch_size / dataset.n
                end
                pop.members[argmin([m.birth for m in pop.members])] = b1
                pop.members[argmin([m.birth for m in pop.members])] = b2
            end
        end
    end
    return pops, num_evals
end

"""
    s_r_cycle_lockstep(dataset, pops, ncycles, curmaxsize, stats, options) -> (pops, best_seen, num_evals)

s_r_cycle (src/SingleIteration.jl:17-61) for every island at once: the
temperature schedule, reg_evol_cycle_lockstep (or reg_evol_cycle_batched when
options.fast_cycle), and each island's best-seen hall of fame. The head node
calls it once per round with every island it would have spawned, instead of
one @sr_spawner job per island (INTEGRATION.md §4).

With options.recorder the lockstep loops would write no genealogy (the
mutation / death events of src/RegularizedEvolution.jl:103-132), so every
island runs the reference's own s_r_cycle instead, recording into records[k].
"""
function s_r_cycle_lockstep(dataset::Dataset{T}, pops::AbstractVector{<:Population}, ncycles::Int,
                            curmaxsize::Int, stats::AbstractVector{RunningSearchStatistics},
                            options::Options; records=nothing, device::Int=0,
                            minibatch::Bool=false) where {T}
    if options.recorder
        best_seen = Vector{HallOfFame{T}}(undef, length(pops))
        num_evals = 0.0
        for k in eachindex(pops)
            rec = records === nothing ? RecordType() : records[k]
            pops[k], best_seen[k], ev = s_r_cycle(dataset, pops[k], ncycles, curmaxsize, stats[k];
                                                  options=options, record=rec)
            num_evals += ev
        end
        return pops, best_seen, num_evals
    end
    max_temp = T(1.0)
    min_temp = options.annealing ? T(0.0) : max_temp
    best_seen = [HallOfFame(options, T) for _ in pops]
    num_evals = 0.0
    for temperature in LinRange(max_temp, min_temp, ncycles)
        _, ev = options.fast_cycle ?
                reg_evol_cycle_batched(dataset, pops, temperature, curmaxsize, stats, options; device=device,
                                       minibatch=minibatch) :
                reg_evol_cycle_lockstep(dataset, pops, temperature, curmaxsize, stats, options; device=device,
                                        minibatch=minibatch)
        num_evals += ev
        for (k, pop) in enumerate(pops), member in pop.members
            size = compute_complexity(member.tree, options)
            if 0 < size <= options.maxsize &&
               (!best_seen[k].exists[size] || member.score < best_seen[k].members[size].score)
                best_seen[k].exists[size] = true
                best_seen[k].members[size] = copy_pop_member(member)
            end
        end
    end
    return pops, best_seen, num_evals
end

"""
    s_r_cycle_devices(dataset, pops, ncycles, curmaxsize, stats, options, group) -> (pops, best_seen, num_evals)

s_r_cycle_lockstep spread over the devices of `group` (an SRHip.DeviceGroup):
island k (1-based) belongs to member d = (k - 1) % ndev, the islands of one
member run their lockstep cycles together on that member's device
(`device = group.devices[d + 1]`), and the members run at once, one task per
member (src/SearchUtils.jl:33-45 spawns one per island; here one per device,
each scoring its islands' candidates in one launch). Every task scores through
the single-device calls on its device's full copy of the dataset, so an island
computes what it computes alone. Migration, the hall of fame and the
statistics stay on the host with the caller, between rounds, as in the
reference (src/SymbolicRegression.jl:717-778). The results come back in
island order.
"""
function s_r_cycle_devices(dataset::Dataset{T}, pops::AbstractVector{<:Population}, ncycles::Int,
                           curmaxsize::Int, stats::AbstractVector{RunningSearchStatistics},
                           options::Options, group::SRHip.DeviceGroup; records=nothing) where {T}
    ndev = SRHip.ndevices(group)
    parts = [collect(d:ndev:length(pops)) for d in 1:ndev]   # islands of member d - 1
    tasks = map(1:ndev) do d
        ks = parts[d]
        Threads.@spawn begin
            isempty(ks) && return (ks, nothing, nothing, 0.0)
            p, b, ev = s_r_cycle_lockstep(dataset, pops[ks], ncycles, curmaxsize, stats[ks], options;
                                          records=(records === nothing ? nothing : records[ks]),
                                          device=Int(group.devices[d]))
            (ks, p, b, ev)
        end
    end
    best_seen = Vector{HallOfFame{T}}(undef, length(pops))
    num_evals = 0.0
    for t in tasks
        ks, p, b, ev = fetch(t)
        for (i, k) in enumerate(ks)
            pops[k] = p[i]
            best_seen[k] = b[i]
        end
        num_evals += ev
    end
    return pops, best_seen, num_evals
end

end # module
