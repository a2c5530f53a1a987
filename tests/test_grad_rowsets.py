"""Constant optimisation on per-tree row samples, the parts that need no device:
the two new entry points' prototypes and Julia bindings against include/srhip.h,
the minibatch keyword of BatchedCallers.jl, the oracle-driven optimiser with an
evaluator that picks each candidate's sample (evaluator_factory with members=),
and the Python argument checks."""
import re

import numpy as np
import pytest

import oracle
import srhip
from test_constant_optimization import OracleEvaluator, oracle_factory, problem
from test_julia_binding import BATCHED, JL, _c_kind, _jl_kind, header_prototypes, julia_ccalls

NEW = ("srhip_eval_loss_grad_rowsets", "srhip_optimize_constants_rowsets")


def test_prototypes_agree_with_the_header():
    import ctypes as C

    from srhip._lib import SIGNATURES

    protos = header_prototypes()
    for name in NEW:
        assert name in protos and name in SIGNATURES, name
        cret, cparams = protos[name]
        assert cret == "int32_t"
        sig = SIGNATURES[name]
        assert len(sig) == len(cparams), name
        for ct, cp in zip(sig, cparams):
            kind = _c_kind(cp)
            if kind == "ptr":
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, cp)
            else:
                assert ct is {"i32": C.c_int32, "i64": C.c_int64}[kind], (name, cp)
    # the row samples and their length come right before the outputs, as in srhip_eval_loss_rowsets
    assert [p.split()[-1].lstrip("*") for p in protos[NEW[0]][1]][4:6] == ["row_idx", "batch_size"]
    assert [p.split()[-1].lstrip("*") for p in protos[NEW[1]][1]][4:6] == ["row_idx", "batch_size"]


def test_julia_binds_the_new_entry_points():
    protos = header_prototypes()
    calls = {c[0]: c for c in julia_ccalls() if c[0] in NEW}
    assert set(calls) == set(NEW)
    for name, (_, ret, argtypes, args) in calls.items():
        cparams = protos[name][1]
        assert ret == "Int32" and len(argtypes) == len(cparams) == len(args), name
        for jt, cp in zip(argtypes, cparams):
            assert _jl_kind(jt) == _c_kind(cp), f"{name}: Julia {jt} vs C {cp}"
    src = JL.read_text()
    assert re.search(r"^function eval_loss_grad_rowsets\(", src, re.M)
    body = re.search(r"function optimize_constants_batch!\(.*?\nend", src, re.S).group(0)
    assert "row_idx::Union{Nothing,AbstractMatrix{<:Integer}}=nothing" in body
    assert "Matrix{Int64}(row_idx .- 1)" in body  # 1-based to 0-based, as eval_loss_batch_rowsets
    assert "srhip_optimize_constants_rowsets" in body and "srhip_optimize_constants_batch," in body


def test_batched_callers_minibatch_keyword():
    code = "\n".join(ln.split("#")[0] for ln in BATCHED.read_text().splitlines())
    oc = re.search(r"function optimize_constants_batched\(.*?\nend", code, re.S).group(0)
    assert "minibatch::Bool=false" in oc.split("where")[0]
    # row samples only under options.batching, drawn as score_batch_minibatch draws them
    assert "sampled = minibatch && options.batching" in oc
    assert "row_idx = sampled ? rand(1:(dataset.n), options.batch_size, length(trees)) : nothing" in oc
    assert "row_idx=row_idx" in oc
    assert "num_evals .* (options.batch_size / dataset.n)" in oc
    mb = re.search(r"function score_batch_minibatch\(.*?\nend", code, re.S).group(0)
    assert "rand(1:(dataset.n), options.batch_size, length(trees))" in mb
    for fn, passed_on in (("optimize_and_simplify_population_batched", "minibatch=minibatch"),
                          ("s_r_cycle_lockstep", "minibatch=minibatch"),
                          ("reg_evol_cycle_batched", "minibatch ? optimize_sampled(dataset, to_opt, options)"),
                          ("reg_evol_cycle_lockstep", "minibatch ? optimize_sampled(dataset, to_opt, options)")):
        body = re.search(rf"function {fn}\(.*?\nend", code, re.S).group(0)
        assert "minibatch::Bool=false" in body.split("where")[0], fn
        assert passed_on in body, fn
        if "optimize_sampled" in passed_on:  # the :optimize mutations of a cycle
            assert "optimize_constants_batched(ds, ms, o; device=device, minibatch=true)" in body, fn


class SampledOracle(OracleEvaluator):
    """The oracle evaluator with candidate k scored on rows[members[k]]."""

    def __init__(self, cands, options, X, y, rows, members):
        super().__init__(cands, options, X, y)
        self.samples = [np.asarray(rows[int(m)]) for m in members]

    def _one(self, t, c):
        k, a, _ = self.flat.tree(t)
        r = self.samples[t]
        out, g, ok = oracle.eval_grad_consts(k, a, c, self.X[:, r], len(c))
        if not ok:
            return np.inf, np.full(len(c), np.nan)
        res = out - self.y[r]
        return float(np.mean(res * res)), 2.0 * (g @ res) / len(res)


def test_oracle_minibatch_optimisation_recovers_constants():
    o, X, y, trees = problem(n=2000)
    rows = np.random.default_rng(5).integers(0, 2000, (len(trees), 200))
    seen = []

    def factory(cands, members=None):
        assert members is not None and len(members) == len(cands)
        seen.append(np.asarray(members).copy())
        return SampledOracle(cands, o, X, y, rows, members)

    res = srhip.optimize_constants_batch(srhip.Dataset(X, y), trees, o, rng=np.random.default_rng(0),
                                         evaluator_factory=factory, row_idx=rows)
    assert res.converged[0] and res.converged[1]
    assert np.allclose(srhip.get_constants(trees[0]), [2.0, 1.0, -2.0], atol=1e-6)  # noise-free: any sample recovers them
    assert np.allclose(srhip.get_constants(trees[1]), [2.0, 2.0], atol=1e-6)
    assert res.losses[0] < 1e-10 and res.losses[1] < 1e-10
    assert seen and all(m.dtype.kind == "i" and m.min() >= 0 and m.max() < len(trees) for m in seen)
    assert any(len(m) > len(trees) for m in seen)  # the starts of one tree share its index


def test_factory_without_members_is_called_as_before():
    o, X, y, trees = problem()
    _, _, _, trees_ref = problem()
    calls = []

    def plain(cands):  # no members parameter
        calls.append(len(cands))
        return OracleEvaluator(cands, o, X, y)

    ds = srhip.Dataset(X, y)
    res = srhip.optimize_constants_batch(ds, trees, o, rng=np.random.default_rng(0), evaluator_factory=plain)
    ref = srhip.optimize_constants_batch(ds, trees_ref, o, rng=np.random.default_rng(0),
                                         evaluator_factory=oracle_factory(o, X, y))
    assert calls and np.array_equal(res.losses, ref.losses) and np.array_equal(res.num_evals, ref.num_evals)
    assert [srhip.get_constants(t) for t in trees] == [srhip.get_constants(t) for t in trees_ref]


def test_python_argument_checks():
    o, X, y, trees = problem(np.float32)
    ds = srhip.Dataset(X, y)
    good = np.zeros((3, 4), dtype=np.int64)
    for bad in (good[:2], good[0], good.astype(np.float64), np.zeros((4, 3, 2), dtype=np.int64)):
        with pytest.raises(ValueError):
            srhip.eval_loss_grad_batch(trees, ds, o, row_idx=bad)
        with pytest.raises(ValueError):
            srhip.optimize_constants_batch(ds, trees, o, row_idx=bad, evaluator_factory=oracle_factory(o, X, y))
    gds = object.__new__(srhip.GroupDataset)  # the check comes before the dataset is looked at
    with pytest.raises(ValueError, match="GroupDataset"):
        srhip.eval_loss_grad_batch(trees, gds, o, row_idx=good)
    with pytest.raises(ValueError, match="GroupDataset"):
        srhip.optimize_constants_batch(gds, trees, o, row_idx=good)
    assert hasattr(srhip.engine.Program, "eval_loss_grad_rowsets")
