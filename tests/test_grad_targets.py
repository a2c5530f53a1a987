"""Gradients and constant optimisation with a target per tree, the parts that need no device:
the three new calls in the header, srhip._lib and the library, the Julia binding's new ccalls
against the header (the parsing of tests/test_julia_binding.py), the argument rules that are
answered before any device work, and the regroup fallback's slices of the start noise."""
import ctypes as C
import re

import numpy as np
import pytest

import srhip
from srhip import _lib
from test_julia_binding import BATCHED, HDR, JL, _c_kind, _jl_kind, header_prototypes, julia_ccalls

NEW_CALLS = ("srhip_eval_loss_grad_targets", "srhip_eval_loss_grad_rowsets_targets",
             "srhip_optimize_constants_targets")


def data(T=np.float32, n=40, k=3):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4, n)).astype(T)
    Y = rng.standard_normal((k, n)).astype(T)
    W = np.abs(rng.standard_normal((k, n))).astype(T)
    return X, Y, W


def test_header_python_signatures_and_symbols():
    hdr = HDR.read_text()
    assert re.search(r"#define SRHIP_ABI_VERSION\s+1\b", hdr)
    protos = header_prototypes()
    want = {"srhip_eval_loss_grad_targets": 9, "srhip_eval_loss_grad_rowsets_targets": 11,
            "srhip_optimize_constants_targets": 11}
    for name, nargs in want.items():
        assert name in protos, name
        assert protos[name][0] == "int32_t" and len(protos[name][1]) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(_lib.lib(), name), name
    # the parameter kinds of the optimiser: ctx, ds, trees, opts, target, row_idx, batch_size, 4 outputs
    kinds = [_c_kind(p) for p in protos["srhip_optimize_constants_targets"][1]]
    assert kinds == ["ptr"] * 6 + ["i64"] + ["ptr"] * 4
    kinds = [_c_kind(p) for p in protos["srhip_eval_loss_grad_rowsets_targets"][1]]
    assert kinds == ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"]
    assert _lib.lib().srhip_version() == 1


def test_header_keeps_its_wording_and_says_what_is_left_out():
    hdr = HDR.read_text()
    assert "Not in this version: fused gradients" in hdr and "multi-target group datasets" in hdr
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    block = flat[flat.index("constant gradients with a target per tree"):]
    block = block[:block.index("srhip_constopt_profile(")]
    for phrase in ("expression losses", "multi-target group datasets", "targets in srhip_optimize_constants_cb",
                   "staging only the columns"):
        assert phrase in block, phrase


def test_every_new_ccall_matches_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, argtypes, args in julia_ccalls():
        if name not in NEW_CALLS:
            continue
        seen.add(name)
        cret, cparams = protos[name]
        assert ret == "Int32" and cret == "int32_t", name
        assert len(argtypes) == len(cparams) == len(args), name
        for jt, cp in zip(argtypes, cparams):
            assert _jl_kind(jt) == _c_kind(cp), f"{name}: Julia {jt} vs C {cp}"
    assert seen == set(NEW_CALLS), set(NEW_CALLS) ^ seen
    src = JL.read_text()
    for fn in ("eval_loss_grad_targets", "optimize_constants_targets!"):
        assert re.search(rf"^function {re.escape(fn)}\(", src, re.M), fn
    body = re.search(r"function optimize_constants_targets!\(.*?\nend", src, re.S).group(0)
    assert "MultiCopy(datasets, device)" in body and "srhip_optimize_constants_targets" in body
    assert "Int32.(js .- 1)" in body and "row_idx .- 1" in body


def test_julia_caller_has_the_fused_call_and_the_per_output_fallback():
    code = "\n".join(ln.split("#")[0] for ln in BATCHED.read_text().splitlines())
    multi = re.search(r"function optimize_constants_batched_multi\(.*?\nend", code, re.S).group(0)
    assert "SRHip.optimize_constants_targets!(" in multi
    assert "e isa SRHip.Unsupported || rethrow()" in multi
    assert "optimize_constants_batched(datasets[j]" in multi
    assert "datasets[j].baseline_loss" in multi
    assert "d.X === datasets[1].X" in multi
    # the default switch is the one the Python side uses
    jl = int(re.search(r"const FUSED_CONSTOPT_MAX_MEMBERS = (\d+)", code).group(1))
    assert jl == srhip.interface.FUSED_GRAD_TARGETS_MAX_TREES


def test_null_dataset_and_options_are_invalid_without_a_device():
    lib = _lib.lib()
    out = np.full(4, 7.5)
    p = out.ctypes.data_as(C.c_void_p)
    tg = np.zeros(1, dtype=np.int32)
    rc = lib.srhip_optimize_constants_targets(None, None, None, None, tg.ctypes.data_as(C.c_void_p), None, 0, p, p,
                                              None, p)
    assert rc == _lib.ERR_INVALID and b"dataset" in lib.srhip_last_error()
    assert np.all(out == 7.5)
    # (a dataset needs a device; the options are looked at right after it, as in srhip_optimize_constants_batch)
    for fn in (lib.srhip_eval_loss_grad_targets, ):
        assert fn(None, None, 0, None, None, p, p, p, None) == _lib.ERR_INVALID
    assert lib.srhip_eval_loss_grad_rowsets_targets(None, None, 0, None, None, None, 4, p, p, p,
                                                    None) == _lib.ERR_INVALID
    assert np.all(out == 7.5)


def test_python_argument_rules_need_no_device():
    X, Y, W = data()
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["cos"])
    trees = srhip.random_population(4, o, 4, np.float32, seed=1)
    mds = srhip.MultiDataset(X, Y)
    rng = np.random.default_rng(0)
    for call in (lambda **kw: srhip.eval_loss_grad_batch(trees, mds, o, **kw),
                 lambda **kw: srhip.optimize_constants_batch(mds, trees, o, rng=rng, **kw)):
        with pytest.raises(ValueError, match="targets="):
            call()
        with pytest.raises(ValueError):
            call(targets=[0, 1, 2])
        with pytest.raises(ValueError):
            call(targets=[0, 1, 2, 3])
        with pytest.raises(ValueError):
            call(targets=[0, 1, 2, -1])
        with pytest.raises(ValueError, match="row_idx"):
            call(targets=[0, 1, 2, 0], row_idx=np.zeros((3, 5), dtype=np.int64))
        with pytest.raises(ValueError, match="row_idx"):
            call(targets=[0, 1, 2, 0], row_idx=np.zeros(4, dtype=np.int64))
    plain = srhip.Dataset(X, Y[0])
    with pytest.raises(ValueError, match="MultiDataset"):
        srhip.eval_loss_grad_batch(trees, plain, o, targets=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="MultiDataset"):
        srhip.optimize_constants_batch(plain, trees, o, rng=rng, targets=[0, 0, 0, 0])


class StubEvaluator:
    """Quadratic bowls: candidate k's loss is Σ (c - 1)², so every run moves; records what it is given."""

    def __init__(self, cands, log, target, members):
        self.co = np.concatenate([[0], np.cumsum([len(srhip.get_constants(c)) for c in cands])])
        self.entry = dict(target=target, members=None if members is None else np.asarray(members).copy(), x0=None)
        log.append(self.entry)

    def loss_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        if self.entry["x0"] is None:  # the constants of the evaluator's first call, per candidate
            self.entry["x0"] = [x[a:b].copy() for a, b in zip(self.co[:-1], self.co[1:])]
        f = np.array([np.sum((x[a:b] - 1.0) ** 2) for a, b in zip(self.co[:-1], self.co[1:])])
        return f, 2.0 * (x - 1.0)

    def loss_only(self, x):
        return self.loss_grad(x)[0]


def test_regroup_fallback_hands_each_group_its_slice_of_the_noise():
    """With evaluator_factory the MultiDataset call regroups by target. The first evaluator of a
    group is first called with the group's starts: x0 and x0·(1 + noise/2) per tree, so they show
    which draws each tree was given: those of its own position in the caller's noise array."""
    T = np.float64
    X, Y, W = data(T)
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["cos"])
    B = o.make_binary
    mk = lambda a, b: B("+", B("*", srhip.Node(val=a), srhip.Node("x1")), srhip.Node(val=b))
    trees = [mk(2.0 + t, -1.0 - t) for t in range(5)] + [B("*", srhip.Node(val=0.5), srhip.Node("x2"))]
    tg = np.array([2, 0, 2, 1, 0, 2], dtype=np.int32)
    mds = srhip.MultiDataset(X, Y)
    flat = srhip.flatten(trees, o, dtype=T)
    nre = o.optimizer_nrestarts
    noise = srhip.constant_optimization.start_noise(flat, nre, np.random.default_rng(3))
    noff = nre * np.asarray(flat.const_off)
    log = []
    factory = lambda cands, members=None, target=None: StubEvaluator(cands, log, target, members)
    mine = [t.copy() for t in trees]
    res = srhip.optimize_constants_batch(mds, mine, o, noise=noise, evaluator_factory=factory, targets=tg)
    assert res.losses.shape == (6,) and res.converged.any()
    firsts = {}
    for entry in log:
        firsts.setdefault(entry["target"], entry)  # the group's first evaluator: every start of every tree
    assert set(firsts) == {0, 1, 2}
    for k, entry in firsts.items():
        idx = np.flatnonzero(tg == k)
        assert len(entry["x0"]) == len(idx) * (1 + nre)
        assert np.array_equal(np.unique(entry["members"]), np.arange(len(idx)))  # positions within the group
        for m, x in zip(entry["members"], entry["x0"]):
            t = idx[m]
            c0 = np.asarray(srhip.get_constants(trees[t]), dtype=np.float64)
            draws = noise[noff[t]:noff[t + 1]].reshape(nre, len(c0))
            starts = [c0] + [c0 * (1.0 + 0.5 * d) for d in draws]
            assert any(np.allclose(x, s, rtol=1e-14, atol=0) for s in starts), (k, t, x, starts)
        # every restart of every tree of the group is there: its own draws, nobody else's
        for j, t in enumerate(idx):
            c0 = np.asarray(srhip.get_constants(trees[t]), dtype=np.float64)
            draws = noise[noff[t]:noff[t + 1]].reshape(nre, len(c0))
            mine_x = [x for m, x in zip(entry["members"], entry["x0"]) if m == j]
            for d in draws:
                assert any(np.allclose(x, c0 * (1.0 + 0.5 * d), rtol=1e-14, atol=0) for x in mine_x), (k, t)
    # converged trees were updated in place, through the sub-lists
    moved = [not np.array_equal(srhip.get_constants(a), srhip.get_constants(b)) for a, b in zip(mine, trees)]
    assert any(moved) and np.array_equal(np.asarray(moved), res.converged & np.asarray(moved))
    # the wrong noise length is refused before any work
    with pytest.raises(ValueError, match="start noise"):
        srhip.optimize_constants_batch(mds, [t.copy() for t in trees], o, noise=noise[:-1], evaluator_factory=factory,
                                       targets=tg)
