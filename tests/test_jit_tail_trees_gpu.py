"""The tail split along trees of the loss tree code (csrc/tail_map.h, api.cpp
tail_trees, the hand-written loops of csrc/jit_template.hip): each tree group
of the last row groups is run by S workgroups, sub-workgroup `sub` walking the
list positions sub, sub + S, ... Every partial is still stored per (row group,
position) and summed by the finalize in its fixed order, so no output bit may
change.

Every variant (tests/jit_tail_trees_cases.py: the batch, its hand-made trees
and the settings) runs in a child process, one program evaluated under
SRHIP_JIT_TAIL_RG ∈ {1, 2, 4} × SRHIP_JIT_TAIL_TREES ∈ {2, 4, 8} (the knobs
are read per launch). Loss sums, Σ w and did_succeed of every setting are
byte-identical to S = 1 of the same process and to a child run with
SRHIP_JIT_TAIL=0 (both tail splits off). Variants: the prefetching loop,
weighted rows, the memory-constant loop (after set_constants), the plain loop
(SRHIP_JIT_PREFETCH=0), SRHIP_JIT_ROTATE 0 / 1 / 2, blocks in launch order
(SRHIP_RG_XCD=0), a program of a second context on the dataset, and the
Periodic loss, under which trees are handed back to the interpreter.

Geometry. The children run with SRHIP_TARGET_WG=92: four row groups, 22 tree
groups of 14 list positions, 308 slots for 300 trees. 14 is no multiple of 4
or 8, so the sub-workgroups' walks differ in length and end raggedly; a
4-wave sub-workgroup of S = 2 walks 7 positions, so its waves claim again
after a tree call has returned (the counter's step S must survive the call);
and the last positions of 8 groups have no slot, which a split walk passes
over. One more case runs the default geometry, 75 groups of 4: S = 8 is
larger than a group's tree count and sub-workgroups 4 .. 7 own nothing. The
geometry of every launch is read back (Context.last_loss_launch) and asserted,
so no case passes unsplit.

Each variant first asserts what it is there for (the kernel that ran, trees
failing, a tile redone, a tree handed back). With the knobs unset the launch
and the tree code's counters are those of S = 1."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import jit_tail_trees_cases as cases

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
VARIANTS = ["l2", "weighted", "set_constants", "plain", "rotate", "plain_order", "two_contexts", "periodic_bail"]
KERNEL = {"l2": "sr_jit_eval_dlp", "weighted": "sr_jit_eval_dlpw", "set_constants": "sr_jit_eval_dlm",
          "plain": "sr_jit_eval_dl", "rotate": "sr_jit_eval_dlp", "plain_order": "sr_jit_eval_dlp",
          "two_contexts": "sr_jit_eval_dlp"}
KNOBS = ("SRHIP_JIT_TAIL", "SRHIP_JIT_TAIL_TREES", "SRHIP_JIT_TAIL_RG", "SRHIP_JIT_TAIL_ROUNDS", "SRHIP_JIT_ROTATE",
         "SRHIP_JIT_PREFETCH", "SRHIP_JIT_DYNLOOP", "SRHIP_JIT_MEMC", "SRHIP_RG_XCD", "SRHIP_TARGET_WG",
         "SRHIP_MIN_PER_GROUP")
RAGGED = {"SRHIP_TARGET_WG": "92"}  # 22 tree groups of 14


def child(names, **kv):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(kv)
    run = subprocess.run([sys.executable, str(HERE / "jit_tail_trees_cases.py"), *names], env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def reference(gpu_ctx):
    """Every variant once, in one child process, with SRHIP_JIT_TAIL=0."""
    return child(VARIANTS, SRHIP_JIT_TAIL="0", **RAGGED)


def ok_of(r):
    return bytes.fromhex(r["ok"])


def check(name, got, ref, ntg_tpb):
    tags = [t for t, _ in cases.settings((0, 1, 2) if name == "rotate" else (None,))]
    assert list(got) == tags and list(ref) == tags
    base = got[tags[1]]  # S1 (of the first rotate mode)
    assert tags[1].startswith("S1")
    ok = ok_of(base)
    print(name, "kernel", base["kernel"], "launches", base["launches"], "tree code", base["tree_code"], "failed",
          len(ok) - sum(ok), "bailed", base["bailed"], "tiles redone", base["redone"], base["geometry"])
    # what the batch is there for
    assert base["tree_code"] >= 0.9 * cases.NTREES
    assert not ok[cases.HAND["every_row"]] and not ok[cases.HAND["late_row"]]
    assert 0.1 * cases.NTREES < len(ok) - sum(ok) < 0.5 * cases.NTREES
    if name == "periodic_bail":
        assert base["bailed"] >= 1
    else:
        assert base["kernel"] == KERNEL[name], base["kernel"]
        assert ok[cases.HAND["redo"]] and ok[cases.HAND["bail"]]
    if name in ("l2", "plain", "rotate", "plain_order", "two_contexts"):
        assert base["redone"] >= 1
    dealt = name != "plain_order"  # the XCD-dealt block order pads the head and the tail to octets of row groups
    for tag in tags:
        g = got[tag]
        # the launch really was split as the setting says (and is not where it says so)
        geo, rgeo = g["geometry"], ref[tag]["geometry"]
        nrg, ntg, tpb = geo["nrg"], geo["ntg"], geo["tpb"]
        assert (nrg, ntg, tpb) == (4,) + ntg_tpb, geo
        unsplit = (8 if dealt else nrg) * ntg
        assert (rgeo["tsub"], rgeo["grid"]) == (1, unsplit), (geo, rgeo)
        if tag.startswith("S") and not tag.startswith("S1"):
            S, n = (int(x[1:]) for x in tag.split("-")[:2])
            assert (geo["tsub"], geo["tbig"]) == (S, nrg - n), (tag, geo)
            head = ((nrg - n + 7) // 8 * 8 if dealt else nrg - n) * ntg
            assert geo["grid"] == head + 8 * ntg * S, (tag, geo)  # the tail: one octet of row groups
        else:
            assert (geo["tsub"], geo["grid"]) == (1, unsplit), (tag, geo)
        for other, what in ((base, "S = 1"), (ref[tag], "SRHIP_JIT_TAIL=0")):
            assert g["ok"] == other["ok"], f"{tag}: did_succeed differs from {what}"
            assert g["sums"] == other["sums"], f"{tag}: loss sums differ from {what}"
            assert g["wsum"] == other["wsum"]
        assert g["kernel"] == base["kernel"] and g["tree_code"] == base["tree_code"]
        # (trees handed back and tiles redone are not compared: a tree that also fails on some row is
        # skipped by the row groups that start after its flag is set, which depends on the timing)
        assert (g["bailed"] > 0) == (base["bailed"] > 0), tag
        assert g["launches"] == base["launches"], tag  # a split launch is still one launch
        assert g["info"] == base["info"], tag


@pytest.mark.parametrize("name", VARIANTS)
def test_tree_tail_changes_no_bit(gpu_ctx, reference, name):
    ntg, tpb = 22, 14
    # the walks of a split group differ in length, and the list is ragged: some last positions have no slot
    assert tpb % 4 != 0 and tpb % 8 != 0 and ntg * tpb > cases.NTREES
    check(name, child([name], **RAGGED)[name], reference[name], (ntg, tpb))


def test_more_workgroups_than_trees_in_a_group(gpu_ctx):
    """The default geometry: 75 groups of 4 trees, so S = 8 exceeds a group's tree count."""
    ntg, tpb = 75, 4
    assert max(cases.TAIL_TREES) > tpb
    check("l2", child(["l2"])["l2"], child(["l2"], SRHIP_JIT_TAIL="0")["l2"], (ntg, tpb))


@pytest.mark.parametrize("name", ["l2", "set_constants"])
def test_knobs_off_is_the_unsplit_launch(gpu_ctx, reference, name):
    """With no knob set a grid this small is never split (it fills no round of
    the resident workgroups): the launch, its count and the tree code's
    counters are those of S = 1 and of SRHIP_JIT_TAIL=0."""
    got = child([name], **RAGGED)[name]
    for other in (got["S1"], reference[name]["default"], reference[name]["S1"]):
        for k in ("launches", "info", "tree_code", "kernel", "sums", "ok", "geometry"):
            assert got["default"][k] == other[k], k
