"""The shortened packed divisions (csrc/gen_jit.py manual_div, manual_div_lc and
their FAST forms) on the CPU: what the generator wrote, where the routines
lie, and the C model of the sequence (tools/check_div_short.c). What the
bodies compute on the hardware is tests/test_div_short_gpu.py's."""
import json
import re
import struct
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GEN = ROOT / "symbolicregression.jl_amd" / "csrc" / "gen"
GOLDEN = Path(__file__).resolve().parent / "golden"


def routine_bodies():
    """{sr_rt_<region>_<name>: instructions up to and including the routine's return}."""
    inc = (GEN / "jit_routines_r4.inc").read_text()
    lines = re.findall(r'^\s*"([^"\n]*)\\n"', inc, re.M)
    bodies, cur = {}, None
    for ln in lines:
        m = re.match(r"(sr_rt_(?:fast|prec)_\w+):$", ln)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur and not ln.startswith((".globl", ".L", ".p2align", ".fill")):
            bodies[cur].append(ln)
    return bodies


@pytest.mark.parametrize("region", ["fast", "prec"])
@pytest.mark.parametrize("name", ["b_div", "b_div_lc"])
def test_division_bodies_hold_one_residual_step(region, name):
    """4 v_rcp_f32 and 10 packed multiply / fma instructions: two for each of
    e = 1 - b*r, y = r + e*r, q = a*y, s = a - b*q, q + s*y. The last two write
    the quotient to A, and nothing reads a reciprocal in the slot after its
    v_rcp_f32 (a non-trans read of a trans result needs one in between)."""
    body = routine_bodies()[f"sr_rt_{region}_{name}"]
    ret = next(k for k, ln in enumerate(body) if ln.startswith("s_setpc_b64"))
    main = body[:ret]  # the packed path; the branch to the compiled routine leaves before
    assert sum(ln.startswith("v_rcp_f32") for ln in main) == 4
    pk = [ln for ln in main if ln.startswith(("v_pk_mul_f32", "v_pk_fma_f32"))]
    assert len(pk) == 10, pk
    assert sum(ln.startswith("v_pk_mul_f32") for ln in pk) == 2
    assert [ln.split()[1] for ln in main[-2:]] == ["v[32:33],", "v[34:35],"]
    assert not any(ln.startswith("v_pk_add_f32") for ln in main)
    for k, ln in enumerate(main):
        if ln.startswith("v_rcp_f32"):
            dst = int(re.match(r"v_rcp_f32_e32 v(\d+),", ln).group(1))
            nxt = main[k + 1]
            srcs = nxt.split(",", 1)[1]
            regs = set()
            for lo, hi in re.findall(r"v\[(\d+):(\d+)\]", srcs):
                regs |= set(range(int(lo), int(hi) + 1))
            regs |= {int(r) for r in re.findall(r"\bv(\d+)\b", srcs)}
            assert dst not in regs, (ln, nxt)


def elf_symbols(path):
    """{name: value} of an ELF64 little-endian file's symbol table."""
    d = Path(path).read_bytes()
    assert d[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + k * shentsize) for k in range(shnum)]
    syms = {}
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        for off in range(s[4], s[4] + s[5], 24):
            name, _, _, _, value, _ = struct.unpack_from("<IBBHQQ", d, off)
            end = d.index(b"\0", stroff + name)
            syms[d[stroff + name:end].decode()] = value
    return syms


def routine_offsets(hsaco):
    """Entry offset of every routine from the start of its region (jit.cpp's
    rt_va[rid] - fast0, which generated tree code holds)."""
    syms = elf_symbols(hsaco)
    out = {}
    for region in ("fast", "prec"):
        base = syms[f"sr_rt_{region}"]
        out[region] = {n[len(f"sr_rt_{region}_"):]: v - base for n, v in syms.items() if n.startswith(f"sr_rt_{region}_")}
    return out


@pytest.mark.parametrize("tmpl", ["jit_tmpl_s.hsaco", "jit_tmpl_l.hsaco"])
def test_routine_entry_offsets_are_those_before_the_change(tmpl):
    """Generated tree code holds every call's offset from the region start, and
    tests pin digests of that code: the division routines keep their slots
    (gen_jit.py SLOT_MIN), so no routine moved when their bodies shrank."""
    want = json.loads((GOLDEN / "div_short_routine_offsets.json").read_text())
    got = routine_offsets(GEN / tmpl)
    assert got["fast"] == got["prec"]
    assert len(got["fast"]) > 50
    assert got["fast"] == want["offsets"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("div_short") / "check_div_short"
    r = subprocess.run(["cc", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe),
                        str(ROOT / "tools" / "check_div_short.c"), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_model_reduced_run(model):
    """Every divisor significand with the reciprocal RN(1/b) and its two
    neighbours; the first divisors whose refined reciprocal is not RN(1/b)
    against all numerators; 2 million random pairs. With r = RN(1/b) the
    sequence is the IEEE quotient everywhere (exit status, and the line)."""
    r = subprocess.run([str(model), "A", "sig", "2000000", "4"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^r = RN\(1/b\) +refined y != RN\(1/b\) at (\d+) divisors; .*: (\d+) mismatches; random pairs: (\d+) mismatches",
                  r.stdout, re.M)
    assert m and [int(x) for x in m.groups()] == [0, 0, 0], r.stdout
    # the neighbours are what the device sweep is for: the model must see them fail somewhere
    assert re.search(r"^MISMATCH r = RN\(1/b\) - 1 ulp a=0x1p\+0 b=0x1\.fffffep\+0", r.stdout, re.M), r.stdout


def test_model_exponent_pairs(model):
    """The exponent-pair model at the FAST bound 2^-50 and the PRECISE bounds:
    no kept pair gives a finite value other than the IEEE quotient."""
    r = subprocess.run([str(model), "A", "range", "-50", "200000"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    kept = [int(x) for x in re.findall(r"kept (\d+), finite results that differ from IEEE 0,", r.stdout)]
    assert len(kept) == 2 and min(kept) > 1_000_000, r.stdout
