"""The block map of the tree-wise tail split (csrc/tail_map.h) is plain integer
code shared by the loss tree-code kernels and the host. A stand-alone C++
program (tests/tail_map_test.cpp, its own main) checks it on the CPU: every
(row group, tree group, sub-workgroup) owned by one block, S = 1 the unsplit
map, a tail row group on one XCD, and the walk the loops make over a group's
list positions. It is built and run twice: plain, and with the address and
undefined-behaviour sanitizers (skipped, with the reason, where the compiler
has no sanitizer runtimes). No GPU, nothing loaded into Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "symbolicregression.jl_amd" / "csrc"
SRC = Path(__file__).resolve().parent / "tail_map_test.cpp"


def _compiler():
    for name in ("g++", "c++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.parametrize("sanitized", [False, True])
def test_tail_map_program(tmp_path, sanitized):
    cxx = _compiler()
    assert cxx, "no C++ compiler on PATH"
    exe = tmp_path / "tail_map_test"
    base = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), str(SRC), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if sanitized:  # can this compiler link the sanitizer runtimes at all? (checked before any work)
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        can = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if can.returncode != 0:
            pytest.skip("the C++ compiler cannot link -fsanitize=address,undefined: " + can.stderr.strip()[-200:])
    built = subprocess.run(base[:4] + san + base[4:] if sanitized else base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tail map ok" in run.stdout
