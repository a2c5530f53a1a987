"""The slot registry (csrc/slots.h) is host logic: assignment, least-recently-used
replacement, "skip the slots of the program being assigned", the column limit.
A stand-alone C++ program (tests/slot_registry_test.cpp, its own main) checks it
on the CPU, built with the address and undefined-behaviour sanitizers where the
compiler has them. No GPU, nothing loaded into Python."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "symbolicregression.jl_amd" / "csrc"
SRC = Path(__file__).resolve().parent / "slot_registry_test.cpp"


def _compiler():
    for name in ("g++", "c++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def test_slot_registry_program(tmp_path):
    cxx = _compiler()
    assert cxx, "no C++ compiler on PATH"
    exe = tmp_path / "slot_registry_test"
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), str(SRC), "-o", str(exe)]
    built = subprocess.run(base[:4] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[4:],
                           capture_output=True, text=True)
    if built.returncode != 0:  # a compiler without the sanitizer runtimes: the plain build still checks the logic
        print(built.stderr)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert "slot registry ok" in run.stdout
