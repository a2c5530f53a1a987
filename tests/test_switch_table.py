"""DESIGN.md "Environment switches" lists exactly the SRHIP_* switches the library reads: every quoted
SRHIP_[A-Z0-9_]+ name in csrc/*.{cpp,h,hip} is a row of the table, every row is such a name, and no
retired switch is named in those sources at all. Plain text matching (SRHIP_LIB, SRHIP_DEVICE and
SRHIP_BENCH_* live in Python and are outside its scope)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "symbolicregression.jl_amd" / "csrc"
SOURCES = sorted(p for ext in ("cpp", "h", "hip") for p in CSRC.glob(f"*.{ext}"))


def section():
    text = (ROOT / "DESIGN.md").read_text()
    m = re.search(r"^## \d+\. Environment switches\n(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert m, "DESIGN.md has no 'Environment switches' section"
    return m.group(1)


def test_table_lists_exactly_the_switches_the_sources_read():
    read = {n for p in SOURCES for n in re.findall(r'"(SRHIP_[A-Z0-9_]+)"', p.read_text())}
    rows = re.findall(r"^\| `(SRHIP_[A-Z0-9_]+)` \|", section(), re.M)
    assert len(SOURCES) > 20 and len(read) > 40
    assert len(rows) == len(set(rows)), "a switch has two rows"
    assert set(rows) == read, f"only in the sources: {sorted(read - set(rows))}; only in the table: {sorted(set(rows) - read)}"
    for row in re.findall(r"^\| `SRHIP_.*$", section(), re.M):  # name, default, accepted, read, file, for
        assert len(re.split(r"(?<!\\)\|", row.strip().strip("|"))) == 6, row


def test_retired_switches_are_gone_from_the_sources():
    tail = section().split("\nRetired", 1)[1]
    retired = set(re.findall(r"`(SRHIP_[A-Z0-9_]+)`", tail))
    assert len(retired) >= 20
    rows = set(re.findall(r"^\| `(SRHIP_[A-Z0-9_]+)` \|", section(), re.M))
    assert not retired & rows
    for p in SOURCES:
        named = set(re.findall(r"SRHIP_[A-Z0-9_]+", p.read_text()))
        assert not named & retired, f"{p.name} names {sorted(named & retired)}"
