"""The library's environment switches are declared in one table (csrc/zk_switches.h), read through one accessor, and
documented from that table.  Text checks on the sources; no GPU, no build."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "motif-learn_amd", "csrc")
READ = {"call": "per call", "plan": "at plan creation", "comm": "at communicator creation"}
# run-time switches and compile-time experiment variants that were removed with the branches only they reached
REMOVED = ["ZK_STRIP_V1", "ZK_TILE_NBUF", "ZK_ROW_GRID_MARGIN", "ZK_ESTEP_WAVES", "ZK_BATCH_PAIR", "ZK_AUTO_DIRECT_NMAX",
           "ZK_ABLATE", "ZK_DMA_AUX", "ZK_STORE_NT", "ZK_BATCH_PIPE", "ZK_ROTATE", "ZK_STRIP2", "ZK_STRIP3", "ZK_EXP_HALF_TABLE"]


def _text(path):
    with open(path, "rb") as f:
        raw = f.read()
    return None if b"\0" in raw else raw.decode("utf-8", errors="replace")


def _source_files(top):
    for base, dirs, files in os.walk(top):
        dirs[:] = [d for d in dirs if d not in ("build", "__pycache__")]
        for name in files:
            path = os.path.join(base, name)
            text = _text(path)
            if text is not None:  # (binaries -- a built library, golden vectors -- are not source)
                yield path, text


def _declared():
    """{name: (kind, default, read)} of the X-macro table."""
    text = _text(os.path.join(CSRC, "zk_switches.h"))
    rows = re.findall(r'^\s*X\((ZK_\w+), (\w+), (\w+), (\w+), "[^"]+"\)', text, flags=re.M)
    assert rows, "no switch table in zk_switches.h"
    assert len({r[0] for r in rows}) == len(rows), "a switch is declared twice"
    return {name: (kind, dflt, READ[read]) for name, kind, dflt, read in rows}


def _documented():
    """{name: (kind, default, read)} of the rows of INTEGRATION.md's table of library switches."""
    text = _text(os.path.join(ROOT, "INTEGRATION.md"))
    rows = re.findall(r"^\| `(ZK_\w+)` \| (\w+) \| (\w+) \| ([a-z ]+) \| .+ \|$", text, flags=re.M)
    assert len({r[0] for r in rows}) == len(rows), "a switch has two rows"
    return {name: (kind, dflt, read) for name, kind, dflt, read in rows}


def test_the_library_reads_its_environment_in_one_place():
    users = [os.path.basename(p) for p, text in _source_files(CSRC) if "getenv" in text]
    assert users == ["zk_switches.h"], users


def test_every_switch_is_documented_and_every_documented_switch_exists():
    declared, documented = _declared(), _documented()
    assert sorted(declared) == sorted(documented)
    assert declared == documented  # kind, default and when it is read, row by row


def test_every_switch_the_sources_ask_for_is_declared():
    declared = _declared()
    asked = set()
    for _, text in _source_files(CSRC):
        asked |= set(re.findall(r"zk_switch_(?:on|int|str)\((ZK_\w+)", text))
    assert asked == set(declared), sorted(asked ^ set(declared))


def test_removed_switches_and_experiment_variants_are_gone():
    me = os.path.abspath(__file__)
    pattern = re.compile(r"\b(?:%s)\b" % "|".join(REMOVED))
    found = []
    for top in ("motif-learn_amd", "include", "tests"):
        for path, text in _source_files(os.path.join(ROOT, top)):
            if os.path.abspath(path) != me:
                found += [f"{os.path.relpath(path, ROOT)}: {m}" for m in sorted(set(pattern.findall(text)))]
    assert not found, found
