"""The set-up of the free-gas inner walk through item records (fg_pipeline.h fg_item_build, mu_init,
mu_init_split, split_segment), checked on the CPU by tests/itemcheck/itemcheck.cpp against a
restatement of the set-up it replaced: the closed form for an item's segment against the loops for
all 16 x 16 (peak node, rank) pairs, each peak node's ranks a permutation of the 16 segments, and
the lane state built from a record equal, field by field and bit for bit, to the one gathered from
the node, job and task arrays -- for dead nodes, level-0 aliases and Gauss-taken rows too."""
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "itemcheck" / "itemcheck.cpp"
ARITHMETICS = {"product": ["-DNDPP_FAST=1", "-ffp-contract=fast"], "reference": ["-DNDPP_FAST=0", "-ffp-contract=off"]}


@pytest.mark.parametrize("arith", sorted(ARITHMETICS))
def test_item_records_and_segment_order_match_the_previous_set_up(tmp_path, arith):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/itemcheck")
    exe = tmp_path / "itemcheck"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", *ARITHMETICS[arith], "-o", str(exe), str(SRC)],
                   check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(arith, res.stdout.strip(), res.stderr.strip())
    assert res.returncode == 0, res.stdout + res.stderr
    words = res.stdout.split()
    assert words[:2] == ["segments", "ok;"]
    # 2 orders x 100 tasks x 16 items, and the case holds each kind of task
    assert int(words[3]) == 2 * 100 * 16 and int(words[5]) > 0 and int(words[7]) > 0 and int(words[9]) > 0
