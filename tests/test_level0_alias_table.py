"""The level-0 alias table of the free-gas pipeline (fg_pipeline.h fg_setup_group, FgBatch::t_alias),
checked on the CPU: tests/aliascheck/aliascheck.cpp calls the product's fg_setup_group and compares the
table with a brute-force look at the roots it laid out -- an alias and its source are live tasks of one
job with the same double for E_out, no source is an alias, and an end point shared by two segments is
aliased exactly once.  The cases are those of tests/test_gpu_level0_alias.py."""
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_level0_alias import ALIASES, CASES, KT

SRC = ROOT / "tests" / "aliascheck" / "aliascheck.cpp"
# the GPU test's cases (the same energies, to the bit) and a group of zero width between two live ones
TABLE_CASES = dict(CASES)
TABLE_CASES["degenerate_edges"] = (0.999167, 6, np.array([0.0, 1e-8, 1e-8, 6.25e-7, 20.0]),
                                   np.geomspace(1e-10, 1e-5, 64), True)
TABLE_ALIASES = dict(ALIASES, degenerate_edges=384)


@pytest.fixture(scope="module")
def aliascheck(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/aliascheck")
    exe = tmp_path_factory.mktemp("aliascheck") / "aliascheck"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-DNDPP_FAST=1", "-ffp-contract=fast",
                    "-o", str(exe), str(SRC)], check=True)
    return exe


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_alias_table_names_each_shared_end_point_once(aliascheck, name):
    A, _, bins, ein, shared = TABLE_CASES[name]
    res = subprocess.run([str(aliascheck), repr(float(A)), repr(KT), str(len(bins) - 1), *[repr(float(b)) for b in bins],
                          *[repr(float(e)) for e in ein]], capture_output=True, text=True)
    print(name, res.stdout.strip(), res.stderr.strip())
    assert res.returncode == 0, res.stdout + res.stderr
    words = res.stdout.split()
    n_shared, n_alias = int(words[3]), int(words[5])
    assert n_alias == n_shared and (n_shared > 0) == shared
    assert n_alias == TABLE_ALIASES[name]
