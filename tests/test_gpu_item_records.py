"""The inner walk sets its lanes up from item records (fg_pipeline.h fg_item_build, one per inner
integral in task order, written by fg_item_kernel after the level's sort) instead of gathering
through the task order, the node, the job and the task records itself.  Nothing of the arithmetic
moved, so every result must have the bits it had before: the cases below -- every path the set-up
takes: joint and single-row jobs, each lane type, split and unsplit levels, node order, no alias
table, no Gauss stage, several chunks, two contexts, per-job A and kT, the strict context, an energy on a
group edge -- are compared with tests/golden/item_records_parent.npz, recorded on an MI355X with the
library of the commit before the records (tools/make_item_records_golden.py; the fixture holds the
seeds of the inputs and the outputs).
Needs a real MI355X:  pytest -m gpu"""
import os
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "item_records_parent.npz"
STRICT_LIB = os.environ.get("NDPP_HIP_STRICT") == "1"   # the verification build computes other bits

# the headline workload of bench.py: H-1 at 293 K, three rows linear in mu, two groups
A_H1, KT, CUTOFF, M = 0.999167, 2.5301e-8, 400.0, 2001
BINS = np.array([0.0, 6.25e-7, 20.0])
E_GRID = np.array([1e-11, 1e-6, 20.0])
N_HEADLINE = 100000

# name -> (seed, energies, L, environment, kind)
CASES = {
    "joint": (101, 64, 6, {}, "headline"),
    "no_joint": (102, 64, 6, {"NDPP_HIP_NO_JOINT": "1"}, "headline"),
    "L4": (103, 64, 4, {}, "headline"),
    "L8": (104, 64, 8, {}, "headline"),
    "L11": (105, 64, 11, {}, "headline"),
    "no_split": (106, 64, 6, {"NDPP_HIP_NO_SPLIT": "1"}, "headline"),
    "no_sort": (107, 64, 6, {"NDPP_HIP_NO_SORT": "1"}, "headline"),
    "no_sort_no_split": (108, 64, 6, {"NDPP_HIP_NO_SORT": "1", "NDPP_HIP_NO_SPLIT": "1"}, "headline"),
    "no_alias": (109, 64, 6, {"NDPP_HIP_NO_ALIAS": "1"}, "headline"),
    "no_gauss": (110, 64, 6, {"NDPP_HIP_GAUSS": "0"}, "headline"),
    "three_chunks": (111, 64, 6, {"NDPP_HIP_MAX_CHUNK_EIN": "22"}, "headline"),
    "two_contexts": (112, 200, 6, {}, "headline"),
    "mixed_nuclides": (113, 64, 6, {}, "multi"),
    "stepped_table": (114, 16, 6, {}, "stepped"),
    "group_edge": (115, 8, 6, {}, "edge"),
}


def headline_energies(rng, n):
    grid = np.logspace(-11, np.log10(CUTOFF * KT), N_HEADLINE)
    return np.ascontiguousarray(grid[np.sort(rng.choice(N_HEADLINE, n, replace=False))])


def brackets(ein):
    row = (np.searchsorted(E_GRID, ein, side="right") - 1).clip(0, 1).astype(np.int32)
    return row, (ein - E_GRID[row]) / (E_GRID[row + 1] - E_GRID[row])


def run_case(hip, name, setenv, delenv):
    """(moments, status) of one case; setenv / delenv: monkeypatch's, or os.environ's."""
    seed, n, L, env, kind = CASES[name]
    rng = np.random.default_rng(seed)
    mu = hip.mu_grid(M)
    lin = np.ascontiguousarray(np.stack([np.full(M, 0.5), 0.5 * (1 + 0.1 * mu), 0.5 * (1 + 0.3 * mu)]))
    p = hip.Params.default(L, M)
    for k, v in env.items():
        setenv(k, v)
    try:
        if kind == "multi":
            # four nuclides with their own A and kT, their energies interleaved
            n_nuc = 4
            A = np.exp(rng.uniform(0.0, np.log(240.0), n_nuc))
            kT = KT * rng.uniform(1.0, 4.0, n_nuc)
            nuc = (np.arange(n) % n_nuc).astype(np.int32)
            ein = 10 ** rng.uniform(-10, np.log10(300 * kT[nuc]))
            row = (rng.integers(0, 2, n) + 3 * nuc).astype(np.int32)
            out, status = hip.elastic_leg_multi(p, A, kT, np.full(n_nuc, 1e300), np.zeros(n_nuc), ein, nuc, row,
                                                rng.uniform(0, 1, n), np.concatenate([lin] * n_nuc), BINS)
        else:
            ein = headline_energies(rng, n)
            f_tab = lin
            if kind == "stepped":
                # rows that are no straight lines: these energies go to the context of the reference arithmetic
                f_tab = np.ascontiguousarray(np.stack([np.where(mu < 0.2, 0.4, 0.6), np.where(mu < -0.3, 0.3, 0.7),
                                                       np.where(mu < 0.5, 0.45, 0.55)]))
            if kind == "edge":
                # E_in on the edge between the groups: neither group has a [.., E_in] segment (dead roots), and
                # the upper group's low tail has zero width
                ein = np.sort(np.concatenate([ein[:n - 1], [BINS[1]]]))
            row, w = brackets(ein)
            out, status = hip.elastic_leg_batch(p, A_H1, KT, 1e300, 0.0, ein, row, w, f_tab, BINS)
    finally:
        for k in env:
            delenv(k)
    return out, status


@pytest.fixture(scope="module")
def parent():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_have_the_bits_of_the_walk_that_gathered_its_own_set_up(hip, monkeypatch, parent, name):
    if STRICT_LIB:
        return      # (recorded with the product library)
    assert int(parent[f"seed_{name}"]) == CASES[name][0] and int(parent[f"n_{name}"]) == CASES[name][1]
    out, status = run_case(hip, name, monkeypatch.setenv, monkeypatch.delenv)
    ref, ref_status = parent[f"out_{name}"], parent[f"status_{name}"]
    assert out.shape == ref.shape and out.dtype == ref.dtype
    differ = int((out.view(np.uint64) != ref.view(np.uint64)).sum())
    print(f"{name}: {out.size} moments, {differ} differ in some bit; status {np.unique(status).tolist()}")
    assert differ == 0
    assert np.array_equal(status, ref_status)
