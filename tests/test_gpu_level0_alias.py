"""Level 0 of the free-gas pipeline integrates each distinct E_out once: the segments of a group are
chained end to end (fg_pipeline.h fg_setup_group), so the lower end of a live segment is the very
double at which the live segment before it ends -- in the group, or at the top of the group below --
and takes that task's inner integrals instead of repeating them (FgBatch::t_alias).
NDPP_HIP_NO_ALIAS=1 integrates every end point as before.  Same inputs, same arithmetic: same bits.
An alias is flagged in the task's Gauss-rule byte, so the table exists where that byte does: in the
contexts of the product arithmetic with the Gauss stage on (the tables here are linear in mu).
Needs a real MI355X:  pytest -m gpu"""
import os

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

STRICT_LIB = os.environ.get("NDPP_HIP_STRICT") == "1"   # the verification build: no Gauss-rule byte, no aliases

KT = 2.5301e-8
H1 = 0.999167
TWO = np.array([0.0, 6.25e-7, 20.0])

# name -> (A, L, bins, incoming energies, a chain of segments exists).  Every energy here is above
# 1e-4 kT, so every list runs in the product arithmetic as a whole.
CASES = {
    # alpha E_in (alpha = ((A - 1) / (A + 1))^2) is a point of its own inside the window
    "h1": (H1, 6, TWO, np.geomspace(1e-10, 1e-5, 64), True),
    # A = 1 exactly: alpha = 0, no [Elo, alpha E_in] segment
    "a1": (1.0, 6, TWO, np.geomspace(1e-10, 1e-5, 64), True),
    # heavy target: alpha E_in = 0.983 E_in sits next to E_in
    "a236": (236.0058, 6, TWO, np.geomspace(1e-9, 1e-5, 64), True),
    # E_in exactly on a group edge: no [.., E_in] segment in either group
    "ein_on_edge": (H1, 6, TWO, np.concatenate([np.geomspace(3e-7, 1.2e-6, 63), [6.25e-7]]), True),
    # the upper group lies wholly above the window (the `else` branch); the lower one is chained
    "group_outside": (H1, 6, np.array([0.0, 1.0, 20.0]), np.geomspace(1e-10, 1e-6, 64), True),
    # nothing but the `else` branch: one segment per job, nothing shared
    "all_outside": (H1, 6, np.array([1.0, 20.0]), np.geomspace(1e-10, 1e-7, 64), False),
    # bins[0] > 0: the low tail starts at the group edge, not at Elo / 100
    "bins0_positive": (H1, 6, np.array([1e-9, 6.25e-7, 20.0]), np.geomspace(1e-10, 1e-5, 64), True),
    "g1": (H1, 6, np.array([0.0, 20.0]), np.geomspace(1e-10, 1e-5, 64), True),
    # neighbouring groups both inside the window: the top of one is the bottom of the next
    "g5": (H1, 6, np.array([0.0, 1e-8, 3e-8, 1e-7, 6.25e-7, 20.0]), np.geomspace(1e-9, 1e-6, 64), True),
    # L > 8: one row per job (R = 1)
    "p10_single_row": (H1, 11, TWO, np.geomspace(1e-10, 1e-5, 64), True),
}

# aliases per case, counted by tests/aliascheck on these very energies with one job per energy
# (tests/test_level0_alias_table.py asserts them): an alias is one inner integral less
ALIASES = {"h1": 320, "a1": 192, "a236": 320, "ein_on_edge": 319, "group_outside": 320, "all_outside": 0,
           "bins0_positive": 179, "g1": 256, "g5": 510, "p10_single_row": 320}


def run(hip, monkeypatch, name, **env):
    A, L, bins, ein, _ = CASES[name]
    f_tab = load_golden("freegas_h1_p3")["f_tab"]
    row_lo = (np.arange(len(ein)) % (f_tab.shape[0] - 1)).astype(np.int32)
    w_hi = np.linspace(0.05, 0.95, len(ein))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out, status, st = hip.elastic_leg_batch(hip.Params.default(L, f_tab.shape[1]), A, KT, 1e300, 0.0, ein, row_lo,
                                            w_hi, f_tab, bins, want_stats=True)
    for k in env:
        monkeypatch.delenv(k)
    return out, status, st


@pytest.mark.parametrize("no_split", ["0", "1"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_aliased_level0_points_have_the_bits_of_their_own_integrals(hip, monkeypatch, name, no_split):
    on, s_on, st_on = run(hip, monkeypatch, name, NDPP_HIP_NO_SPLIT=no_split)
    off, s_off, st_off = run(hip, monkeypatch, name, NDPP_HIP_NO_SPLIT=no_split, NDPP_HIP_NO_ALIAS="1")
    n_on = st_on.mu_integrals + st_on.gauss_integrals
    n_off = st_off.mu_integrals + st_off.gauss_integrals
    print(f"{name} no_split={no_split}: inner integrals {n_off} -> {n_on}")
    assert np.array_equal(on, off, equal_nan=True) and np.array_equal(s_on, s_off)
    if CASES[name][4]:
        assert (s_on == 0).all() and np.isfinite(on).all()
    if STRICT_LIB:
        assert n_on == n_off
    else:
        # every alias honoured, by every stage: L > 8 walks the two rows of an energy as two jobs
        assert n_off - n_on == ALIASES[name] * (2 if CASES[name][1] > 8 else 1)
