"""The order ladder of the Legendre launchers (kernels.h dispatch_lmax: kernels instantiated for 4, 6,
8 and 11 orders, the rungs breaking at 4/5, 6/7 and 8/9) on every path that goes through it, at
every order 1 ... 11 and the smallest shapes -- 3 incoming energies, 3 groups, 33 cosines, 3 lab
energies per group -- against the oracle, each path with the comparison of its own tests: bit
patterns for file 4 (tests/test_gpu_file4.py), the 1e-10 scale-aware bar for file 6 and law 9
(tests/test_gpu_file6.py).  And law 9's tabular output through the sink it now shares with the
Legendre moments.  -m gpu"""
import ctypes as C

import numpy as np
import pytest

from conftest import dp, ip, oracle_params, scale_rel_err
from synth import kalbach_rows, law9_edata, mu_grid, same_bits
from test_file6_oracle import bind
from test_gpu_file6 import FILE6_TOL
from test_gpu_tabular import sum_rule_err

pytestmark = pytest.mark.gpu

M, NEG = 33, 3
ORDERS = list(range(1, 12))


def _params(hip, oracle, L):
    p, op = hip.Params.default(L, M), oracle_params(oracle, L, M)
    p.ne_per_grp = op.ne_per_grp = NEG
    return p, op


def law9_case():
    mu = mu_grid(M)
    f_tab = np.array([0.5 * (1.0 + a * mu + b * (1.5 * mu * mu - 0.5)) for a, b in ((0.1, 0.0), (0.3, 0.2), (-0.2, 0.3))])
    e_grid = np.array([1.0, 5.0, 20.0])
    ein = np.array([2.0, 7.0, 15.0])
    row = np.array([0, 1, 1], np.int32)
    w = (ein - e_grid[row]) / (e_grid[row + 1] - e_grid[row])
    return ein, row, w, f_tab, law9_edata(1.0, 20.0), np.array([0.0, 0.5, 2.0, 20.0])


@pytest.mark.parametrize("L", ORDERS)
def test_law9_every_order_vs_oracle(hip, oracle, L):
    bind(oracle)
    p, op = _params(hip, oracle, L)
    ein, row, w, f_tab, edata, bins = law9_case()
    out, st = hip.law9_leg_batch(p, ein, row, w, f_tab, edata, bins)
    ref = np.zeros_like(out)
    assert oracle.oracle_law9_leg_batch(C.byref(op), len(ein), dp(ein), ip(row), dp(w), len(f_tab), dp(f_tab),
                                        dp(edata), len(bins) - 1, dp(bins), dp(ref), 0) == 0
    err = scale_rel_err(out, ref)
    print(f"law 9, L = {L}: {err:.2e}")
    assert out.shape == (3, 3, L) and (st == 0).all() and np.abs(ref[:, :, 0]).max() > 0.1
    assert err < FILE6_TOL


@pytest.mark.parametrize("frame", [1, 0], ids=["cm", "lab"])
@pytest.mark.parametrize("L", ORDERS)
def test_file6_every_order_vs_oracle(hip, oracle, L, frame):
    bind(oracle)
    p, op = _params(hip, oracle, L)
    T = kalbach_rows(M, 3, 4, 6, 0.5, 20.0, seed=3)
    ein = np.array([0.8, 3.0, 17.0])
    row = (np.searchsorted(T["e_grid"], ein, side="right") - 1).clip(0, 1).astype(np.int32)
    bins = np.array([0.0, 0.1, 1.0, 20.0])
    out, st = hip.file6_leg_batch(p, 236.0058, frame, ein, row, T["e_grid"], T["row_ptr"], T["eout"], T["pdf"],
                                  T["intt"], T["f"], bins)
    ref = np.zeros_like(out)
    assert oracle.oracle_file6_leg_batch(C.byref(op), 236.0058, frame, len(ein), dp(ein), ip(row), 3, dp(T["e_grid"]),
                                         ip(T["row_ptr"]), dp(T["eout"]), dp(T["pdf"]), ip(T["intt"]), dp(T["f"]),
                                         len(bins) - 1, dp(bins), dp(ref), 0) == 0
    err = scale_rel_err(out, ref)
    print(f"file 6 {'cm' if frame else 'lab'}, L = {L}: {err:.2e}")
    assert out.shape == (3, 3, L) and np.isfinite(ref).all() and (st == 0).all()
    assert np.array_equal(ref[:, :, 0] != 0, out[:, :, 0] != 0)
    assert err < FILE6_TOL


@pytest.mark.parametrize("L", ORDERS)
def test_file4_single_call_every_order_vs_oracle(hip, oracle, L):
    mu = mu_grid(M)
    fw = 0.5 * (1.0 + 0.3 * mu + 0.2 * (1.5 * mu * mu - 0.5))
    A, Q, Ein = 11.9, 0.0, 2.0                     # E_out from 1.43 to 2 MeV: groups 2 and 3
    bins = np.array([0.0, 1.0, 1.7, 20.0])
    op = oracle_params(oracle, L, M)
    ref = np.zeros((3, L))
    oracle.oracle_integrate_file4_cm_leg(C.byref(op), dp(fw), Ein, A, Q, dp(bins), 4, dp(mu), dp(ref))
    got = hip.integrate_file4_cm_leg(fw, Ein, A, Q, bins, mu, L).T
    assert got.shape == (3, L) and (ref[0] == 0).all() and (ref[1:, 0] > 0.1).all()
    assert same_bits(got, ref)


def test_law9_tabular_through_the_shared_sink(hip):
    """law9_tab_batch at n_tab = 1 and 4: the single bin is the P0 column of law9_leg_batch and four
    bins add up to it (the bar of test_law9_sum_rule_and_restatement), no status bit, and a repeat
    call gives the same bits."""
    p = hip.Params.default(4, M)
    args = law9_case()
    leg, st = hip.law9_leg_batch(p, *args)
    assert (st == 0).all()
    for N in (1, 4):
        tab, st = hip.law9_tab_batch(p, N, *args)
        assert tab.shape == (3, 3, N) and (st == 0).all()
        assert sum_rule_err(tab, leg) <= 1e-13
        again, st = hip.law9_tab_batch(p, N, *args)
        assert np.array_equal(again, tab) and (st == 0).all()
    one, _ = hip.law9_tab_batch(p, 1, *args)
    scale = np.abs(leg[:, :, 0]).max(axis=1)
    assert (np.abs(one[:, :, 0] - leg[:, :, 0]).max(axis=1) <= 1e-13 * scale).all()
