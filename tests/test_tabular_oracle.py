"""The references that pin the tabular kernels (test_gpu_tabular.py), checked on the CPU against
what is already pinned to the Fortran: the oracle's tabular entries (oracle/c/file6.c -- the
Legendre integrators with the per-panel functional replaced by a clipped long double bin integral)
against the oracle's own Legendre moments, and the numpy restatements of law 9 and file 4."""
import numpy as np
import pytest

from tabular_ref import (BIN_TOL, FILE6_TOL, GROUPS, bin_err, bind_tab, enclosure_violation, file4_level_case,
                         file4_numpy, file6_case, law9_case, law9_numpy, oracle_file6, oracle_law9, p0_scale)

AWRS = (0.9992, 2.0, 11.9, 236.0058)
NS = (1, 3, 7, 128)


@pytest.mark.parametrize("frame", [1, 0], ids=["cm", "lab"])
@pytest.mark.parametrize("M", [2, 3, 5, 33, 513])
def test_file6_oracle_bins_sum_to_p0_and_enclose_the_moments(oracle, M, frame):
    """sum_k of the oracle's bins is the oracle's Legendre P0, to 1e-12 of the E_in's largest P0 for
    M <= 33 and to FILE6_TOL at M = 513 (measured: <= 3.6e-15 for M <= 5; 1.3e-13 CM / 4.7e-15 lab at
    M = 33; 8.9e-12 CM / 3.9e-13 lab at M = 513 -- the growth is the rounding noise of the reference's
    closed-form P0 on narrow CM panels, not the bins), the same (E_in, group) pairs are populated, and
    at N = 128 the bins are non-negative and enclose the moments of orders 1..5 (measured violation:
    0)."""
    bind_tab(oracle)
    worst_sum = worst_enc = 0.0
    tol = BIN_TOL if M <= 33 else FILE6_TOL
    for intt in (1, 2):
        T, ein, row = file6_case(M, intt)
        for awr in AWRS:
            for bins in GROUPS.values():
                leg = oracle_file6(oracle, T, awr, frame, ein, row, bins)
                assert np.isfinite(leg).all()
                for N in NS:
                    tab = oracle_file6(oracle, T, awr, frame, ein, row, bins, n_tab=N)
                    err = (np.abs(tab.sum(axis=2) - leg[:, :, 0]).max(axis=1) / p0_scale(leg[:, :, 0])).max()
                    worst_sum = max(worst_sum, err)
                    assert err <= tol, (intt, awr, len(bins) - 1, N, err)
                    assert np.array_equal(tab.sum(axis=2) != 0, leg[:, :, 0] != 0)
                assert (tab >= 0).all()
                v = enclosure_violation(tab, leg)
                worst_enc = max(worst_enc, v)
                assert v <= FILE6_TOL, (intt, awr, len(bins) - 1, v)
    print(f"oracle file 6 {'cm' if frame else 'lab'} M={M}: |sum_k T - P0| {worst_sum:.2e}; "
          f"enclosure violation {worst_enc:.2e}")


@pytest.mark.parametrize("M", [2, 5, 33, 257])
def test_law9_oracle_bins_match_numpy(oracle, M):
    bind_tab(oracle)
    c = law9_case(M)
    leg = oracle_law9(oracle, c)
    assert (leg[0] == 0).all() and (leg[1:, :, 0].sum(axis=1) > 0).all()
    assert (leg[1, -3:] == 0).all()              # groups above E_in - U
    for N in NS:
        tab = oracle_law9(oracle, c, n_tab=N)
        err, at = bin_err(tab, law9_numpy(c["f_tab"], c["row"], c["w"], leg[:, :, 0], N), leg[:, :, 0])
        print(f"oracle law 9 M={M} N={N}: vs numpy {err:.2e} at (E_in, group, bin) {at}")
        assert err <= BIN_TOL
    assert (tab >= 0).all()
    v = enclosure_violation(tab, leg)
    print(f"oracle law 9 M={M}: enclosure violation {v:.2e}")
    assert v <= FILE6_TOL


@pytest.mark.parametrize("M", [5, 33, 2001])
def test_file4_numpy_level_bins_sum_to_the_trapezoid_p0(M):
    """Q = -0.0449 at A = 236.0058, R from 0.05 to 20: the restatement's bins add up to the plain
    trapezoid P0 in w (measured <= 8e-16)."""
    c = file4_level_case(M)
    assert c["R"].min() < 0.06 and np.abs(c["R"] / np.array([0.05, 0.2, 0.5, 0.9, 0.999999, 1.000001, 1.5, 20.0])
                                          - 1).max() < 1e-6
    for N in (1, 3, 7, 32, 128):
        tab, p0 = file4_numpy(c, N, c["Q"])
        assert (p0.sum(axis=1) > 0).all()
        err = (np.abs(tab.sum(axis=2) - p0).max(axis=1) / p0_scale(p0)).max()
        print(f"file 4 numpy, level, M={M} N={N}: |sum_k T - P0| {err:.2e}")
        assert err <= 1e-14
