"""The file-4 two-body kernels (file4_kernels.hip: file4_wave_kernel, one wave per incoming
energy, and file4_blend_kernel, one thread per (energy, group)) against the C oracle and against
what the reference Fortran wrote into tests/golden/file4_cm_edges.npz -- bit for bit, since only
+ - * / sqrt are involved; every comparison is of bit patterns (synth.same_bits: np.array_equal
that also tells -0.0 from +0.0).  Beyond mu_bins = 2001: on small and odd cosine grids a bound
clamped to +1 falls in cell M (the top-of-grid branch of file4_f_at and the zero-width last piece),
which at M = 2001 it never does.  Needs a real MI355X:  pytest -m gpu"""
import ctypes as C

import numpy as np
import pytest

from conftest import dp, ip, load_golden, oracle_params
from synth import (FILE4_KINDS, FILE4_M, FILE4_TOP_AWR, file4_batch, file4_bins, file4_bound_classes,
                   file4_energies, file4_golden_cases, file4_matrix, file4_tables, file4_top_inputs, mu_grid,
                   same_bits)

pytestmark = pytest.mark.gpu

KT = 2.53e-8      # not read above the cutoff
CUTOFF = 0.0      # freegas_cutoff = 0: every incoming energy is file 4


def oracle_batch(oracle, L, M, A, Q, ein, row_lo, w_hi, f_tab, bins):
    op = oracle_params(oracle, L, M)
    ein, w_hi, f_tab, bins = (np.ascontiguousarray(a, dtype=np.float64) for a in (ein, w_hi, f_tab, bins))
    row_lo = np.ascontiguousarray(row_lo, dtype=np.int32)
    G = len(bins) - 1
    ref = np.zeros((len(ein), G, L))
    rc = oracle.oracle_elastic_leg_batch(C.byref(op), A, KT, CUTOFF, Q, len(ein), dp(ein), ip(row_lo), dp(w_hi),
                                         f_tab.shape[0], dp(f_tab), G, dp(bins), dp(ref), 0, None)
    assert rc == 0
    return ref


def hip_batch(hip, L, M, A, Q, ein, row_lo, w_hi, f_tab, bins):
    out, status = hip.elastic_leg_batch(hip.Params.default(L, M), A, KT, CUTOFF, Q, ein, row_lo, w_hi, f_tab, bins)
    assert (status == 0).all()
    return out


def wave_kernel_fits(G, L):
    """The dynamic LDS of file4_wave_kernel as launch_file4 computes it, against its 48 KiB bound."""
    lmax = 4 if L <= 4 else 6 if L <= 6 else 8 if L <= 8 else 11
    return 8 * 64 * (2 * lmax + 1) + 4 * (64 + G + 1) <= 48 * 1024


@pytest.mark.parametrize("M", FILE4_M)
def test_batch_both_kernels_vs_oracle(hip, oracle, monkeypatch, M):
    """elastic_leg_batch with every energy routed to file 4, one reaction per call, through the wave
    kernel (NDPP_HIP_FILE4_PER_GROUP=0) and the per-group kernel (=1), each against the oracle.

    The subset of M x L x G x kinematics is synth.file4_matrix(): all 60 (M, L) pairs, hence every
    (M, LMAX template) pair and every L below its template; case k = 10 iM + iL takes (G,
    kinematics) pair number 11 k mod 56, which visits each of the 56 pairs (11 and 56 are coprime).
    One test per M runs that M's ten cases.  Each call has ten energies (threshold (1 + 1e-7), that
    times 1.0000001, a ladder to 19.5, the top edge 20, and 25 above it), a random lower row among
    the eight unlike tables (the six shapes and two negated ones, synth.file4_tables; two energies
    blend the two negative rows) and blend weights in [0, 1] with exact 0 and 1.

    Host-side conditions on the inputs, not on the kernels: the reference's cell of a bound clamped
    to +1 is M for every M but 2001 (M - 1 there), and every call has groups whose upper bound
    clamps to +1 while the lower does not."""
    mu = mu_grid(M)
    top_cell = int(2.0 / (mu[1] - mu[0])) + 1
    assert top_cell == (M - 1 if M == 2001 else M)
    cases = [c for c in file4_matrix() if c[0] == M]
    assert len(cases) == 10
    n_top = n_skipped = 0
    for _, L, G, A, Q in cases:
        c = file4_batch(M, L, G, A, Q)
        args = (L, M, A, Q, c["ein"], c["row_lo"], c["w_hi"], c["f_tab"], c["bins"])
        assert 0.0 in c["w_hi"] and 1.0 in c["w_hi"]
        skipped = np.zeros((len(c["ein"]), G), bool)
        top = 0
        for k, Ein in enumerate(c["ein"]):
            wlo, whi, ilo, ihi = file4_bound_classes(M, A, Q, Ein, c["bins"])
            skipped[k] = (wlo == whi) & ((wlo == -1.0) | (wlo == 1.0))
            clamped = (whi == 1.0) & (wlo < 1.0)
            assert (ihi[clamped] == top_cell).all() and ihi.max() <= M
            top += int(clamped.sum())
        assert top >= 1, (M, L, G, A, Q)
        n_top += top
        n_skipped += int(skipped.sum())
        ref = oracle_batch(oracle, *args)
        assert np.isfinite(ref).all()
        for per_group in ("0", "1"):
            monkeypatch.setenv("NDPP_HIP_FILE4_PER_GROUP", per_group)
            got = hip_batch(hip, *args)
            assert same_bits(got, ref), (M, L, G, A, Q, per_group)
            # a group whose two bounds clamp to the same end: exact zeros, and 0 (1 - f) + 0 f is +0.0
            # -- also where both rows are negative, and a zero-width piece would give -0.0
            assert (got[skipped].view(np.uint64) == 0).all(), (M, L, G, A, Q, per_group)
            if Q == 0.0:
                # sum_g P0, the oracle's bits.  (Follows from the comparison above -- both sums run
                # over equal arrays; it says nothing about normalisation, which holds only within
                # the trapezoid rule's error.)
                le20 = c["ein"] <= 20.0
                assert np.array_equal(got[le20, :, 0].sum(axis=1), ref[le20, :, 0].sum(axis=1))
    print(f"M={M}: cell of +1 is {top_cell}; {n_top} groups with only the upper bound clamped to +1, "
          f"{n_skipped} skipped groups")


@pytest.mark.parametrize("M", [M for M in FILE4_M if M != 2001])
def test_value_of_the_top_of_grid_branch(hip, oracle, monkeypatch, M):
    """Where a bound is clamped to +1, what file4_f_at returns for cell M is multiplied by the zero
    width 1 - mu[M - 1] and cannot be seen.  synth.file4_top_inputs has bin edges a few ulps below
    E_in, whose cosine is below 1 and still in cell M: the group above such an edge is one piece
    [w, 1] that starts in cell M, so its moments are f[M - 1] times ~1e-16 and not zero.  Every table
    as the lower row, weights 0, 1 and between, L = 11, both kernels, against the oracle.
    Host-side conditions on the inputs: each energy has such a group, its cell is M for both bounds,
    and the tables' last two values differ (else f[M - 2] would do as well)."""
    ein0, bins = file4_top_inputs(M)
    assert len(ein0) >= 2
    mu = mu_grid(M)
    f_tab = file4_tables(mu, M)
    nk = len(FILE4_KINDS)
    assert (f_tab[:, M - 1] != f_tab[:, M - 2]).sum() >= nk - 2     # (the step has 1.0 twice)
    ein = np.repeat(ein0, nk - 1)
    row_lo = np.tile(np.arange(nk - 1), len(ein0))
    w_hi = np.tile(np.array([0.0, 1.0, 0.25, 0.5, 0.75, 0.125, 0.875])[:nk - 1], len(ein0))
    at_top = np.zeros((len(ein), len(bins) - 1), bool)
    for k, Ein in enumerate(ein):
        wlo, whi, ilo, ihi = file4_bound_classes(M, FILE4_TOP_AWR, 0.0, Ein, bins)
        at_top[k] = (wlo < 1.0) & (ilo == M) & (ihi == M)
        assert at_top[k].sum() == 1 and ilo.max() <= M and ihi.max() <= M
    args = (11, M, FILE4_TOP_AWR, 0.0, ein, row_lo, w_hi, f_tab, bins)
    ref = oracle_batch(oracle, *args)
    assert np.isfinite(ref).all() and (ref[at_top][:, 0] != 0.0).all()
    for per_group in ("0", "1"):
        monkeypatch.setenv("NDPP_HIP_FILE4_PER_GROUP", per_group)
        assert same_bits(hip_batch(hip, *args), ref), (M, per_group)


@pytest.mark.parametrize("G,L,A,Q,fits", [(12000, 4, 0.999167, 0.0, False), (9500, 11, 236.0058, -0.0449, False),
                                          (9000, 11, 236.0058, -0.0449, True)])
def test_group_structures_around_the_lds_bound(hip, oracle, G, L, A, Q, fits):
    """launch_file4 runs file4_blend_kernel when the wave kernel's prefix array does not fit 48 KiB of
    LDS: G = 12 000 at LMAX = 4 and G = 9 500 at LMAX = 11 are above that bound, G = 9 000 at LMAX = 11
    is the largest wave-kernel case next to it.  No environment switch: the launch decides."""
    assert wave_kernel_fits(G, L) == fits
    M = 65
    mu = mu_grid(M)
    rng = np.random.default_rng(G + L)
    ein = file4_energies(A, Q)[[0, 3, 6, 8, 9]]
    row_lo = rng.integers(0, len(FILE4_KINDS) - 1, len(ein))
    w_hi = rng.uniform(0.0, 1.0, len(ein))
    args = (L, M, A, Q, ein, row_lo, w_hi, file4_tables(mu, M), file4_bins(G))
    ref = oracle_batch(oracle, *args)
    assert np.isfinite(ref).all() and np.count_nonzero(ref) > 0
    assert same_bits(hip_batch(hip, *args), ref)


def test_more_energies_than_blocks(hip, oracle):
    """70 000 energies: the wave kernel launches 65 536 blocks and its grid-stride loop takes the
    rest (so does the per-group kernel's)."""
    n, G, L, M, A, Q = 70000, 2, 1, 65, 0.999167, 0.0
    mu = mu_grid(M)
    rng = np.random.default_rng(70000)
    ein = rng.permutation(np.geomspace(1e-6, 19.5, n))
    row_lo = rng.integers(0, len(FILE4_KINDS) - 1, n)
    w_hi = rng.uniform(0.0, 1.0, n)
    args = (L, M, A, Q, ein, row_lo, w_hi, file4_tables(mu, M), file4_bins(G))
    ref = oracle_batch(oracle, *args)
    got = hip_batch(hip, *args)
    assert same_bits(got, ref)
    assert np.count_nonzero(got[65536:]) > 0


@pytest.mark.parametrize("M", FILE4_M)
def test_single_call_vs_oracle_and_fortran_golden(hip, oracle, M):
    """ndpp_integrate_file4_cm_leg on the calls of file4_cm_edges.npz: the bits of the oracle and of
    the reference Fortran that wrote the file."""
    g = load_golden("file4_cm_edges")
    mu = mu_grid(M)
    n = 0
    for _, L, G, A, Q, Ein, kind, fw, bins, ref in file4_golden_cases(g, M):
        p = oracle_params(oracle, L, M)
        orc = np.zeros((G, L))
        oracle.oracle_integrate_file4_cm_leg(C.byref(p), dp(fw), Ein, A, Q, dp(bins), G + 1, dp(mu), dp(orc))
        got = hip.integrate_file4_cm_leg(fw, Ein, A, Q, bins, mu, L).T
        assert same_bits(got, orc), (M, L, G, A, Q, Ein, FILE4_KINDS[kind])
        assert same_bits(got, ref), (M, L, G, A, Q, Ein, FILE4_KINDS[kind])
        n += 1
    assert n >= 30      # 30 of the matrix and, below M = 2001, the top-of-grid inputs
