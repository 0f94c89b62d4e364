"""CPU: ACE law 66 (N-body phase space) in lab-cosine bins -- the definition of ndpp_nbody_tab_batch as
tests/nbody_tab_ref.py restates it, the host half of the entry point and of the option, and the driver's
refusals.  The kernel itself is tests/test_gpu_nbody_tab.py.

The cases are those of tests/test_nbody.py (CASES, energies(), B5, B70), N = 1, 7, 32 on the 5-group
structure and N = 8 on the 70-group one.  Measured on them with the numpy restatements (float64; each
bound below is 10 x the figure; the restatements are the measure, never the kernel):
  32 against 96 points of the same scheme: FIG_CONV absolute on rows of total mass 1, in the most forward
    of 32 bins of n = 3, A = 236 at 14 MeV (per case: 1.721e-14, 8.549e-15, 1.443e-15, 1.868e-13)
  sum over the bins against nbody_numpy's P0 of the group: FIG_SUM (per case: 2.587e-14, 7.216e-15,
    1.887e-15, 5.334e-12, the last at N = 32 and 2.232e-14 at N = 7; the Legendre rule's own 32-against-96
    error is 1.7e-11)
  sum over groups and bins - 1, edges that cover the window: FIG_ONE (the same row)
  96 points against the CM route at 4000 panels: FIG_CM of the row's largest group (the CM route
    converges algebraically)
  bins enclose the moments of nbody_converged, l = 1..5: no violation, FIG_ENC = 0; the slack of the test is
    the 32-against-96 figure
  N = 14 summed in pairs against N = 7: FIG_REF
  both roots of a bin edge inside the range (Emax = 0.25, 0.5, 0.9 E0, which the energies above do not
    reach: they have Emax > E0, or Emax so far below E0 that only mu = 1 is inside), N = 7 and 32:
    32 against 96 points FIG_ROOTS_CONV, sum over the bins against P0 FIG_ROOTS_SUM.  With the lower
    root left out of the breakpoints these are 1.3e-5 and 8.3e-6, and nothing else in this file moves.
  heavy target (A = 1e6, n = 4, Q = -1, Ap = 4, E = 2 and 10, 6 groups, N = 8): bins against P0 / N:
    FIG_HEAVY (the physics of a finite A, sqrt(E0 / Emax) = 1.6e-6, as in tests/test_nbody.py's large-A
    test).  32 against 96 points there: 1.9e-16 at N = 8 and 6.7e-16 at N = 1 for n = 4 (and n = 5), whose D
    has no square root near its branch point; for n = 3 (Ap = 3) at the same A 7.5e-10 at N = 1, 2.9e-11
    at N = 8, 1.4e-12 at N = 32 -- the known limit E0 << Emax of the 32-point rule (3.1e-11 at A = 0.9992,
    Q = +0.5, E = 1e-6 MeV, N = 32), see profiles/nbody_tab/README.md; recorded, not a bound of this
    file."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
import nbody_ref
from conftest import dp, ip
from nbody_ref import nbody_converged, nbody_numpy, threshold
from nbody_tab_ref import nbody_tab_cm_check, nbody_tab_converged, nbody_tab_numpy, tab_edges

ROOT = Path(__file__).resolve().parent.parent
CASES = [(3, 1.9968, -2.2246, 2.9986), (4, 8.9, -1.6, 4.0), (5, 11.9, -7.0, 5.0), (3, 236.0, -6.2, 3.0)]
B5 = np.array([0.0, 1e-3, 0.1, 1.0, 5.0, 20.0])
B70 = np.concatenate([[0.0], np.geomspace(1e-11, 20.0, 70)])
SHAPES = [("b5", B5, 1), ("b5", B5, 7), ("b5", B5, 32), ("b70", B70, 8)]

FIG_CONV = 1.868e-13
FIG_SUM = 5.334e-12
FIG_ONE = 5.338e-12
FIG_CM = 3.645e-07
FIG_ENC = 0.0
FIG_REF = 6.987e-14
FIG_HEAVY = 5.409e-07
FIG_ROOTS_CONV = 4.774e-15
FIG_ROOTS_SUM = 2.998e-15


def energies(A, Q):
    thr = threshold(A, Q)
    return np.array([e for e in (thr * (1.0 + 1e-6), 6.0, 14.0, 19.9) if e > thr])


@pytest.fixture(scope="module")
def rows(hip):
    """per case and shape: the 32-point rows, the 96-point rows and the Legendre P0, computed once"""
    out = {}
    for case in CASES:
        n, A, Q, Ap = case
        E = energies(A, Q)
        p0 = {name: nbody_numpy(A, Q, n, Ap, E, bins, 1)[0][:, :, 0] for name, bins in (("b5", B5), ("b70", B70))}
        for name, bins, N in SHAPES:
            t32, st = nbody_tab_numpy(A, Q, n, Ap, E, bins, N)
            assert not st.any()
            out[case, name, N] = (t32, nbody_tab_converged(A, Q, n, Ap, E, bins, N), p0[name])
    return out


def test_rule_against_the_finer_rule(rows):
    worst = max(np.abs(a - b).max() for a, b, _ in rows.values())
    print(f"32 against 96 points: {worst:.3e}")
    assert worst <= 10 * FIG_CONV


def test_bins_sum_to_the_legendre_p0(rows):
    worst = max(np.abs(a.sum(axis=2) - p0).max() for a, _, p0 in rows.values())
    print(f"sum of the bins - P0: {worst:.3e}")
    assert worst <= 10 * FIG_SUM


def test_rows_sum_to_one_when_the_edges_cover_the_window(rows):
    worst = max(np.abs(a.sum(axis=(1, 2)) - 1.0).max() for a, _, _ in rows.values())
    print(f"sum over groups and bins - 1: {worst:.3e}")
    assert worst <= 10 * FIG_ONE


def test_finer_rule_against_the_cm_route(rows):
    worst = 0.0
    for (case, name, N), (_, b, _) in rows.items():
        n, A, Q, Ap = case
        c = nbody_tab_cm_check(A, Q, n, Ap, energies(A, Q), B5 if name == "b5" else B70, N)
        worst = max(worst, (np.abs(b - c).max(axis=(1, 2)) / b.sum(axis=2).max(axis=1)).max())
    print(f"96 points against the CM route, of the row's largest group: {worst:.3e}")
    assert worst <= 10 * FIG_CM


def legendre_range(l, m0, m1):
    """(min, max) of P_l over [m0, m1]: the ends and the stationary points inside"""
    P = np.polynomial.legendre.Legendre.basis(l)
    at = [m0, m1] + [float(r.real) for r in P.deriv().roots() if m0 < r.real < m1]
    v = P(np.array(at))
    return v.min(), v.max()


def test_bins_enclose_the_moments(rows):
    worst = 0.0
    for (case, name, N), (t32, _, _) in rows.items():
        n, A, Q, Ap = case
        mom = nbody_converged(A, Q, n, Ap, energies(A, Q), B5 if name == "b5" else B70, 6)
        edges = tab_edges(N)
        for l in range(1, 6):
            rng = np.array([legendre_range(l, edges[k], edges[k + 1]) for k in range(N)])
            lower, upper = (t32 * rng[:, 0]).sum(axis=2), (t32 * rng[:, 1]).sum(axis=2)
            worst = max(worst, (lower - mom[:, :, l]).max(), (mom[:, :, l] - upper).max())
    print(f"moments outside their enclosure by at most {worst:.3e}")
    assert worst <= max(10 * FIG_ENC, FIG_CONV)             # (no violation measured: the 32-against-96 figure)


def test_refinement(hip):
    worst = 0.0
    for n, A, Q, Ap in CASES:
        E = energies(A, Q)
        fine, coarse = nbody_tab_numpy(A, Q, n, Ap, E, B5, 14)[0], nbody_tab_numpy(A, Q, n, Ap, E, B5, 7)[0]
        worst = max(worst, np.abs(fine[:, :, 0::2] + fine[:, :, 1::2] - coarse).max())
    print(f"N = 14 in pairs against N = 7: {worst:.3e}")
    assert worst <= 10 * FIG_REF


def energy_at_ratio(A, Q, Ap, ratio):
    """the incoming energy at which Emax = ratio * E0"""
    f = (Ap - 1.0) / Ap
    return -Q * f / (f * A / (A + 1.0) - ratio / (A + 1.0) ** 2)


def test_both_roots_of_an_edge_inside_the_range(hip):
    d_conv = d_sum = 0.0
    for n, A, Q, Ap in CASES:
        E = np.array([energy_at_ratio(A, Q, Ap, r) for r in (0.25, 0.5, 0.9)])
        Emax, E0 = nbody_ref._setup(A, Q, Ap, E)
        assert np.abs(Emax / E0 - [0.25, 0.5, 0.9]).max() < 1e-9
        p0 = nbody_numpy(A, Q, n, Ap, E, B5, 1)[0]
        for N in (7, 32):
            t32 = nbody_tab_numpy(A, Q, n, Ap, E, B5, N)[0]
            assert (t32 >= 0.0).all()
            d_conv = max(d_conv, np.abs(t32 - nbody_tab_converged(A, Q, n, Ap, E, B5, N)).max())
            d_sum = max(d_sum, np.abs(t32.sum(axis=2, keepdims=True) - p0).max())
    print(f"Emax < E0, both roots inside: 32 against 96 points {d_conv:.3e}, sum of the bins - P0 {d_sum:.3e}")
    assert d_conv <= 10 * FIG_ROOTS_CONV and d_sum <= 10 * FIG_ROOTS_SUM


def test_exact_zeros_and_no_negative_bin(rows):
    seen_below = seen_outside = 0
    for (case, name, N), (t32, t96, _) in rows.items():
        n, A, Q, Ap = case
        assert (t32 >= 0.0).all() and (t96 >= 0.0).all()
        E = energies(A, Q)[0]                                # the near-threshold energy
        Emax, E0 = nbody_ref._setup(A, Q, Ap, E)
        assert 0.0 < Emax < E0
        below = tab_edges(N)[1:] < np.sqrt(1.0 - Emax / E0)  # bins wholly below the smallest lab cosine
        assert not t32[0][:, below].any()
        seen_below += int(below.sum())
        rE0, rEm = np.sqrt(E0), np.sqrt(Emax)
        bins = B5 if name == "b5" else B70
        outside = (bins[1:] <= (rE0 - rEm) ** 2 * (1.0 - 1e-12)) | (bins[:-1] >= (rE0 + rEm) ** 2 * (1.0 + 1e-12))
        assert not t32[0][outside].any() and t32[0][~outside].any()
        seen_outside += int(outside.sum())
    assert seen_below > 0 and seen_outside > 0


def test_rows_at_or_below_the_threshold_are_zero(hip):
    for n, A, Q, Ap in CASES:
        thr = threshold(A, Q)
        out, st = nbody_tab_numpy(A, Q, n, Ap, [0.5 * thr, thr, float(np.nextafter(thr, np.inf))], B5, 7)
        assert not out[:2].any() and out[2].any() and (out >= 0.0).all() and not st.any()


def test_heavy_target(hip):
    A, n, Q, Ap, N = 1e6, 4, -1.0, 4.0, 8
    bins = np.array([0.0, 0.1, 0.5, 1.0, 2.0, 5.0, 20.0])
    E = np.array([2.0, 10.0])
    t32 = nbody_tab_numpy(A, Q, n, Ap, E, bins, N)[0]
    p0 = nbody_numpy(A, Q, n, Ap, E, bins, 1)[0]
    d = np.abs(t32 - p0 / N).max()
    conv = np.abs(t32 - nbody_tab_converged(A, Q, n, Ap, E, bins, N)).max()
    conv1 = np.abs(nbody_tab_numpy(A, Q, n, Ap, E, bins, 1)[0] - nbody_tab_converged(A, Q, n, Ap, E, bins, 1)).max()
    print(f"A = 1e6: bins against P0 / N {d:.3e}; 32 against 96 points {conv:.3e} (N = 8), {conv1:.3e} (N = 1)")
    assert (t32 >= 0.0).all()
    assert d <= 10 * FIG_HEAVY


# ---- the host half ----------------------------------------------------------------------------------
def _args(hip, **kw):
    v = dict(n_tab=8, awr=1.9968, Q=-2.2246, n=3, Ap=2.9986, n_ein=2, G=2, mu_bins=65)
    v.update(kw)
    p = hip.Params.default(4, v["mu_bins"])
    ein, bins = np.array([6.0, 14.0]), np.array([0.0, 1.0, 20.0])
    out, st = np.zeros(2 * 2 * 128), np.zeros(2, np.int32)
    hold = (p, ein, bins, out, st)
    return hold, [C.byref(p), v["n_tab"], v["awr"], v["Q"], v["n"], v["Ap"], v["n_ein"], dp(ein), v["G"], dp(bins),
                  dp(out), ip(st)]


# the bad arguments of the Legendre call (tests/test_nbody.py: BAD) without its order -- tabular output
# does not read the order, as in every other tabular call -- and n_tab outside 1..NDPP_MAX_TAB_BINS
BAD = [dict(n_tab=0), dict(n_tab=-1), dict(n_tab=129), dict(n=2), dict(n=6), dict(Ap=1.0), dict(Ap=0.5),
       dict(Ap=float("nan")), dict(Ap=float("inf")), dict(awr=0.0), dict(awr=-1.0), dict(awr=float("nan")),
       dict(Q=float("nan")), dict(Q=float("inf")), dict(n_ein=-1), dict(G=0), dict(mu_bins=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_entry_refuses_before_the_device(hip, bad):
    lib = hip.load()
    hold, args = _args(hip, **bad)
    assert lib.ndpp_nbody_tab_batch(*args) == -22
    assert lib.ndpp_last_error()
    del hold


def test_entry_null_arguments_and_the_empty_call(hip):
    lib = hip.load()
    hold, args = _args(hip)
    for at in (0, 7, 9, 10):                                 # params, ein, e_bins, out
        a = list(args)
        a[at] = None
        assert lib.ndpp_nbody_tab_batch(*a) == -22
    a = list(args)
    a[11] = None                                             # status may be NULL: not an argument error
    if lib.ndpp_device_count() == 0:
        assert lib.ndpp_nbody_tab_batch(*a) == -5
        assert lib.ndpp_nbody_tab_batch(*args) == -5
        assert b"no HIP device" in lib.ndpp_last_error()
    hold0, empty = _args(hip, n_ein=0)
    assert lib.ndpp_nbody_tab_batch(*empty) == 0             # nothing to do needs no device
    out, st = hip.nbody_tab_batch(hip.Params.default(4, 65), 8, 1.9968, -2.2246, 3, 2.9986, np.zeros(0), B5)
    assert out.shape == (0, 5, 8) and st.shape == (0,)
    del hold, hold0


def test_option_round_trip(hip):
    assert hip.get_nbody_tab() is False                      # the default
    assert hip.set_nbody_tab(True) is False and hip.get_nbody_tab() is True
    assert hip.get_nbody() is False                          # an option of its own
    assert hip.set_nbody_tab(True) is True
    assert hip.set_nbody_tab(False) is True and hip.get_nbody_tab() is False
    lib = hip.load()
    assert lib.ndpp_set_nbody_tab(7) == 0 and lib.ndpp_get_nbody_tab() == 1 and lib.ndpp_set_nbody_tab(0) == 1


def _tabular_run(tmp_path, nuc, **kw):
    run = tmp_path / "run"
    ace_synth.write_inputs(run, "1002.80c", nuc, scatt_order=8, mu_bins=nuc["mu_bins"], threads=1, **kw)
    xml = run / "ndpp.xml"
    xml.write_text(xml.read_text().replace("<scatt_type>legendre</scatt_type>", "<scatt_type>tabular</scatt_type>"))
    return run


def test_run_with_the_flag_and_hdf5_is_still_an_input_error(tmp_path):
    nuc = ace_synth.quantise(nbody_ref.nbody_nuclide())
    run = _tabular_run(tmp_path, nuc, output_format="hdf5")
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), "--nbody-tabular"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 2 and "input error" in r.stderr
    assert not list(run.glob("*.g5")) and not (run / "ndpp_lib.xml").exists()
