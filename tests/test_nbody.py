"""CPU: ACE law 66 (N-body phase space) -- the definition of ndpp_nbody_leg_batch as tests/nbody_ref.py
restates it, the host half of the entry point and of the option, the ACE reader and the driver's
refusal.  The kernel itself is tests/test_gpu_nbody.py.

Measured on the committed cases (float64, numpy; each bound below is 10 x the figure):
  large-A limit (A = 1e6, n = 4, Q = -1, Ap = 4, E = 2 and 10, 6 groups): group masses against the
    closed-form CDF of x^(1/2) (1 - x)^2: 1.285e-11; |P_l / P0|, l = 1..10: 8.807e-06 (both are the
    physics of a finite A, E0 / Emax = 1e-12 E / Emax, not rounding)
  32 x 32 rule against 96 x 96 of the same scheme, CASES x energies x both structures, L = 11:
    1.700e-11 absolute on rows of total mass 1 (the 5-group structure, whose lowest group starts at 0;
    1.7e-14 on the 70-group structure)
  96 x 96 against the CM-cosine form at 64 x 64: 1.652e-10 (the CM form converges algebraically)
  sum over the groups of P0 - 1, edges that cover the lab window: 8.8e-15 at most."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
import nbody_ref
from conftest import dp, ip
from nbody_ref import nbody_cm_check, nbody_converged, nbody_numpy, threshold

ROOT = Path(__file__).resolve().parent.parent
CASES = [(3, 1.9968, -2.2246, 2.9986), (4, 8.9, -1.6, 4.0), (5, 11.9, -7.0, 5.0), (3, 236.0, -6.2, 3.0)]
B5 = np.array([0.0, 1e-3, 0.1, 1.0, 5.0, 20.0])
B70 = np.concatenate([[0.0], np.geomspace(1e-11, 20.0, 70)])
L = 11


def energies(A, Q):
    thr = threshold(A, Q)
    return np.array([e for e in (thr * (1.0 + 1e-6), 6.0, 14.0, 19.9) if e > thr])


@pytest.fixture(scope="module")
def rows(hip):
    """the three restatements on every case and both structures, computed once"""
    out = {}
    for case in CASES:
        n, A, Q, Ap = case
        for name, bins in (("b5", B5), ("b70", B70)):
            E = energies(A, Q)
            out[case, name] = (nbody_numpy(A, Q, n, Ap, E, bins, L)[0], nbody_converged(A, Q, n, Ap, E, bins, L),
                               nbody_cm_check(A, Q, n, Ap, E, bins, L))
    return out


def test_rows_sum_to_one_when_the_edges_cover_the_window(rows):
    worst = max(np.abs(r[0][:, :, 0].sum(axis=1) - 1.0).max() for r in rows.values())
    print(f"sum of P0 - 1: {worst:.3e}")
    assert worst <= 1e-13


def test_top_edge_below_the_lab_maximum_loses_mass(hip):
    n, A, Q, Ap = CASES[0]
    out, st = nbody_numpy(A, Q, n, Ap, [6.0], np.array([0.0, 1e-3]), 3)
    assert 0.0 < out[0, :, 0].sum() < 1.0 and st[0] == 0


def test_large_a_limit(hip):
    A, n, Q, Ap = 1e6, 4, -1.0, 4.0
    bins = np.array([0.0, 0.1, 0.5, 1.0, 2.0, 5.0, 20.0])
    E = np.array([2.0, 10.0])
    out, _ = nbody_numpy(A, Q, n, Ap, E, bins, L)
    cdf = lambda x: 105.0 / 16.0 * (2.0 / 3.0 * x ** 1.5 - 4.0 / 5.0 * x ** 2.5 + 2.0 / 7.0 * x ** 3.5)
    d_mass = d_l = 0.0
    for e, En in enumerate(E):
        Emax = (Ap - 1.0) / Ap * (A / (A + 1.0) * En + Q)
        mass = np.diff(cdf(np.clip(bins / Emax, 0.0, 1.0)))
        d_mass = max(d_mass, np.abs(out[e, :, 0] - mass).max())
        nz = out[e, :, 0] > 0.0
        d_l = max(d_l, np.abs(out[e, nz, 1:] / out[e, nz, :1]).max())
    print(f"large A: masses {d_mass:.3e}, |P_l / P0| {d_l:.3e}")
    assert d_mass <= 1.285e-10 and d_l <= 8.807e-05


def test_rule_against_the_finer_rule_and_the_cm_form(rows):
    d_conv = max(np.abs(a - b).max() for a, b, _ in rows.values())
    d_cm = max(np.abs(b - c).max() for _, b, c in rows.values())
    d70 = max(np.abs(a - b).max() for (case, name), (a, b, _) in rows.items() if name == "b70")
    print(f"32 x 32 against 96 x 96: {d_conv:.3e} (70 groups: {d70:.3e}); 96 x 96 against the CM form: {d_cm:.3e}")
    assert d_conv <= 1.700e-10 and d_cm <= 1.652e-09


def test_constants_of_the_rule(hip):
    x, w = hip.nbody_rule()
    xn, wn = np.polynomial.legendre.leggauss(32)
    assert np.abs(x - xn).max() < 5e-16 and np.abs(w - wn).max() < 5e-15
    assert np.array_equal(x, -x[::-1]) and np.array_equal(w, w[::-1]) and (np.diff(x) > 0).all()
    for n, k in ((3, 16.0 / np.pi), (4, 105.0 / 8.0), (5, 512.0 / (7.0 * np.pi))):       # (a last bit: pi is rounded)
        assert abs(nbody_ref.TWO_OVER_B[n] - k) <= np.spacing(k)


def _args(hip, **kw):
    v = dict(awr=1.9968, Q=-2.2246, n=3, Ap=2.9986, n_ein=2, G=2, order=4, mu_bins=65)
    v.update(kw)
    p = hip.Params.default(v["order"], v["mu_bins"])
    ein, bins = np.array([6.0, 14.0]), np.array([0.0, 1.0, 20.0])
    out, st = np.zeros(2 * 2 * 11), np.zeros(2, np.int32)
    hold = (p, ein, bins, out, st)
    return hold, [C.byref(p), v["awr"], v["Q"], v["n"], v["Ap"], v["n_ein"], dp(ein), v["G"], dp(bins), dp(out), ip(st)]


BAD = [dict(n=2), dict(n=6), dict(Ap=1.0), dict(Ap=0.5), dict(Ap=float("nan")), dict(Ap=float("inf")), dict(awr=0.0),
       dict(awr=-1.0), dict(awr=float("nan")), dict(Q=float("nan")), dict(Q=float("inf")), dict(n_ein=-1),
       dict(G=0), dict(order=0), dict(order=12), dict(mu_bins=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_entry_refuses_before_the_device(hip, bad):
    lib = hip.load()
    hold, args = _args(hip, **bad)
    assert lib.ndpp_nbody_leg_batch(*args) == -22
    assert lib.ndpp_last_error()
    del hold


def test_entry_null_arguments_and_the_empty_call(hip):
    lib = hip.load()
    hold, args = _args(hip)
    for at in (0, 6, 8, 9):                                  # params, ein, e_bins, out
        a = list(args)
        a[at] = None
        assert lib.ndpp_nbody_leg_batch(*a) == -22
    a = list(args)
    a[10] = None                                             # status may be NULL: not an argument error
    if lib.ndpp_device_count() == 0:
        assert lib.ndpp_nbody_leg_batch(*a) == -5
        assert lib.ndpp_nbody_leg_batch(*args) == -5
        assert b"no HIP device" in lib.ndpp_last_error()
    hold0, empty = _args(hip, n_ein=0)
    assert lib.ndpp_nbody_leg_batch(*empty) == 0             # nothing to do needs no device
    del hold, hold0


def test_option_round_trip(hip):
    assert hip.get_nbody() is False                          # the default
    assert hip.set_nbody(True) is False and hip.get_nbody() is True
    assert hip.set_nbody(True) is True
    assert hip.set_nbody(False) is True and hip.get_nbody() is False
    lib = hip.load()
    assert lib.ndpp_set_nbody(7) == 0 and lib.ndpp_get_nbody() == 1 and lib.ndpp_set_nbody(0) == 1


def test_law_66_reads_back_from_an_ace_table(tmp_path):
    from ndpp_amd import ace
    nuc = ace_synth.quantise(nbody_ref.nbody_nuclide())
    f = tmp_path / "synth.ace"
    ace_synth.write_ace(f, "1002.80c", nuc, zaid=1002)
    d = ace.neutron(ace.read_table(f, 1, expect_name="1002.80c"))
    r16 = [r for r in d["reactions"] if r["MT"] == 16]
    assert len(r16) == 1 and r16[0]["mult"] == 2 and r16[0]["thr"] == 19
    (ed,) = r16[0]["edists"]
    assert ed["law"] == 66 and np.array_equal(ed["data"], [3.0, 2.9986])
    assert np.array_equal(ed["pv_y"], [1.0, 0.8])


def test_run_refuses_law_66_in_a_tabular_run(tmp_path):
    nuc = ace_synth.quantise(nbody_ref.nbody_nuclide())
    run = tmp_path / "run"
    ace_synth.write_inputs(run, "1002.80c", nuc, scatt_order=4, mu_bins=nuc["mu_bins"], threads=1)
    xml = run / "ndpp.xml"
    xml.write_text(xml.read_text().replace("<scatt_type>legendre</scatt_type>", "<scatt_type>tabular</scatt_type>"))
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), "--nbody"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 2 and "law 66" in r.stderr and "input error" in r.stderr
    assert not list(run.glob("*.g5")) and not (run / "ndpp_lib.xml").exists()
