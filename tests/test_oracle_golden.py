"""The C restatement against the committed golden vectors (generated from the
reference Fortran by tests/golden/make_golden.py).  Runs everywhere."""
import ctypes as C

import numpy as np
import pytest

from conftest import dp, ip, load_golden, oracle_params, scale_rel_err
from synth import (FILE4_G, FILE4_KINDS, FILE4_L, FILE4_M, file4_golden_cases, file4_kinematics, mu_grid,
                   same_bits)

# The reference's own known answers that still pin the current API
# (tests/test_scatt/test_scattdata.F90:1650,1687-1692 -- moments of a linear f
# are exact for the tablelin integrals; here we pin calc_pn through them).


def test_scalars(oracle):
    g = load_golden("scalars")
    for n in range(11):
        got = np.array([oracle.oracle_calc_pn(n, x) for x in g["xs"]])
        assert (got == g["pn"][n]).all()
    p = oracle_params(oracle)
    for A, kT, Ein, Eout, lo, hi in g["find_mu"]:
        m = np.zeros(2)
        oracle.oracle_find_fg_mu(C.byref(p), A, kT, Ein, Eout, dp(m))
        assert m[0] == lo and m[1] == hi
    for R, w, u in g["tolab"]:
        assert oracle.oracle_tolab(R, w) == u


def _run_oracle_case(oracle, g, sel):
    L, M = int(g["L"]), int(g["M"])
    p = oracle_params(oracle, L, M)
    bins = np.ascontiguousarray(g["bins"])
    G = len(bins) - 1
    ein = np.ascontiguousarray(g["ein"][sel])
    row = np.ascontiguousarray(g["row_lo"][sel].astype(np.int32))
    w = np.ascontiguousarray(g["w_hi"][sel])
    f_tab = np.ascontiguousarray(g["f_tab"])
    out = np.zeros((len(ein), G, L))
    rc = oracle.oracle_elastic_leg_batch(C.byref(p), float(g["A"]), float(g["kT"]), 1e300, 0.0,
                                         len(ein), dp(ein), ip(row), dp(w), f_tab.shape[0],
                                         dp(f_tab), G, dp(bins), dp(out), 0, None)
    assert rc == 0
    return out


@pytest.mark.parametrize("name,sel", [
    ("freegas_h1_p3", [0, 9, 17, 25, 32, 33]),
    ("freegas_h1_p5", [2, 4]),
    ("freegas_u238_p7_g3", [1]),
    ("freegas_o16_p1_m65", [0, 1, 2]),
])
def test_freegas_golden(oracle, name, sel):
    g = load_golden(name)
    out = _run_oracle_case(oracle, g, sel)
    ref = g["out"][sel]
    # the restatement is bit-compatible with the flang -O0 build
    assert np.array_equal(out, ref), scale_rel_err(out, ref)


def test_file4_golden(oracle):
    g = load_golden("file4_cm")
    M = int(g["M"])
    mu = np.empty(M)
    oracle.oracle_mu_grid(M, dp(mu))
    ob, oo = 0, 0
    for k in range(int(g["n"])):
        nb, L = int(g["nb"][k]), int(g["L"][k])
        bins = np.ascontiguousarray(g["bins"][ob:ob + nb])
        G = nb - 1
        ref = g["out"][oo:oo + G * L].reshape(G, L)
        ob += nb
        oo += G * L
        fw = 0.5 * (1 + g["fa"][k] * mu + g["fb"][k] * (1.5 * mu * mu - 0.5))
        p = oracle_params(oracle, L, M)
        out = np.zeros((G, L))
        oracle.oracle_integrate_file4_cm_leg(C.byref(p), dp(fw), float(g["Ein"][k]), float(g["A"][k]),
                                             float(g["Q"][k]), dp(bins), nb, dp(mu), dp(out))
        assert np.array_equal(out, ref), k


def test_file4_edges_golden(oracle):
    """file4_cm_edges.npz, written by the Fortran: small and odd cosine grids (a bound clamped to +1
    falls in cell M), orders 1..11, 1..300 groups, R < 1, thresholds, Q > 0, rough tables.  The
    oracle bit for bit, and the file holds every value of every axis."""
    g = load_golden("file4_cm_edges")
    seen = dict(M=set(), L=set(), G=set(), kin=set(), kind=set())
    n = 0
    for M, L, G, A, Q, Ein, kind, fw, bins, ref in file4_golden_cases(g):
        mu = mu_grid(M)
        p = oracle_params(oracle, L, M)
        out = np.zeros((G, L))
        oracle.oracle_integrate_file4_cm_leg(C.byref(p), dp(fw), Ein, A, Q, dp(bins), G + 1, dp(mu), dp(out))
        assert same_bits(out, ref), (M, L, G, A, Q, Ein, FILE4_KINDS[kind])   # (the sign of a zero too)
        for key, v in (("M", M), ("L", L), ("G", G), ("kin", (A, Q)), ("kind", kind)):
            seen[key].add(v)
        n += 1
    assert n == int(g["n"])
    assert seen["M"] == set(FILE4_M) and seen["L"] == set(FILE4_L) and seen["G"] >= set(FILE4_G)
    assert seen["kin"] >= set(file4_kinematics()) and seen["kind"] == set(range(len(FILE4_KINDS)))
