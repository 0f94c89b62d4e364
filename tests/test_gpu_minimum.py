"""Certified positivity on the GPU (ndpp_scatt_minimum, ndpp_amd.validate.minimum, --certified)
against validate.minimum_reference: the real roots of f' with both ends, evaluated by legval.

Reference tolerance: 1e-13 S per row, S = sum (l + 1/2)|a_l| -- legval at degree <= 10 rounds to
about 2e-15 S, and the error of a root of f' enters the minimum only quadratically.  E = 256 eps S
is the entry point's own evaluation allowance (include/ndpp_hip.h)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb
from numpy.polynomial import legendre as leg
from numpy.polynomial import polynomial as poly

from synth import nuclide_case
from test_minimum import PLANTED

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-13
EPS = np.finfo(np.float64).eps


def moments_of(power_coeffs):
    """stored moments a_l of the polynomial sum_k p_k mu^k: c = poly2leg(p), a_l = c_l / (l + 1/2)"""
    c = leg.poly2leg(np.asarray(power_coeffs, dtype=np.float64))
    return c / (np.arange(len(c)) + 0.5)


def scale(rows, nm=None):
    rows = np.asarray(rows, dtype=np.float64)
    nm = rows.shape[-1] if nm is None else nm
    return (np.abs(rows[..., :nm]) * (np.arange(nm) + 0.5)).sum(axis=-1)


def m2_of(rows):
    l = np.arange(rows.shape[-1], dtype=np.float64)
    return (np.abs(rows) * (l + 0.5) * (l - 1) * l * (l + 1) * (l + 2) / 8.0)[..., 2:].sum(axis=-1)


def f_at(row, mu, nm=None):
    nm = len(row) if nm is None else nm
    return float(leg.legval(mu, (np.arange(nm) + 0.5) * np.asarray(row)[:nm]))


@pytest.fixture(scope="module")
def p10():
    """64 E_in x 7 groups x 11 moments, every P0 > 0, moments decaying like exp(-0.3 l); with the
    reference minimum of every row (computed once, read only)."""
    from ndpp_amd import validate
    rng = np.random.default_rng(20251018)
    mat = rng.standard_normal((64, 7, 11)) * np.exp(-0.3 * np.arange(11)) * rng.choice([0.05, 0.15, 0.5], (64, 7, 1))
    mat[:, :, 0] = np.abs(rng.standard_normal((64, 7))) + 0.05       # (a mix of positive and negative rows)
    ref = np.array([[validate.minimum_reference(r)[0] for r in e] for e in mat])
    mat.setflags(write=False)
    ref.setflags(write=False)
    return mat, ref, scale(mat)


def check_enclosure(mat, ref, lo, hi, mu_at, cls, nm=None):
    """every examined finite row: lo - tol <= ref <= hi + tol and hi = f(mu_at) to tol (an all-zero
    E_in is no polynomial's row: its lo = hi = 0 is asserted where it occurs)"""
    S = scale(mat, nm)
    t = TOL * S
    ex = (cls >= 0) & ((cls & 3) != 3) & (mat[:, :, 0] > 0).any(axis=1)[:, None]
    assert (lo[ex] - t[ex] <= ref[ex]).all() and (ref[ex] <= hi[ex] + t[ex]).all()
    assert (np.abs(mu_at[ex]) <= 1.0).all()
    for i, g in np.argwhere(ex):
        assert abs(f_at(mat[i, g], mu_at[i, g], nm) - hi[i, g]) <= t[i, g], (i, g)


def planted_section():
    """3 x 4 x 3: the planted dip at (1, 2) among rows that are positive everywhere"""
    m = np.zeros((3, 4, 3))
    m[0, 1] = [1.0, 0.1, 0.0]
    m[0, 2] = [0.5, 0.0, 0.05]
    m[1, 0] = [0.3, 0.05, 0.0]
    m[1, 2] = PLANTED
    m[1, 3] = [2.0, -0.2, 0.1]
    m[2, 3] = [1.0, 0.0, 0.0]
    return m


def test_planted_dip(hip):
    from ndpp_amd import validate
    m = planted_section()
    sampled = validate.positivity(m, mu_points=21)
    assert sampled.positive and sampled.sections["section"].rows == 2 + 4 + 1
    rep = validate.minimum(m)
    s = rep.sections["section"]
    print(f"planted: hi {s.offending_hi} at mu {s.offending_mu}")
    assert not rep.positive and (s.rows, s.negative, s.nonfinite, s.unsettled) == (7, 1, 0, 0)
    assert s.offending == [(1, 2)] and (s.min_ein, s.min_group) == (1, 2)
    assert s.offending_hi[0] <= -1e-4 * (1 - 1e-6) and abs(s.offending_mu[0] - 0.05) <= 1e-3
    assert s.min_hi == s.offending_hi[0] and s.min_mu == s.offending_mu[0]


def test_enclosure_at_P10(hip, p10):
    mat, ref, S = p10
    s, lo, hi, mu_at, cls, evals = hip.scatt_minimum(mat, want_evals=True)
    print(f"P10: evaluations per row mean {evals.mean():.1f} max {evals.max()}; classes "
          f"{np.bincount((cls & 3).ravel(), minlength=4).tolist()}; widest (hi - lo) / S {((hi - lo) / S).max():.3e}")
    assert s.rows == 64 * 7 and (cls >= 0).all()
    check_enclosure(mat, ref, lo, hi, mu_at, cls)
    E = 256 * EPS * S
    assert (hi - lo <= 1e-10 * S + E + TOL * S).all()
    assert s.unsettled == 0 and not (cls & hip.MIN_UNSETTLED).any()
    assert (evals >= 130).all() and evals.max() <= hip.MIN_MAX_EVALS
    # the summary is the fold of the arrays in (iE, g) order
    kind = cls & 3
    assert (s.negative, s.undecided, s.nonfinite) == ((kind == 2).sum(), (kind == 1).sum(), 0)
    k = np.unravel_index(np.argmin(hi), hi.shape)
    assert (s.min_ein, s.min_group) == k and s.min_hi == hi[k] and s.min_mu == mu_at[k]
    assert ((kind == 0) == (lo >= 0)).all() and ((kind == 2) == (hi < 0)).all()


def hand_section():
    L = 11
    row = lambda a: np.pad(np.asarray(a, dtype=np.float64), (0, L - len(a)))
    m = np.zeros((4, 4, L))
    m[0, 0] = row([3.0])                                              # constant 1.5
    m[0, 1] = row([2.0, 2.0 / 3.0])                                   # 1 + mu: 0 at mu = -1
    m[0, 2] = row(moments_of(poly.polyadd(poly.polypow([-0.3, 1.0], 4), [1e-6])))   # (mu - 0.3)^4 + 1e-6
    m[0, 3] = row(moments_of(cheb.cheb2poly([1.001] + [0.0] * 9 + [1.0])))          # T10 + 1.001: ten minima of 0.001
    m[1, 0] = row([1.0])
    m[1, 1] = row([1.0, 0.0, 0.0, np.nan])                            # a NaN moment
    m[1, 2] = row([0.0, 0.1])                                         # interior row with P0 <= 0: 0.15 mu
    m[1, 3] = row([1.0])
    m[2, 0] = row([-0.5, 0.1])                                        # E_in 2: no P0 > 0 anywhere
    m[2, 3] = row([0.0, 5.0])
    m[3, 1] = row([1.0, 0.1])                                         # E_in 3: band 1..2
    m[3, 2] = row([0.5, -0.1])
    m[3, 3] = row([0.0, 7.0])                                         # outside the band
    return m


def test_hand_rows(hip):
    from ndpp_amd import validate
    m = hand_section()
    s, lo, hi, mu_at, cls = hip.scatt_minimum(m)
    kind = cls & 3
    # who is examined: 4 + 4 + the zero row + 2
    assert s.rows == 11 and (cls[2] == [0, -1, -1, -1]).all() and (cls[3] == [-1, 0, 0, -1]).all()
    out = cls < 0
    assert not lo[out].any() and not hi[out].any() and not mu_at[out].any()
    assert (lo[2, 0], hi[2, 0], mu_at[2, 0]) == (0.0, 0.0, 0.0)
    # constant: settled at once, positive
    assert cls[0, 0] == 0 and hi[0, 0] == 1.5 and 1.5 - 256 * EPS * 1.5 <= lo[0, 0] <= 1.5
    # 1 + mu: never negative
    assert kind[0, 1] != 2 and hi[0, 1] >= 0.0 and mu_at[0, 1] == -1.0 and not cls[0, 1] & 4
    # the flat quartic and the Chebyshev-like row: positive, settled
    assert cls[0, 2] == 0 and cls[0, 3] == 0
    assert 0.0 <= lo[0, 2] <= 1e-6 * (1 + 1e-9) and abs(mu_at[0, 2] - 0.3) < 1e-2
    ref = np.zeros(m.shape[:2])
    for i, g in np.argwhere((cls >= 0) & (kind != 3)):
        ref[i, g] = validate.minimum_reference(m[i, g])[0]
    ref[2] = 0.0
    check_enclosure(m, ref, lo, hi, mu_at, cls)
    S = scale(m)
    fin = (cls >= 0) & (kind != 3)
    assert (hi - lo)[fin].max() >= 0 and ((hi - lo)[fin] <= (1e-10 + 256 * EPS + TOL) * S[fin]).all()
    # the NaN row: class 3, NaN enclosure, counted
    assert cls[1, 1] == 3 and np.isnan(lo[1, 1]) and np.isnan(hi[1, 1]) and s.nonfinite == 1
    # the interior P0 <= 0 row is examined: -0.15 at mu = -1, the section's only negative row
    assert cls[1, 2] == 2 and hi[1, 2] == -(1.5 * 0.1) and mu_at[1, 2] == -1.0
    assert (s.negative, s.unsettled) == (1, 0) and (s.min_ein, s.min_group, s.min_hi, s.min_mu) == (1, 2, hi[1, 2], -1.0)
    rep = validate.minimum(m).sections["section"]
    assert rep.offending == [(1, 1), (1, 2)] and np.isnan(rep.offending_hi[0]) and not rep.positive


def test_all_zero_section_names_group_minus_one(hip):
    s, lo, hi, mu_at, cls = hip.scatt_minimum(np.zeros((3, 5, 3)))
    assert (s.rows, s.negative, s.undecided, s.min_hi, s.min_ein, s.min_group) == (3, 0, 0, 0.0, 0, -1)
    assert (cls[:, 0] == 0).all() and (cls[:, 1:] == -1).all() and not lo.any() and not hi.any()


def test_single_moment_and_truncation(hip, p10):
    # L = 1: f = a_0 / 2
    m = np.array([[[2.0], [0.0], [4.0]], [[0.0], [1.0], [0.0]]])
    s, lo, hi, mu_at, cls = hip.scatt_minimum(m)
    assert s.rows == 4 and (cls == [[0, 0, 0], [-1, 0, -1]]).all()
    assert (hi == [[1.0, 0.0, 2.0], [0.0, 0.5, 0.0]]).all() and (lo <= hi).all()
    # n_moments < L is the call on the cut matrix, bit for bit
    mat = p10[0]
    for nm in (1, 2, 4, 7):
        a = hip.scatt_minimum(mat[:16], n_moments=nm)
        b = hip.scatt_minimum(np.ascontiguousarray(mat[:16, :, :nm]))
        assert bytes(a[0]) == bytes(b[0]), nm
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes(), nm


def test_block_shapes_agree(hip, p10):
    """a row's result does not depend on where it sits: several blocks with a partial last one (7 groups:
    64 E_in per block), and a group count above the block size (several passes of one block)"""
    mat = p10[0]
    base = hip.scatt_minimum(mat)
    many = hip.scatt_minimum(np.concatenate([mat, mat, mat[:2]]))
    assert many[0].rows == 130 * 7
    for x, y in zip(base[1:], many[1:]):
        assert x.tobytes() == y[:64].tobytes() == y[64:128].tobytes() and x[:2].tobytes() == y[128:].tobytes()
    rows = np.tile(mat.reshape(-1, 11), (3, 1))[:1200]
    wide = hip.scatt_minimum(rows.reshape(2, 600, 11))
    tall = hip.scatt_minimum(rows.reshape(1200, 1, 11))
    assert wide[0].rows == tall[0].rows == 1200 and wide[0].min_hi == tall[0].min_hi
    for x, y in zip(wide[1:], tall[1:]):
        assert x.tobytes() == y.tobytes()
    assert wide[2].ravel()[:448].tobytes() == base[2].tobytes()


def test_terminates_at_zero_tolerance(hip, p10):
    mat, ref, S = p10
    s, lo, hi, mu_at, cls, evals = hip.scatt_minimum(mat, rel_tol=0.0, want_evals=True)      # returns: NDPP_OK
    print(f"rel_tol 0: evaluations per row mean {evals.mean():.1f} max {evals.max()}")
    assert evals.max() <= hip.MIN_MAX_EVALS
    assert (m2_of(mat) > 0).all() and (cls & hip.MIN_UNSETTLED).all() and s.unsettled == s.rows == 64 * 7
    check_enclosure(mat, ref, lo, hi, mu_at, cls)
    # M2 = 0 settles at once also at rel_tol = 0
    lin = np.array([[[1.0, 0.2, 0.0], [3.0, 0.0, 0.0]]])
    assert not (hip.scatt_minimum(lin, rel_tol=0.0)[4] & hip.MIN_UNSETTLED).any()


def test_against_expand_moments(hip, p10):
    mat, ref, S = p10
    s, lo, hi, mu_at, cls = hip.scatt_minimum(mat)
    for g in range(mat.shape[1]):
        f, _ = hip.expand_moments(np.ascontiguousarray(mat[:, g]), mu_points=201)
        fmin = f.min(axis=1)
        assert (hi[:, g] <= fmin + TOL * S[:, g]).all() and (lo[:, g] <= fmin).all()


def test_repeatable_bits(hip, p10):
    mat = p10[0]
    a = hip.scatt_minimum(mat, want_evals=True)
    b = hip.scatt_minimum(mat, want_evals=True)
    assert bytes(a[0]) == bytes(b[0])
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_in_memory_result_equals_file(hip):
    """a synthetic nuclide: scatt_nuclide -> finish_scatt, report on the result == report on its file"""
    from ndpp_amd import reader, validate
    c = nuclide_case()
    p = hip.Params.default(c["order"] + 1, c["mu_bins"])
    p.extend_pts, p.inel_extend_pts = c["extend_pts"], c["inel_extend_pts"]
    r = hip.scatt_nuclide(p, c, c["bins"], nuscatt=True)
    o = hip.OutputOptions(hip.FMT_BINARY, 0, c["order"], 1, 0, c["mu_bins"], 1e-10, 1e-3)
    fin, _ = hip.finish_scatt(o, r, c["bins"])
    t = reader.read_binary(hip.nuclide_file(o, "8016.71c  ", 2.53e-8, fin, c["bins"]))
    a, b = validate.minimum(fin), validate.minimum(t)
    assert json.loads(json.dumps(a.as_dict())) == json.loads(json.dumps(b.as_dict()))
    assert set(a.sections) == {"elastic", "inelastic", "nuinelastic"}
    print("8016-like: " + ", ".join(f"{k} {v.rows} rows {v.negative} negative {v.undecided} undecided "
                                    f"{v.unsettled} unsettled" for k, v in a.sections.items()))


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "ndpp_amd.validate", *map(str, args)], cwd=ROOT,
                          capture_output=True, text=True, timeout=240)


def test_cli(hip, tmp_path):
    """a small written library with the planted row: the sampled run passes it, --certified names it"""
    bins = np.array([1e-11, 1e-6, 1e-3, 1.0, 20.0])
    res = dict(ein_el=np.array([1e-9, 1e-4, 2.0]), el_mat=planted_section(), ein_inel=None, inel_mat=None,
               nuinel_mat=None)
    o = hip.OutputOptions(hip.FMT_BINARY, 0, 2, 0, 0, 2001, 1e-8, 0.0)
    (tmp_path / "planted.71c").write_bytes(hip.nuclide_file(o, "%10s" % "1001.71c", 2.53e-8, res, bins))
    (tmp_path / "ndpp_lib.xml").write_bytes(hip.lib_xml(
        str(tmp_path), hip.FMT_BINARY, [dict(alias="H-1.71c", awr=0.999167, name="1001.71c", path="planted.71c",
                                             kT=2.53e-8, zaid=1001, metastable=0, freegas_cutoff=1e-5)],
        bins, 0, 2, 2001, 0, 0, 1e-8, 0.0))
    r = _cli(tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1001.71c: positive" in r.stdout and "1 tables, 0 with negative rows" in r.stdout
    r = _cli(tmp_path, "--certified", "--json", tmp_path / "rep.json")
    print(r.stdout)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "1001.71c: NEGATIVE" in r.stdout and "1 tables, 1 with negative or non-finite rows: 1001.71c" in r.stdout
    line = next(ln for ln in r.stdout.splitlines() if "E_in      2" in ln)
    assert "group    3" in line and "mu =  0.0500" in line and "f = -9.99999" in line
    rep = json.loads((tmp_path / "rep.json").read_text())
    assert rep["certified"] is True and rep["positive"] is False and rep["rel_tol"] == 1e-10
    sec = rep["tables"]["1001.71c"]["sections"]["elastic"]
    assert rep["tables"]["1001.71c"]["certified"] is True
    assert (sec["rows"], sec["negative"], sec["undecided"], sec["nonfinite"], sec["unsettled"]) == (7, 1, 0, 0, 0)
    assert sec["offending"] == [[1, 2]] and (sec["min_ein"], sec["min_group"]) == (1, 2)
    assert sec["offending_hi"][0] <= -1e-4 * (1 - 1e-6) and abs(sec["offending_mu"][0] - 0.05) <= 1e-3
    # a looser tolerance still finds it; undecided and unsettled rows alone do not fail a run
    assert _cli(tmp_path, "--certified", "--rel-tol", 1e-6).returncode == 1
