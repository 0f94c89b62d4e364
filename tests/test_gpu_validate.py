"""Library validation on the GPU (ndpp_scatt_positivity, ndpp_expand_moments, ndpp_amd.validate)
against the independent numpy/scipy restatement of tests/test_validate.py.

Values are compared to |Δ| <= 1e-13 Σ_l (l+½)|a_l| per row; offending lists, row counts and
(min_ein, min_group) exactly."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.special import eval_legendre

from synth import nuclide_case
from test_validate import hand_sections, np_expand, np_positivity

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
E2E = ROOT / "tests" / "golden" / "e2e"
TOL = 1e-13

# the reference executable's tables (tests/golden/e2e): section -> negative rows at M = 21 / 201 / 2001
# and the band rows (first..last group with P0 > 0) + all-zero E_in rows
GOLDEN_TABLE = {
    ("92238.71c.g2", "elastic"): ((2, 2, 2), 151, 0),
    ("92238.71c.g2", "inelastic"): ((0, 0, 0), 161, 1),
    ("92238.71c.g2", "nuinelastic"): ((0, 0, 0), 161, 1),
    ("chi_sab/94239.71c.g7", "elastic"): ((0, 0, 0), 62, 0),
    ("chi_sab/hh2o.10t.g7", "elastic"): ((193, 194, 194), 415, 2),
    ("chi_sab/grph.10t.g7", "elastic"): ((364, 364, 364), 364, 0),
    ("chi_sab/be.10t.g7", "elastic"): ((302, 302, 302), 308, 0),
}


def read(path):
    from ndpp_amd import reader
    return reader.read_binary((E2E / path).read_bytes())


def check_section(hip, mat, M, nm=None, cap=None):
    """kernel vs restatement on one section; returns (summary, numpy result)"""
    s, rows, rmin, rmu = hip.scatt_positivity(mat, n_moments=nm, mu_points=M, cap=cap)
    ref = np_positivity(mat, M, nm)
    assert s.rows == ref["rows"] and s.negative == len(ref["negative"])
    k = len(rows)
    assert [tuple(r) for r in rows.tolist()] == ref["negative"][:k]
    assert (s.min_ein, s.min_group) == ref["min_row"]
    scale_min = ref["all_scale"][(ref["all_rows"] == ref["min_row"]).all(axis=1)]
    assert abs(s.min_value - ref["min_value"]) <= TOL * max(scale_min.max(initial=0.0), 1e-300) or \
        s.min_value == ref["min_value"]
    fin = ~np.isnan(ref["row_min"][:k])
    assert np.array_equal(np.isnan(rmin), ~fin)
    assert (np.abs(rmin[fin] - ref["row_min"][:k][fin]) <= TOL * ref["scale"][:k][fin]).all()
    # the mu index is where this row's own minimum lies
    if k:
        ie, g = rows[:, 0], rows[:, 1]
        nmom = mat.shape[2] if nm is None else nm
        mu = np.linspace(-1, 1, M)
        at = np.array([(l + 0.5) * eval_legendre(l, mu[rmu]) for l in range(nmom)]).T
        f_at = (mat[ie, g, :nmom] * at).sum(axis=1)
        ok = fin & (np.abs(f_at - rmin) <= 1e-12 * np.maximum(ref["scale"][:k], 1e-300))
        assert ok[fin].all()
    return s, ref


@pytest.mark.parametrize("key", list(GOLDEN_TABLE), ids=lambda k: f"{k[0]}:{k[1]}")
def test_golden_tables(hip, key):
    path, sec = key
    negs, band_rows, zero_rows = GOLDEN_TABLE[key]
    mat = getattr(read(path), sec).mat
    for M, n_neg in zip((21, 201, 2001), negs):
        for nm in (None, 3):
            s, ref = check_section(hip, mat, M, nm)
            assert s.rows == band_rows + zero_rows
            if nm is None:
                assert s.negative == n_neg, (M, s.negative)
            print(f"{path} {sec} M={M} n_mom={nm or mat.shape[2]}: rows {s.rows} negative {s.negative} "
                  f"min {s.min_value:.6g} at ({s.min_ein}, {s.min_group})")
    if sec == "inelastic":          # the all-zero E_in
        s, _, _, _ = hip.scatt_positivity(mat)
        assert s.min_value == 0.0 and s.min_group == -1


@pytest.mark.parametrize("M", [21, 201, 2001])
def test_expand_vs_scipy(hip, M):
    rng = np.random.default_rng(M)
    t = read("chi_sab/hh2o.10t.g7")
    golden = t.elastic.mat.reshape(-1, t.moments)
    golden = golden[golden[:, 0] != 0.0]
    for L in range(1, 12):
        for mom in (rng.standard_normal((300, L)) / (np.arange(L) + 1.0), golden[:, :min(L, golden.shape[1])]):
            f, mu = hip.expand_moments(mom, mu_points=M)
            assert np.array_equal(mu, np.linspace(-1, 1, M)) and f.shape == (len(mom), M)
            scale = (np.abs(mom) * (np.arange(mom.shape[1]) + 0.5)).sum(axis=1)
            assert (np.abs(f - np_expand(mom, M)) <= TOL * scale[:, None]).all(), L
            if L > 2:
                f3, _ = hip.expand_moments(mom, n_moments=2, mu_points=M)
                s2 = (np.abs(mom[:, :2]) * [0.5, 1.5]).sum(axis=1)
                assert (np.abs(f3 - np_expand(mom, M, 2)) <= TOL * s2[:, None]).all()


def test_expand_and_positivity_agree_bitwise(hip):
    """one operation sequence: a row's minimum from positivity is the minimum of its expansion"""
    mat = read("chi_sab/be.10t.g7").elastic.mat
    s, rows, rmin, rmu = hip.scatt_positivity(mat, mu_points=2001)
    f, _ = hip.expand_moments(mat[rows[:, 0], rows[:, 1]], mu_points=2001)
    assert np.array_equal(f.min(axis=1), rmin) and np.array_equal(f.argmin(axis=1), rmu)


@pytest.mark.parametrize("case", list(hand_sections()), ids=lambda c: c[0])
def test_hand_sections(hip, case):
    name, mat, M, exp = case
    s, rows, rmin, rmu = hip.scatt_positivity(mat, mu_points=M)
    assert s.rows == exp["rows"] and [tuple(r) for r in rows.tolist()] == exp["negative"]
    assert (s.min_ein, s.min_group) == exp["min_row"] and abs(s.min_value - exp["min_value"]) < 1e-15
    check_section(hip, mat, M)


def test_planted_rows(hip):
    rng = np.random.default_rng(11)
    NE, G, L = 300, 5, 6
    mat = np.zeros((NE, G, L))
    mat[:, :, 0] = rng.uniform(1.0, 2.0, (NE, G))
    mat[:, :, 1:] = rng.uniform(-0.02, 0.02, (NE, G, L - 1))     # all rows safely positive
    mat[17, 2, 3] = np.nan                                        # NaN: negative
    mat[40] = 0.0                                                 # an all-zero E_in
    # negative only between the points of the 21-point grid: f of (1, 0, 0, 0, 0.09, -0.16) has its
    # minimum -0.0099 between two of them, while the 21 points see no less than +0.0117
    planted = np.array([1.0, 0.0, 0.0, 0.0, 0.09, -0.16])
    mu21, mu2001 = np.linspace(-1, 1, 21), np.linspace(-1, 1, 2001)
    f = lambda mu: sum((l + 0.5) * eval_legendre(l, mu) * planted[l] for l in range(L))
    assert f(mu21).min() > 0.01 and f(mu2001).min() < -0.009
    mat[123, 1] = planted
    s21, rows21, _, _ = hip.scatt_positivity(mat, mu_points=21)
    s2001, rows2001, min2001, _ = hip.scatt_positivity(mat, mu_points=2001)
    assert [tuple(r) for r in rows21.tolist()] == [(17, 2)]
    assert [tuple(r) for r in rows2001.tolist()] == [(17, 2), (123, 1)]
    assert np.isnan(min2001[0]) and abs(min2001[1] - f(mu2001).min()) < 1e-13 * 3
    assert s21.rows == s2001.rows == NE * G - G + 1
    check_section(hip, mat, 21)
    check_section(hip, mat, 2001)
    # more offenders than cap: the first cap in (iE, g) order, the count in full
    bad = mat.copy()
    bad[::3, :, 1] = 2.0                     # 100 E_in x 5 groups negative (E_in 123 among them), + the NaN row
    s, rows, rmin, rmu = hip.scatt_positivity(bad, mu_points=21, cap=37)
    ref = np_positivity(bad, 21)
    assert s.negative == len(ref["negative"]) == 501 and len(rows) == 37
    assert [tuple(r) for r in rows.tolist()] == ref["negative"][:37]
    s0, rows0, _, _ = hip.scatt_positivity(bad, mu_points=21, cap=0)
    assert s0.negative == s.negative and len(rows0) == 0


def test_random_rows_at_P10(hip):
    """2.4e5 seeded rows, L = 11, M = 2001: the offending list equals numpy's, except rows whose
    numpy minimum lies within the value tolerance of 0 (counted, printed, excluded)."""
    rng = np.random.default_rng(20261015)
    NE, G, L = 24000, 10, 11
    mat = rng.standard_normal((NE, G, L)) * (0.2 / (np.arange(L) + 0.5))     # ~half the rows negative
    mat[:, :, 0] = rng.uniform(0.5, 1.5, (NE, G))
    M = 2001
    s, rows, rmin, rmu = hip.scatt_positivity(mat, mu_points=M)
    ref = np_positivity(mat, M)
    near = np.abs(ref["all_min"]) <= TOL * ref["all_scale"]
    near_rows = {tuple(r) for r in ref["all_rows"][near].tolist()}
    got = [tuple(r) for r in rows.tolist() if tuple(r) not in near_rows]
    want = [r for r in ref["negative"] if r not in near_rows]
    print(f"random rows: {s.rows} checked, {s.negative} negative, {len(near_rows)} within tolerance of 0 excluded")
    assert s.rows == NE * G and 0.2 < s.negative / s.rows < 0.8
    assert got == want
    assert abs(s.negative - len(ref["negative"])) <= len(near_rows)


def test_positivity_block_shapes_agree(hip):
    """a row's result does not depend on where it sits: 1200 seeded rows as 2 E_in of 600 groups (a
    group count above the block size: several passes of one block per E_in) and as 1200 E_in of one
    group (64 E_in per block); P0 > 0 everywhere, so every row is in the band in both shapes"""
    rng = np.random.default_rng(20261019)
    L, M = 11, 21
    flat = rng.standard_normal((1200, L)) * (0.2 / (np.arange(L) + 0.5))     # ~half the rows negative
    flat[:, 0] = rng.uniform(0.5, 1.5, 1200)
    sw, rw, minw, muw = hip.scatt_positivity(flat.reshape(2, 600, L), mu_points=M)
    st, rt, mint, mut = hip.scatt_positivity(flat.reshape(1200, 1, L), mu_points=M)
    print(f"block shapes: {sw.rows} rows, {sw.negative} negative, min {sw.min_value!r}")
    assert sw.rows == st.rows == 1200 and sw.negative == st.negative and 0.2 < sw.negative / 1200 < 0.8
    assert np.float64(sw.min_value).tobytes() == np.float64(st.min_value).tobytes()
    assert (st.min_ein, st.min_group) == (sw.min_ein * 600 + sw.min_group, 0)
    assert (rw[:, 0] * 600 + rw[:, 1]).tolist() == rt[:, 0].tolist() and not rt[:, 1].any()
    assert minw.tobytes() == mint.tobytes() and muw.tobytes() == mut.tobytes()
    # and the list is numpy's, except rows within the value tolerance of 0 (as test_random_rows_at_P10)
    ref = np_positivity(flat.reshape(1200, 1, L), M)
    near = np.abs(ref["all_min"]) <= TOL * ref["all_scale"]
    near_rows = {tuple(r) for r in ref["all_rows"][near].tolist()}
    got = [tuple(r) for r in rt.tolist() if tuple(r) not in near_rows]
    want = [r for r in ref["negative"] if r not in near_rows]
    assert got == want
    assert abs(st.negative - len(ref["negative"])) <= len(near_rows)


def test_repeatable_bits(hip):
    rng = np.random.default_rng(3)
    mat = rng.standard_normal((5000, 7, 11))
    mat[:, :, 0] = np.abs(mat[:, :, 0])
    a = hip.scatt_positivity(mat, mu_points=201)
    b = hip.scatt_positivity(mat, mu_points=201)
    assert bytes(a[0]) == bytes(b[0])
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    f1, _ = hip.expand_moments(mat[:, 3], mu_points=2001)
    f2, _ = hip.expand_moments(mat[:, 3], mu_points=2001)
    assert f1.tobytes() == f2.tobytes()


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
    for M in (21, 2001):
        a, b = validate.positivity(fin, mu_points=M), validate.positivity(t, mu_points=M)
        assert a.as_dict() == b.as_dict()
        assert set(a.sections) == {"elastic", "inelastic", "nuinelastic"}
        print(f"8016-like M={M}: " + ", ".join(f"{k} {v.rows} rows {v.negative} negative"
                                                for k, v in a.sections.items()))


def _cli(*args, cwd=ROOT):
    return subprocess.run([sys.executable, "-m", "ndpp_amd.validate", *map(str, args)], cwd=cwd,
                          capture_output=True, text=True, timeout=240)


def test_cli(hip, tmp_path):
    from ndpp_amd import validate
    r = _cli(E2E / "chi_sab", "--json", tmp_path / "rep.json")
    print(r.stdout)
    assert r.returncode == 1, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("4 tables, 3 with negative rows")
    for name in ("hh2o.10t", "grph.10t", "be.10t"):
        assert name in last
    assert "94239.71c" not in last
    rep = json.loads((tmp_path / "rep.json").read_text())
    assert rep["positive"] is False and set(rep["tables"]) == {"94239.71c", "hh2o.10t", "grph.10t", "be.10t"}
    for name, path in (("hh2o.10t", "hh2o.10t.g7"), ("94239.71c", "94239.71c.g7")):
        want = validate.positivity(read(f"chi_sab/{path}"), mu_points=21).as_dict()
        got = dict(rep["tables"][name])
        assert got.pop("path") == path
        assert json.loads(json.dumps(want)) == got
    assert rep["tables"]["hh2o.10t"]["sections"]["elastic"]["negative"] == 193
    # a copy listing only the positive table
    d = tmp_path / "pu"
    d.mkdir()
    shutil.copy(E2E / "chi_sab" / "94239.71c.g7", d)
    xml = (E2E / "chi_sab" / "ndpp_lib.xml").read_text().splitlines()
    keep = [ln for ln in xml if "<ndpp_table" not in ln or 'path="94239.71c.g7"' in ln]
    (d / "ndpp_lib.xml").write_text("\n".join(keep).replace("<entries> 4", "<entries> 1") + "\n")
    r = _cli(d, "--mu-points", 201, "--moments", 3)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "94239.71c: positive" in r.stdout and "1 tables, 0 with negative rows" in r.stdout
