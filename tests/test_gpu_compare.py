"""GPU: ndpp_lib_compare against its host restatement bit for bit at the smallest shapes that can go
wrong, as an independent check of what error-bounded thinning and the grid check
(section 12) report, and end to end: the driver's library against the reference executable's."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from test_compare import golden_dir, random_sections
from test_e2e_reference import CASE, e2e_nuclide

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
INF = float("inf")


def cp():
    from ndpp_amd import compare
    return compare


def same_bits(hip, xa, ya, xb, yb, xq):
    want = cp().compare_numpy(xa, ya, xb, yb, xq)
    got = hip.lib_compare(xa, ya, xb, yb, xq)
    for name, g, w in zip(("err", "arg", "worst"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, g, w)
    return got


def queries(xa, xb, rng, extra=0):
    """the union queries, every point of both grids, and `extra` random energies, some outside"""
    lo, hi = min(xa[0], xb[0]) / 2.0, max(xa[-1], xb[-1]) * 2.0
    return np.concatenate([cp().union_queries(xa, xb), xa, xb, np.exp(rng.uniform(np.log(lo), np.log(hi), extra))])


@pytest.mark.parametrize("na,nb,G,La,Lb", [
    (2, 2, 1, 1, 1),          # the smallest call
    (5, 7, 3, 11, 11),        # G * Lc = 33: fewer elements than a wave
    (5, 7, 7, 11, 11),        # 77: more than a wave, no multiple of 64
    (6, 4, 7, 6, 11),         # two row pitches
    (6, 4, 7, 11, 6),
    (4, 5, 2, 70, 65),        # Lc above 64: a lane's step stays inside one group
])
def test_gpu_lib_compare_equals_the_host_restatement(hip, na, nb, G, La, Lb):
    xa, ya, xb, yb = random_sections(100 + na + G + La, na, nb, G, La, Lb)
    rng = np.random.default_rng(7)
    if na == 2:
        err, arg, worst = same_bits(hip, xa, ya, xa * 1.0, yb, xa[:1])      # nq = 1, on the first point
        assert err[0] >= 0 and arg[0] == 0
        same_bits(hip, xa, ya, xa * 1.0, yb, xa[1:])                        # and on the last
        return
    err, _, _ = same_bits(hip, xa, ya, xb, yb, queries(xa, xb, rng, 40))
    assert (err == -1.0).any() and (err > 0).any()


def test_gpu_more_queries_than_waves_in_a_block(hip):
    xa, ya, xb, yb = random_sections(37, 37, 53, 3, 5, 5)
    rng = np.random.default_rng(8)
    xq = np.exp(rng.uniform(np.log(xa[0] / 1.5), np.log(xb[-1] * 1.5), 1000))
    err, arg, worst = same_bits(hip, xa, ya, xb, yb, xq)
    assert len(err) == 1000 and (err == -1.0).sum() > 10 and (err > 0).sum() > 500
    # worst is the maximum over the queries of the per-query figure, element by element at least at the argument
    live = err >= 0
    assert worst.max() == err[live].max() and worst.ravel()[arg[np.argmax(np.where(live, err, -1.0))]] == err[live].max()


def test_gpu_nan_infinity_zero_scale_and_the_end_points(hip):
    rng = np.random.default_rng(41)
    xa, xb = 2.0 ** np.arange(9), 1.5 * 2.0 ** np.arange(8)          # 1 .. 256 and 1.5 .. 192, interleaved
    ya, yb = rng.normal(size=(9, 7, 11)), rng.normal(size=(8, 7, 11))
    ya[3, 2, 5] = np.nan
    ya[3, 6, 10] = np.inf
    yb[1, 0, 0] = -np.inf
    ya[6:, :, 0] = 0.0                      # from 64 up P0 = 0 in every row involved
    yb[5:, :, 0] = 0.0
    rng = np.random.default_rng(9)
    xq = np.concatenate([queries(xa, xb, rng, 60), [0.0, -1.0, np.nan, np.inf, max(xa[0], xb[0]), min(xa[-1], xb[-1])]])
    err, arg, worst = same_bits(hip, xa, ya, xb, yb, xq)
    assert (err == INF).any() and (err == 0.0).any() and (err == -1.0).any() and err[-2] >= 0 and err[-1] >= 0
    assert worst[2, 5] == INF and worst[6, 10] == INF and worst[0, 0] == INF and np.isfinite(worst[1]).all()
    # every query skipped
    e, a, w = same_bits(hip, xa, ya, xb, yb, np.array([xa[0] / 10.0, np.nan]))
    assert np.array_equal(e, [-1.0, -1.0]) and np.array_equal(w, np.full((7, 11), -1.0))


# ---- section 13: what error-bounded thinning reports, by another code path ----------------------------
def bending_rows():
    """the slowly bending rows of tests/test_thin_bounded.py: G = 1, L = 2, P0 = 1, P1 = 1 + c u^2 / 2,
    u = ln x uniform with spacing h"""
    tol, h, c, n = 1e-3, 1e-3, 50.0, 201
    u = h * np.arange(n)
    y = np.ones((n, 1, 2))
    y[:, 0, 1] = 1.0 + 0.5 * c * u * u
    return tol, np.exp(u), y


def test_gpu_thinned_by_ndpp_thin_bounded_stays_within_the_max_err_it_reported(hip):
    tol, x, y = bending_rows()
    kept, max_err = hip.thin_bounded(x, y, tol=tol, window=32)
    rep = cp().compare_sections((x[kept], y[kept]), (x, y))
    print(f"thin_bounded: {len(kept)} of {len(x)} kept, max_err {max_err!r}; compare(thinned, original) {rep['err']!r} "
          f"at {rep['energy']:.6e} over {rep['queries']} queries")
    assert rep["comparable"] and rep["outside_a"]["points"] == rep["outside_b"]["points"] == 0
    assert 0.0 < rep["err"] <= max_err and rep["err"] <= tol
    assert (rep["group"], rep["moment"]) == (0, 1) and rep["worst"][0, 0] == 0.0


def test_gpu_thinned_by_the_reference_rule_exceeds_its_tolerance(hip):
    """the 26x case tests/test_thin_bounded.py documents: ndpp_thin_grid reports maxerr within tol and leaves
    a dropped point 2.64e-2 from the interpolation between its kept neighbours"""
    tol, x, y = bending_rows()
    xr, yr, comp, maxerr = hip.thin_grid(x, y, np.zeros(0), tol)
    rep = cp().compare_sections((xr, yr), (x, y))
    print(f"thin_grid: {len(xr)} of {len(x)} kept, its maxerr {maxerr:.3e}; compare(thinned, original) {rep['err']:.3e} "
          f"= {rep['err'] / tol:.1f} tol")
    assert maxerr <= tol * (1 + 1e-12) and rep["err"] > 10 * tol


# ---- section 12: the grid check's figure, by another code path -----------------------------------------
def test_gpu_a_refined_grid_against_the_original_is_the_grid_checks_error(hip):
    from ndpp_amd import gridcheck
    xa, ya, _, _ = random_sections(51, 12, 3, 3, 4, 4)
    ya[:, :, 0] = np.abs(ya[:, :, 0]) + 0.5
    xm = gridcheck.midpoints(xa)
    assert ((xm > xa[:-1]) & (xm < xa[1:])).all()
    rng = np.random.default_rng(52)
    f = np.array([np.log(m / a) / np.log(b / a) for m, a, b in zip(xm, xa[:-1], xa[1:])])
    y_mid = ya[:-1] + (ya[1:] - ya[:-1]) * f[:, None, None] + 1e-3 * rng.normal(size=(11, 3, 4))    # a known offset
    err, arg = hip.grid_error(xa, ya, xm, y_mid)
    at = np.arange(1, 12)
    xr, yr = np.insert(xa, at, xm), np.insert(ya, at, y_mid, axis=0)
    e, a, _ = hip.lib_compare(xr, yr, xa, ya, xm)
    assert (err > 1e-5).all() and np.array_equal(e, err) and np.array_equal(a, arg)
    # at the original points the refined grid holds the original rows
    e0, _, _ = hip.lib_compare(xr, yr, xa, ya, xa)
    assert np.array_equal(e0, np.zeros(12))


# ---- end to end ---------------------------------------------------------------------------------------------
def test_gpu_driver_library_against_the_reference_executables(tmp_path, capsys):
    """python -m ndpp_amd.run on the U-238-like case, then compare_dirs(result, golden): every section
    comparable and within 1e-10, the bound tests/test_e2e_reference.py holds for this case (moments
    against the reference executable; the ASCII format's 1PE20.12 rounding alone, applied to the golden
    table on the host, gives 1.9e-12 under this metric and is inside it as well)."""
    run = tmp_path / "run"
    ace_synth.write_inputs(run, CASE["name"], e2e_nuclide(), scatt_order=CASE["scatt_order"], mu_bins=CASE["mu_bins"],
                           extend_pts=CASE["extend_pts"], inel_extend_pts=CASE["inel_extend_pts"], threads=1)
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run)], cwd=ROOT, capture_output=True, text=True, timeout=250)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    gold = golden_dir(tmp_path, "gold")
    c = cp()
    rep = c.compare_dirs(run, gold, 1e-10)
    for line in c.format_lines(rep):
        print(line)
    assert rep["only_in_a"] == rep["only_in_b"] == rep["not_comparable"] == []
    secs = rep["tables"][0]["sections"]
    assert list(secs) == ["elastic", "inelastic", "nu-inelastic"] and all(s["comparable"] for s in secs.values())
    print(f"e2e: worst {rep['err']:.3e} in {rep['at']}")
    assert rep["err"] < 1e-10 and rep["above"] == []
    # the command line on the same two directories
    assert c.main([str(run), str(gold), "--tol", "1e-10", "--json", str(tmp_path / "cmp.json")]) == 0
    assert (tmp_path / "cmp.json").exists() and "92238.71c" in capsys.readouterr().out
