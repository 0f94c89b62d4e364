"""GPU: ndpp_thin_segments against its host restatement bit for bit, the guarantee of ndpp_thin_bounded
checked by an independent interpolation between kept neighbours, and the driver's --thin-grid end to end
on the U-238-like run directory."""
import json

import numpy as np
import pytest

from test_gpu_gridcheck import bits, drive, files_of
from test_run_inputs import case1

pytestmark = pytest.mark.gpu
INF = float("inf")


def smooth_rows(rng, n, G, L, noise=1e-3, scale=1.0):
    """x[n] and rows y[n][G][L]: smooth in ln x, plus noise; P0 of the order of `scale`"""
    x = 1e-9 * np.exp(np.cumsum(rng.uniform(0.05, 0.5, n)))
    u = np.log(x)[:, None, None]
    amp = rng.uniform(0.2, 1.0, (1, G, L)) * 10.0 ** rng.integers(-6, 1, (1, G, L))
    y = amp * np.sin(rng.uniform(0.05, 0.4, (1, G, L)) * u + rng.uniform(0, 6, (1, G, L)))
    y[:, :, 0] = np.abs(y[:, :, 0]) + 0.1
    y = scale * y * (1.0 + noise * rng.standard_normal((n, G, L)))
    return x, y


def compare(hip, x, y, y2, keep, W):
    from ndpp_amd import thin
    want = thin.segment_errors_numpy(x, y, y2, keep, W)
    got = hip.thin_segments(x, y, y2, keep, W)
    print(f"n={len(x)} G x L={y.shape[1]}x{y.shape[2]} W={W} y2={'yes' if y2 is not None else 'no'}: "
          f"bit differences {(bits(got) != bits(want)).sum()} of {got.size}, -1: {(got == -1).sum()}, "
          f"inf: {np.isinf(got).sum()}, largest finite {got[np.isfinite(got)].max():.3e}")
    assert got.shape == want.shape == (len(x), W - 1)
    assert np.array_equal(bits(got), bits(want))
    return got


@pytest.mark.parametrize("G,L,n,W,with_y2", [
    (1, 1, 40, 8, False), (2, 6, 40, 8, False), (3, 7, 40, 8, True), (70, 11, 40, 8, True), (70, 11, 40, 8, False),
    (2, 6, 70, 64, True), (3, 7, 5, 16, False)])
def test_gpu_segment_errors_equal_the_host_restatement_bit_for_bit(hip, G, L, n, W, with_y2):
    rng = np.random.default_rng(100 * G + L + n + W)
    x, y = smooth_rows(rng, n, G, L)
    y2 = smooth_rows(rng, n, G, L, scale=3.0)[1] if with_y2 else None
    keep = np.array([0.0, x[n // 2], 1.0])                # one point of the grid, two that are not on it
    got = compare(hip, x, y, y2, keep, W)
    assert (got == -1.0).sum() == sum(1 for a in range(n) for d in range(2, W + 1) if a + d > n - 1)
    inside = [(a, d) for a in range(n) for d in range(2, W + 1) if a + d <= n - 1 and a < n // 2 < a + d]
    assert inside and all(got[a, d - 2] == INF for a, d in inside)
    assert np.isfinite(got[(got >= 0)]).sum() > 0


def test_gpu_segment_errors_edge_cases(hip):
    from ndpp_amd import thin
    rng = np.random.default_rng(7)
    # n = 2 and n = 3
    x, y = smooth_rows(rng, 3, 2, 3)
    got = compare(hip, x[:2], y[:2], None, None, 4)
    assert np.array_equal(got, np.full((2, 3), -1.0))
    got = compare(hip, x, y, None, None, 4)
    assert got[0, 0] >= 0 and (got.ravel()[1:] == -1.0).all()
    idx, worst = hip.thin_bounded(x[:2], y[:2], tol=1e-3, window=4)
    assert idx.tolist() == [0, 1] and worst == 0.0
    idx, worst = hip.thin_bounded(x, y, tol=1e300, window=4)
    assert idx.tolist() == [0, 2] and worst == got[0, 0]
    # a row of NaN, an infinity, an all-zero stretch (scale 0 -> err 0), zero P0 with other moments not zero
    x, y = smooth_rows(rng, 30, 3, 4)
    y[5] = np.nan
    y[12, 1, 2] = np.inf
    y[18:23] = 0.0
    y[25:29, :, 0] = 0.0
    got = compare(hip, x, y, None, None, 6)
    assert (got[0:5, 4] == INF).all() and got[6, 0] >= 0 and got[4, 0] == INF and got[10, 1] == INF
    assert np.array_equal(got[18, :3], [0.0, 0.0, 0.0]) and got[25, 1] == 0.0 and np.isfinite(got[17, 0])
    # y2 is divided by its own scale: the same rows as y2 at a thousandth of the scale give the same errors, to
    # rounding, and y2 with a noise y does not have decides
    x, y = smooth_rows(rng, 30, 2, 5)
    alone = compare(hip, x, y, None, None, 6)
    both = compare(hip, x, y, 1e-3 * y, None, 6)
    ok = alone >= 0
    assert np.allclose(both[ok], alone[ok], rtol=1e-12, atol=0.0)
    noisy = 1e-3 * y * (1.0 + 0.05 * rng.standard_normal(y.shape))
    both = compare(hip, x, y, noisy, None, 6)
    only2 = compare(hip, x, noisy, None, None, 6)
    assert np.array_equal(both[ok], np.maximum(alone[ok], only2[ok])) and (both[ok] > alone[ok]).any()
    # a must-keep point: every segment with it strictly inside, and no other
    got = compare(hip, x, y, None, [x[10]], 6)
    for a in range(30):
        for d in range(2, 7):
            if a + d <= 29:
                assert (got[a, d - 2] == INF) == (a < 10 < a + d), (a, d)
    assert thin.chain(got, 1e300)[0].tolist().count(10) == 1


def dropped_errors(x, y, y2, kept):
    """independent of ndpp_amd.thin: per dropped point the scale-relative error against the interpolation
    between its kept neighbours"""
    lx = np.log(x)
    out = []
    for a, b in zip(kept[:-1], kept[1:]):
        for k in range(a + 1, b):
            f = (lx[k] - lx[a]) / (lx[b] - lx[a])
            e = 0.0
            for m in (y, y2):
                if m is not None:
                    d = np.abs(m[a] + (m[b] - m[a]) * f - m[k]).max()
                    s = max(np.abs(m[i, :, 0]).max() for i in (a, k, b))
                    e = max(e, d / s if s > 0 else 0.0)
            out.append(e)
    return np.array(out)


def test_gpu_thin_bounded_keeps_every_dropped_point_within_tol(hip):
    rng = np.random.default_rng(2024)
    n, G, L, tol = 400, 2, 6, 1e-3
    x = 1e-9 * np.exp(np.cumsum(rng.uniform(0.01, 0.1, n)))
    u = np.log(x)[:, None, None]
    y = rng.uniform(0.2, 1.0, (1, G, L)) * np.sin(rng.uniform(0.05, 0.3, (1, G, L)) * u + rng.uniform(0, 6, (1, G, L)))
    y[:, :, 0] = np.abs(y[:, :, 0]) + 0.5
    y = y * (1.0 + 1e-5 * rng.standard_normal((n, G, L)))
    y2 = 2.0 * y * (1.0 + 1e-5 * rng.standard_normal((n, G, L)))
    keep = np.array([0.0, x[57], x[58], x[200], x[333], 20.0])
    for sec2 in (None, y2):
        kept, max_err = hip.thin_bounded(x, y, sec2, keep, tol, 32)
        errs = dropped_errors(x, y, sec2, kept)
        print(f"thin_bounded n={n}: kept {len(kept)}, max_err {max_err:.6e}, worst dropped point {errs.max():.6e}, "
              f"longest run {np.diff(kept).max() - 1}")
        assert len(kept) < n and len(errs) == n - len(kept) and np.all(np.diff(kept) > 0) and np.diff(kept).max() <= 32
        assert kept[0] == 0 and kept[-1] == n - 1 and np.isin([57, 58, 200, 333], kept).all()
        assert errs.max() <= tol and max_err <= tol
        # np.log here, the C library's log there: the same number to rounding, not to the bit
        assert np.isclose(max_err, errs.max(), rtol=1e-9, atol=0.0)
        assert len(kept) < n // 2                      # and it does thin: the rows are smooth
    # a tolerance of zero keeps everything on rows with noise; the window bounds a run
    kept, max_err = hip.thin_bounded(x, y, None, keep, 0.0, 32)
    assert kept.tolist() == list(range(n)) and max_err == 0.0
    kept, _ = hip.thin_bounded(x, np.ones((n, 1, 1)), None, None, 0.0, 5)
    assert kept.tolist() == list(range(0, n - 1, 5)) + [n - 1]


def test_gpu_thin_grid_end_to_end(hip, tmp_path):
    """case1 (the U-238-like table): --thin-grid 1e-3 writes a library with no more points per section than a
    plain run; the rows it dropped, taken from the raw results before print_tol, are within 1e-3 of the
    interpolation between the kept rows; group edges, cutoff and thresholds survive; and the three grid flags
    run together."""
    from ndpp_amd import gridcheck, reader, run as drv, thin
    plain, thn, all3 = (case1(tmp_path / n) for n in ("plain", "thin", "all"))
    assert drive(plain) == 0
    assert drive(thn, "--thin-grid", "1e-3", "--json", str(tmp_path / "thin.json")) == 0
    t0 = reader.read_binary(next(v for k, v in files_of(plain).items() if k.endswith(".g2")))
    t1 = reader.read_binary(next(v for k, v in files_of(thn).items() if k.endswith(".g2")))
    rep = json.loads((tmp_path / "thin.json").read_text())["grid"]["thin"]
    assert rep["tol"] == 1e-3 and rep["window"] == 32 and len(rep["tables"]) == 1
    secs = rep["tables"][0]["sections"]
    for name, s0, s1 in (("elastic", t0.elastic, t1.elastic), ("inelastic", t0.inelastic, t1.inelastic),
                         ("inelastic", t0.nuinelastic, t1.nuinelastic)):
        print(f"{name}: {len(s0.ein)} -> {len(s1.ein)} E_in, report {secs[name]}")
        assert len(s1.ein) <= len(s0.ein) and np.isin(s1.ein, s0.ein).all() and np.all(np.diff(s1.ein) > 0)
        assert secs[name]["points_before"] == len(s0.ein) and secs[name]["points_after"] == len(s1.ein)
        assert 0.0 <= secs[name]["max_err"] <= 1e-3
    # the raw rows (print_tol renormalises what is written): the same thinning in this process
    s = drv.read_ndpp_xml(thn)
    tables = drv.load_tables(s, drv.read_cross_sections(s["cross_sections"]))
    p, bins = drv.params_of(s), s["energy_bins"]
    res = hip.scatt_library(p, [tables[0]["data"]], bins, s["nuscatter"])
    keep = thin.must_keep(bins, tables[0]["data"])
    assert len(gridcheck.table_breakpoints(tables[0]["data"])) >= 1
    # (a second, looser tolerance: this table's grids are coarse, and the looser one drops more of them)
    for tol, xk, mats in [(t, xk, mats) for t in (1e-3, 5e-2)
                          for xk, mats in (("ein_el", ("el_mat",)), ("ein_inel", ("inel_mat", "nuinel_mat")))]:
        new, _ = thin.thin_results(p, bins, tables, res, s["nuscatter"], tol, 32)
        if tol == 1e-3:
            assert np.array_equal(new[0]["ein_el"], t1.elastic.ein) and np.array_equal(new[0]["ein_inel"], t1.inelastic.ein)
        x = res[0][xk]
        kept = np.searchsorted(x, new[0][xk])
        assert np.array_equal(x[kept], new[0][xk])
        for m in mats:
            assert np.array_equal(bits(new[0][m]), bits(res[0][m][kept]))
        errs = dropped_errors(x, res[0][mats[0]], res[0][mats[1]] if len(mats) > 1 else None, kept)
        print(f"tol {tol:g} {xk}: {len(x)} -> {len(kept)}, worst dropped point {errs.max() if len(errs) else 0.0:.3e}")
        assert len(errs) == len(x) - len(kept) and (len(errs) == 0 or errs.max() <= tol)
        on_grid = keep[np.isin(keep, x)]
        assert (len(on_grid) >= 1 or xk != "ein_el") and np.isin(on_grid, new[0][xk]).all()   # edges, cutoff, thresholds survive
        assert new[0][xk][0] == x[0] and new[0][xk][-1] == x[-1]
    # the three flags together
    assert drive(all3, "--refine-grid", "1e-2", "--thin-grid", "1e-3", "--check-grid", "--json", str(tmp_path / "all.json")) == 0
    g = json.loads((tmp_path / "all.json").read_text())["grid"]
    assert set(g) == {"refine", "thin", "check"}
    t3 = reader.read_binary(next(v for k, v in files_of(all3).items() if k.endswith(".g2")))
    r3, s3 = g["refine"]["tables"][0]["grids"], g["thin"]["tables"][0]["sections"]
    assert s3["elastic"]["points_before"] == r3["elastic"]["points_after"]       # thinning follows refinement
    assert s3["elastic"]["points_after"] == len(t3.elastic.ein) and s3["inelastic"]["points_after"] == len(t3.inelastic.ein)
    c3 = g["check"]["tables"][0]["sections"]
    assert c3["elastic"]["intervals"] == len(t3.elastic.ein) - 2                 # the check saw the thinned grid
