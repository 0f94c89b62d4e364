"""CPU: error-bounded thinning without a device -- the argument checks of ndpp_thin_segments and
ndpp_thin_bounded (decided before the device is touched), chain() on hand-written segment errors, the
driver's refusals, and the case that shows why the reference's rule is not enough: on a row that bends
slowly in ln E, ndpp_thin_grid leaves dropped points far outside its tolerance, where the chain over
segment_errors_numpy stays within it."""
import math

import numpy as np
import pytest

from conftest import dp, ip
from test_run_inputs import case1, drive, listing, set_tag

INF = float("inf")


def th():
    from ndpp_amd import thin
    return thin


# ---- argument checks of the two entry points (before the device) -------------------------------------
def good_args():
    x = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    y, y2 = np.ones((5, 2, 3)), np.ones((5, 2, 3))
    keep = np.array([4.0])
    seg = np.zeros((5, 3))
    kept, n_kept, max_err = np.zeros(5, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1)
    hold = (x, y, y2, keep, seg, kept, n_kept, max_err)
    # L, G, n, x, y, y2, n_keep, tokeep, window, seg_err
    segs = [3, 2, 5, dp(x), dp(y), dp(y2), 1, dp(keep), 4, dp(seg)]
    # L, G, n, x, y, y2, n_keep, tokeep, tol, window, kept, n_kept, max_err
    bnd = [3, 2, 5, dp(x), dp(y), dp(y2), 1, dp(keep), 1e-3, 4, ip(kept), ip(n_kept), dp(max_err)]
    return hold, segs, bnd


def test_thin_entry_points_refuse_bad_arguments_before_the_device(hip):
    lib = hip.load()
    hold, segs, bnd = good_args()

    def refused(fn, args, pos, value, word):
        a = list(args)
        a[pos] = value
        assert fn(*a) == -22, (fn.__name__, pos, value)
        msg = lib.ndpp_last_error()
        assert word in msg, (pos, value, msg)

    for fn, args, w_pos in ((lib.ndpp_thin_segments, segs, 8), (lib.ndpp_thin_bounded, bnd, 9)):
        for pos, value, word in ((0, 0, b"L="), (0, -1, b"L="), (1, 0, b"G="), (2, 1, b"n="), (2, 0, b"n="),
                                 (w_pos, 1, b"window"), (w_pos, 65, b"window"), (w_pos, 0, b"window"),
                                 (3, None, b"x is NULL"), (4, None, b"y is NULL"), (7, None, b"tokeep"),
                                 (6, -1, b"n_keep"), (0, 40000, b"G * L")):
            if pos == 0 and value == 40000:
                a = list(args)
                a[0] = a[1] = 40000                       # G * L does not fit an index
                assert fn(*a) == -22 and b"G * L" in lib.ndpp_last_error()
                continue
            refused(fn, args, pos, value, word)
        for bad in ([1.0, 2.0, 2.0, 8.0, 16.0], [1.0, 2.0, 1.5, 8.0, 16.0], [0.0, 2.0, 4.0, 8.0, 16.0],
                    [-1.0, 2.0, 4.0, 8.0, 16.0], [1.0, 2.0, np.nan, 8.0, 16.0], [1.0, 2.0, 4.0, 8.0, np.inf]):
            xb = np.array(bad)
            refused(fn, args, 3, dp(xb), b"strictly increasing")
    refused(lib.ndpp_thin_segments, segs, 9, None, b"seg_err")
    for value in (float("nan"), INF, -INF, -1e-3):
        refused(lib.ndpp_thin_bounded, bnd, 8, value, b"tol")
    for pos, word in ((10, b"kept"), (11, b"n_kept"), (12, b"max_err")):
        refused(lib.ndpp_thin_bounded, bnd, pos, None, word)
    # y2 and (with n_keep 0) tokeep may be NULL: a valid call, which without a device is the device error
    if lib.ndpp_device_count() == 0:
        for fn, args in ((lib.ndpp_thin_segments, segs), (lib.ndpp_thin_bounded, bnd)):
            assert fn(*args) == -5
            a = list(args)
            a[5], a[6], a[7] = None, 0, None
            assert fn(*a) == -5
        x, y = hold[0], hold[1]
        with pytest.raises(hip.NdppError) as e:
            hip.thin_segments(x, y, window=4)
        assert e.value.code == -5
        with pytest.raises(hip.NdppError) as e:
            hip.thin_bounded(x, y, tol=1e-3, window=4)
        assert e.value.code == -5
    with pytest.raises(ValueError):
        hip.thin_segments(hold[0][:4], hold[1])
    with pytest.raises(ValueError):
        hip.thin_bounded(hold[0], hold[1], y2=np.ones((5, 2, 2)))


# ---- chain() on hand-written segment errors ---------------------------------------------------------
def seg_of(n, W, fill=INF):
    """seg_err[n][W-1] with the segments that end beyond the grid marked -1 and the rest `fill`"""
    seg = np.full((n, W - 1), fill)
    for a in range(n):
        for d in range(2, W + 1):
            if a + d > n - 1:
                seg[a, d - 2] = -1.0
    return seg


def test_chain_picks_the_largest_admissible_d_where_admissibility_is_not_monotone():
    seg = seg_of(10, 5)
    seg[0] = [5e-4, 2e-3, 9e-4, 3e-3]           # d = 2 and d = 4 admissible, d = 3 and d = 5 not
    seg[4, :4] = [2e-3, 2e-3, 1e-3, 2e-3]       # only d = 4, exactly at tol
    kept, worst = th().chain(seg, 1e-3)
    assert kept.tolist() == [0, 4, 8, 9] and worst == 1e-3
    kept, worst = th().chain(seg, 8e-4)          # now d = 2 from 0; nothing admissible afterwards
    assert kept.tolist() == [0, 2, 3, 4, 5, 6, 7, 8, 9] and worst == 5e-4


def test_chain_never_takes_minus_one_or_infinity_and_ends_at_the_last_point():
    n, W = 7, 4
    seg = seg_of(n, W, fill=0.0)                 # every segment inside the grid is free
    kept, worst = th().chain(seg, 0.0)
    assert kept.tolist() == [0, 4, 6] and worst == 0.0      # from 4 only d = 2 is inside the grid: -1 is never taken
    kept, _ = th().chain(seg, 1e300)
    assert kept.tolist() == [0, 4, 6]
    seg = seg_of(n, W)                           # nothing admissible: every point stays
    kept, worst = th().chain(seg, 1e300)
    assert kept.tolist() == list(range(n)) and worst == 0.0
    seg[2, 1] = 0.25                             # one admissible segment (2, 5)
    kept, worst = th().chain(seg, 0.5)
    assert kept.tolist() == [0, 1, 2, 5, 6] and worst == 0.25
    # n = 2 and n = 3
    assert th().chain(seg_of(2, 4), 1.0)[0].tolist() == [0, 1]
    s3 = seg_of(3, 4)
    assert th().chain(s3, 1.0)[0].tolist() == [0, 1, 2]
    s3[0, 0] = 0.5
    assert th().chain(s3, 1.0) [0].tolist() == [0, 2]
    for tol in (-1.0, float("nan"), INF):
        with pytest.raises(ValueError):
            th().chain(s3, tol)


def same(got, want):
    """equal to a few ulps (-1 and inf exactly): the analytic values assume f = k/d, the log gives it to rounding"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want) & (want >= 0)
    return np.array_equal(got[~fin], want[~fin]) and np.allclose(got[fin], want[fin], rtol=1e-14, atol=1e-15)


def test_segment_errors_numpy_by_hand():
    # x a geometric sequence: f is k/d to rounding (ln 2^k is not k ln 2 to the bit); G = 1, L = 2, P0 = 2 everywhere (the scale), P1 = u^2
    x = 2.0 ** np.arange(6)
    y = np.zeros((6, 1, 2))
    y[:, 0, 0] = 2.0
    y[:, 0, 1] = np.arange(6.0) ** 2
    seg = th().segment_errors_numpy(x, y, window=4)
    assert seg.shape == (6, 3)
    # chord of u^2 over (a, a+d) at a+k: k (d - k); the worst over k: d = 2: 1, d = 3: 2, d = 4: 4; over the scale 2
    assert same(seg[0], [0.5, 1.0, 2.0]) and same(seg[1], [0.5, 1.0, 2.0])
    assert same(seg[2], [0.5, 1.0, -1.0]) and same(seg[3], [0.5, -1.0, -1.0])
    assert same(seg[4], [-1.0] * 3) and same(seg[5], [-1.0] * 3)
    # a must-keep point strictly inside; one at an end does not count
    seg = th().segment_errors_numpy(x, y, tokeep=[4.0], window=4)
    assert same(seg[0], [0.5, INF, INF]) and same(seg[1], [INF, INF, INF])
    assert same(seg[2], [0.5, 1.0, -1.0])
    # y2 on its own scale: the same rows over a scale of 1/4 give 8 times the error
    y2 = y.copy()
    y2[:, 0, 0] = 0.25
    seg2 = th().segment_errors_numpy(x, y, y2, window=4)
    assert same(seg2[0], [4.0, 8.0, 16.0])
    # zero scale -> 0, a NaN -> inf in every segment that holds the row
    z = np.zeros((6, 1, 2))
    z[:, 0, 1] = np.arange(6.0) ** 2
    assert same(th().segment_errors_numpy(x, z, window=3)[0], [0.0, 0.0])
    y[3, 0, 1] = np.nan
    seg = th().segment_errors_numpy(x, y, window=3)
    assert same(seg[:, 0], [0.5, INF, INF, INF, -1.0, -1.0]) and same(seg[:3, 1], [INF, INF, INF])


# ---- the reference's rule is unbounded; the chain is not ------------------------------------------------
def worst_dropped(x, y, kept_x):
    """the largest error, under the scale-relative metric, of a dropped point against the interpolation
    between its two kept neighbours, and the longest run of dropped points"""
    n, G, L = y.shape
    Y = y.reshape(n, -1)
    lx = np.log(x)
    s = np.abs(y[:, :, 0]).max(axis=1)
    idx = np.searchsorted(x, kept_x)
    assert np.array_equal(x[idx], kept_x)
    worst, run = 0.0, 0
    for a, b in zip(idx[:-1], idx[1:]):
        run = max(run, b - a - 1)
        for k in range(a + 1, b):
            f = (lx[k] - lx[a]) / (lx[b] - lx[a])
            d = np.abs(Y[a] + (Y[b] - Y[a]) * f - Y[k]).max()
            worst = max(worst, d / max(s[a], s[k], s[b]))
    return worst, run


def test_the_reference_rule_leaves_dropped_points_outside_its_tolerance_and_the_chain_does_not(hip):
    """G = 1, L = 2, P0 = 1, P1 = 1 + c u^2 / 2 with u = ln x on a uniform grid of spacing h.
    thin_grid tests point k = klo + m against the chord (klo, k + 1): d_local = c m h^2 / 2, over
    y ~ 1..2.  It goes on dropping until m ~ 2 tol y / (c h^2); the point in the middle of that run
    is then d_true = c (m h)^2 / 8 off the chord that finally brackets it: d_true / tol ~ m / 4.
    With tol = 1e-3, h = 1e-3, c = 50: m = 40..80, so d_true should be 10 to 20 times tol.

    Observed: thin_grid keeps 5 of 201 points, its longest run of dropped points is 64, and the worst
    dropped point is 2.64e-2 under the scale-relative metric (26.4 times tol; thin_grid itself reports
    maxerr = 1.0e-3, within tol).  The chain over segment_errors_numpy keeps 18 points, its longest run
    is 11, and its worst dropped point is 9.0e-4."""
    tol, h, c, n = 1e-3, 1e-3, 50.0, 201
    u = h * np.arange(n)
    x = np.exp(u)
    y = np.ones((n, 1, 2))
    y[:, 0, 1] = 1.0 + 0.5 * c * u * u
    xr, yr, comp, maxerr = hip.thin_grid(x, y, np.zeros(0), tol)
    w_ref, run = worst_dropped(x, y, xr)
    print(f"thin_grid: {len(xr)} of {n} kept, longest run {run}, its maxerr {maxerr:.3e}, worst dropped point "
          f"{w_ref:.3e} = {w_ref / tol:.1f} tol")
    assert run >= 20 and len(xr) < n // 10           # it drops runs of tens of points
    assert w_ref > tol
    seg = th().segment_errors_numpy(x, y, window=32)
    kept, worst = th().chain(seg, tol)
    w_new, run_new = worst_dropped(x, y, x[kept])
    print(f"chain: {len(kept)} of {n} kept, longest run {run_new}, max_err {worst:.3e}, worst dropped point {w_new:.3e}")
    assert kept[0] == 0 and kept[-1] == n - 1 and len(kept) < n // 5
    assert w_new <= tol and worst <= tol
    assert math.isclose(w_new, worst, rel_tol=1e-12)  # (np.log against math.log: not the same bits by contract)


# ---- driver ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [
    (("--thin-grid", "0"), "positive"),
    (("--thin-grid=-1e-3",), "positive"),
    (("--thin-grid", "x"), "not a number"),
    (("--thin-grid", "nan"), "positive"),
    (("--thin-grid", "inf"), "positive"),
    (("--thin-grid", "1e-3", "--thin-window", "1"), "--thin-window"),
    (("--thin-grid", "1e-3", "--thin-window", "65"), "--thin-window"),
    (("--thin-window", "16"), "--thin-grid"),
])
def test_bad_thin_flags_exit_2_and_write_nothing(tmp_path, extra, msg):
    r = case1(tmp_path / "run")
    before = listing(r)
    rc, out = drive(r, *extra, "--json", str(tmp_path / "run.json"))
    assert rc == 2 and msg in out, out
    assert listing(r) == before and not (tmp_path / "run.json").exists()


@pytest.mark.parametrize("extra", [("--thin-grid", "1e-3"), ("--thin-grid", "1e-3", "--check-grid")])
def test_tabular_with_thin_grid_exits_2_and_writes_nothing(tmp_path, extra):
    r = case1(tmp_path / "run")
    set_tag(r, "scatt_type", "tabular")
    set_tag(r, "scatt_order", "8")
    before = listing(r)
    rc, out = drive(r, *extra)
    assert rc == 2 and "Legendre output only" in out and "--thin-grid" in out, out
    assert listing(r) == before


def test_thin_results_bookkeeping_with_a_host_thinner():
    """thin_results with chain(segment_errors_numpy) in place of the device: which grids are thinned, what
    is kept, what the report says"""
    thin = th()
    bins = np.array([0.0, 1e-6, 1e-2, 20.0])
    x = np.exp(np.linspace(math.log(1e-9), math.log(20.0), 120))
    x[50], x[70] = 1e-6, 3.0e-4                       # a group edge and the free-gas cutoff, on the grid
    x = np.sort(x)

    def rows(e, scale):
        out = np.ones((len(e), 3, 2)) * scale
        out[:, :, 1] = scale * 0.1 * np.sin(0.3 * np.log(e))[:, None]
        return out

    xin = x[60:]
    thr = float(xin[25])
    data = dict(freegas_cutoff=3.0e-4, energy=np.array([1e-11, thr, 20.0]), reactions=[dict(MT=2, thr=1), dict(MT=51, thr=2)])
    tables = [dict(listing=dict(name="92238.70c"), kind="neutron", data=data),
              dict(listing=dict(name="lwtr.10t"), kind="thermal", data={})]
    res = [dict(ein_el=x, el_mat=rows(x, 1.0), ein_inel=xin, inel_mat=rows(xin, 0.5), nuinel_mat=rows(xin, 0.7)),
           dict(ein_el=x[:5], el_mat=rows(x[:5], 1.0), ein_inel=None, inel_mat=None, nuinel_mat=None)]

    def host(x, y, y2, keep, tol, window):
        return thin.chain(thin.segment_errors_numpy(x, y, y2, keep, window), tol)

    new, rep = thin.thin_results(None, bins, tables, res, True, 1e-3, 16, bounded=host)
    assert new[1] is res[1] and rep[1]["sections"] == {} and rep[1]["note"] == "thermal table: not thinned"
    assert rep[0]["breakpoints"] == [3.0e-4, thr] and "chi" in rep[0]["note"]
    e, i = rep[0]["sections"]["elastic"], rep[0]["sections"]["inelastic"]
    assert e["points_before"] == 120 and e["points_after"] == len(new[0]["ein_el"]) < 120
    assert i["points_before"] == 60 and i["points_after"] == len(new[0]["ein_inel"]) < 60 and i["rides_along"] == "nu-inelastic"
    assert 0.0 < e["max_err"] <= 1e-3 and 0.0 < i["max_err"] <= 1e-3
    for k in (1e-6, 3.0e-4, x[0], x[-1]):
        assert k in new[0]["ein_el"]
    for k in (3.0e-4, thr, xin[0], xin[-1]):
        assert k in new[0]["ein_inel"]
    at = np.searchsorted(x, new[0]["ein_el"])
    assert np.array_equal(new[0]["el_mat"], res[0]["el_mat"][at])
    at = np.searchsorted(xin, new[0]["ein_inel"])
    assert np.array_equal(new[0]["inel_mat"], res[0]["inel_mat"][at]) and np.array_equal(new[0]["nuinel_mat"], res[0]["nuinel_mat"][at])
    lines = thin.format_lines(rep, 1e-3)
    assert len(lines) == 2 and "120 ->" in lines[0] and "not thinned" in lines[1]
    with pytest.raises(ValueError):
        thin.thin_results(None, bins, tables, res, True, 0.0, 16, bounded=host)
