"""CPU: the grid check without a device -- the host restatement of ndpp_grid_error on hand-made
matrices, the refinement loop on an analytic y(E) in place of the integrators, the argument
checks of ndpp_grid_error and ndpp_scatt_library_at (decided before the device is touched), and
the driver's refusals."""
import ctypes as C
import json
import math

import numpy as np
import pytest

from conftest import dp, ip
from test_e2e_reference import write_case2
from test_run_inputs import case1, drive, listing, set_tag


def gc():
    from ndpp_amd import gridcheck
    return gridcheck


# ---- grid_error_numpy -------------------------------------------------------------------------------
def rows_of(fun, x, G=2, L=3):
    """y[n][G][L] with element (g, l) = fun(x) * (g + 1) / (l + 1)"""
    w = (np.arange(G)[:, None] + 1.0) / (np.arange(L)[None, :] + 1.0)
    return fun(np.asarray(x, dtype=np.float64))[:, None, None] * w[None]


def test_linear_in_ln_e_gives_zero_exactly():
    # the values are small integers times powers of two and f = 1/2 exactly (x a geometric sequence of
    # ratio 4, midpoints of ratio 2): every operation of the formula is exact
    x = 4.0 ** np.arange(-6, 6)
    xm = gc().midpoints(x)
    assert np.array_equal(xm, 2.0 * x[:-1])
    lin = lambda e: 3.0 + np.log2(e)
    err, arg = gc().grid_error_numpy(x, rows_of(lin, x, L=1), xm, rows_of(lin, xm, L=1))
    assert np.array_equal(err, np.zeros(len(x) - 1)) and np.array_equal(arg, np.zeros(len(x) - 1, dtype=np.int32))


def test_quadratic_in_ln_e_gives_the_analytic_value():
    # y = u^2 with u = log2 E: at the midpoint of [u0, u0 + 2] the chord is (u0 + 1)^2 + 1, so the absolute
    # error is 1 in the first element; its P0 scale is the largest of u0^2, (u0 + 2)^2, (u0 + 1)^2 (G = 1)
    x = 4.0 ** np.arange(1, 7)
    xm = gc().midpoints(x)
    quad = lambda e: np.log2(e) ** 2
    err, arg = gc().grid_error_numpy(x, rows_of(quad, x, G=1), xm, rows_of(quad, xm, G=1))
    u0 = np.log2(x[:-1])
    assert np.array_equal(err, 1.0 / (u0 + 2.0) ** 2)
    assert np.array_equal(arg, np.zeros(len(u0), dtype=np.int32))         # l = 0 carries the largest weight
    # two groups: the second group's element is twice the first's, and decides
    err2, arg2 = gc().grid_error_numpy(x, rows_of(quad, x), xm, rows_of(quad, xm))
    assert np.array_equal(arg2, np.full(len(u0), 3, dtype=np.int32)) and np.array_equal(err2, err)


def test_zero_rows_nan_duplicate_and_out_of_range_midpoints():
    x = np.array([1.0, 4.0, 4.0, 16.0, 64.0, 256.0, 1024.0])
    xm = np.array([2.0, 4.0, 8.0, 32.0, 300.0, 512.0])
    y = np.ones((7, 2, 2))
    ym = np.full((6, 2, 2), 1.5)
    y[3:5] = 0.0
    ym[3] = 0.0                                   # interval 3: three all-zero rows
    ym[5, 1, 0] = np.nan                          # interval 5: a NaN
    err, arg = gc().grid_error_numpy(x, y, xm, ym)
    assert err[0] == 0.5 / 1.5 and arg[0] == 0
    assert err[1] == -1.0 and arg[1] == -1        # duplicate abscissa
    assert err[2] == 1.0 / 1.5 and arg[2] == 0    # 1 -> 0 interpolated at f = 1/2 is 0.5, fresh row 1.5
    assert err[3] == 0.0                          # zero scale
    assert err[4] == -1.0                         # midpoint outside the interval
    assert err[5] == np.inf and arg[5] == 2
    # P0 scale zero but a higher moment differs: still 0 by the rule
    y0, ym0 = np.zeros((2, 1, 2)), np.zeros((1, 1, 2))
    ym0[0, 0, 1] = 1.0
    e, a = gc().grid_error_numpy([1.0, 4.0], y0, [2.0], ym0)
    assert e[0] == 0.0 and a[0] == 1
    # non-positive or non-finite abscissae are skipped as well
    e, _ = gc().grid_error_numpy([0.0, 4.0, np.inf], np.ones((3, 1, 1)), [2.0, 8.0], np.ones((2, 1, 1)))
    assert np.array_equal(e, [-1.0, -1.0])


def test_tie_rule_lowest_index_wins():
    y = np.zeros((2, 3, 2))
    y[:, :, 0] = 1.0
    ym = y[:1].copy()
    ym[0, 2, 1] = 0.25
    ym[0, 1, 0] = 1.25
    ym[0, 1, 1] = -0.25
    err, arg = gc().grid_error_numpy([1.0, 4.0], y, [2.0], ym)
    assert err[0] == 0.25 / 1.25 and arg[0] == 2      # (g, l) = (1, 0) before (1, 1) and (2, 1)


# ---- refine with a fake evaluator -------------------------------------------------------------------
class Fake:
    """y(E) known in closed form instead of the device: G = 1, L = 2, P0 = 1 everywhere"""

    def __init__(self, fun):
        self.fun, self.calls, self.seen = fun, 0, []

    def rows(self, e):
        e = np.asarray(e, dtype=np.float64)
        out = np.ones((len(e), 1, 2))
        out[:, 0, 1] = self.fun(e)
        return out

    def __call__(self, req):
        self.calls += 1
        for e in req.values():
            self.seen.extend(float(v) for v in e)
        return {k: {"elastic": self.rows(e)} for k, e in req.items()}


def run_refine(fun, x, tol, **kw):
    fake = Fake(fun)
    grids = {"g": dict(x=x, mats={"elastic": fake.rows(x)})}
    kw.setdefault("exclude_last", False)
    new, rep = gc().refine_grids(grids, fake, tol, error=gc().grid_error_numpy, **kw)
    return fake, new["g"], rep["g"]


def test_refine_a_smooth_function_ends_below_tol_with_midpoints_only():
    x0 = np.logspace(-3, 1, 9)
    fun = lambda e: np.sin(np.log(e))
    tol = 1e-3
    fake, g, rep = run_refine(fun, x0, tol, max_passes=10, max_growth=100.0)
    x = g["x"]
    assert rep["stopped"] == "converged" and rep["unresolved"] == [] and rep["skipped"] == 0
    assert rep["points_before"] == 9 and rep["points_after"] == len(x) == 9 + rep["added"] and rep["added"] > 9
    assert np.all(np.diff(x) > 0) and set(x0) <= set(x)
    # every point is an original one or the geometric mean of its two neighbours at insertion time: it lies on
    # the dyadic subdivision of an original interval in ln E
    k = np.searchsorted(x0, x, side="right") - 1
    k = np.minimum(k, len(x0) - 2)
    frac = np.log(x / x0[k]) / np.log(x0[k + 1] / x0[k])
    assert np.allclose(frac * 1024, np.round(frac * 1024), atol=1e-6)
    # the rows kept are the rows evaluated, untouched
    assert np.array_equal(g["mats"]["elastic"], fake.rows(x))
    # an independent check of the final grid: every interval at or below tol
    xm = gc().midpoints(x)
    err, _ = gc().grid_error_numpy(x, fake.rows(x), xm, fake.rows(xm))
    assert err.max() <= tol
    # no energy was evaluated twice, and one evaluate() per pass (+ the closing check)
    assert len(fake.seen) == len(set(fake.seen))
    assert fake.calls == rep["passes"] + 1


def test_refine_checks_only_the_intervals_an_insertion_created():
    # rough only in the first decade: the second pass asks for 2 energies per inserted point, nothing else
    fun = lambda e: np.where(e < 1e-2, np.sin(8 * np.log(e)), 0.0)
    fake, g, rep = run_refine(fun, np.logspace(-3, 1, 5), 1e-2, max_passes=1, max_growth=100.0)
    assert fake.calls == 2 and rep["added"] == 1
    assert len(fake.seen) == 4 + 2


def test_refine_honours_max_passes_and_lists_what_is_left():
    fun = lambda e: np.sin(3 * np.log(e))
    fake, g, rep = run_refine(fun, np.logspace(-3, 1, 5), 1e-6, max_passes=2, max_growth=100.0)
    assert rep["stopped"] == "max_passes" and rep["passes"] == 2 and fake.calls == 3
    assert rep["points_after"] == 5 + 4 + 8
    assert len(rep["unresolved"]) == 16 and all(u["reason"] == "max_passes" and u["err"] > 1e-6 and not u["at_breakpoint"]
                                                 for u in rep["unresolved"])
    lo = [u["interval"][0] for u in rep["unresolved"]]
    assert lo == sorted(lo) and set(lo) <= set(g["x"])


def test_refine_honours_max_growth():
    fun = lambda e: np.sin(3 * np.log(e))
    fake, g, rep = run_refine(fun, np.logspace(-3, 1, 5), 1e-6, max_passes=6, max_growth=2.0)
    # 5 -> 9 fits twice the original length, 9 -> 17 does not: the 8 intervals stay as they are, listed
    assert rep["stopped"] == "max_growth" and rep["points_after"] == 9 and len(g["x"]) == 9
    assert len(rep["unresolved"]) == 8 and all(u["reason"] == "max_growth" for u in rep["unresolved"])
    assert fake.calls == 2


def test_refine_a_step_gives_one_breakpoint_chain_of_max_passes_points():
    step = 0.37
    fun = lambda e: np.where(e < step, 0.0, 0.5)
    x0 = np.logspace(-3, 1, 9)
    for mp in (3, 6):
        fake = Fake(fun)
        grids = {"g": dict(x=x0, mats={"elastic": fake.rows(x0)})}
        new, rep = gc().refine_grids(grids, fake, 1e-3, max_passes=mp, max_growth=4.0, error=gc().grid_error_numpy,
                                     breakpoints={"g": [step]}, exclude_last=False)
        r = rep["g"]
        assert r["added"] == mp and r["points_after"] == 9 + mp and r["stopped"] == "max_passes"
        assert len(r["unresolved"]) == 1 and r["unresolved"][0]["at_breakpoint"]
        lo, hi = r["unresolved"][0]["interval"]
        assert lo <= step <= hi and math.isclose(math.log(hi / lo), math.log(x0[1] / x0[0]) / 2 ** mp)
        assert math.isclose(r["unresolved"][0]["err"], 0.25, rel_tol=1e-9) and r["breakpoints"] == [step]
        added = sorted(set(new["g"]["x"]) - set(x0))
        assert len(added) == mp and all(x0[5] < e < x0[6] for e in added)      # one chain, inside one interval


def test_refine_leaves_the_last_interval_alone_and_rejects_a_bad_tol():
    fun = lambda e: np.where(e < 5.0, 0.0, 0.5)           # a jump inside the last interval only
    fake = Fake(fun)
    x0 = np.logspace(-3, 1, 9)
    new, rep = gc().refine_grids({"g": dict(x=x0, mats={"elastic": fake.rows(x0)})}, fake, 1e-3,
                                 error=gc().grid_error_numpy)
    assert rep["g"]["added"] == 0 and rep["g"]["unresolved"] == [] and len(fake.seen) == 7
    for tol in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gc().refine_grids({}, fake, tol)


def test_check_grids_reports_worst_interval_and_counts():
    fun = lambda e: np.where(e < 0.37, 0.0, 0.5)
    fake = Fake(fun)
    x0 = np.logspace(-3, 1, 9)
    x0[2] = x0[1]                                         # a duplicate: one skipped interval (and its neighbour moves)
    rep = gc().check_grids({"g": dict(x=x0, mats={"elastic": fake.rows(x0)})}, fake, 1e-3, error=gc().grid_error_numpy,
                           breakpoints={"g": [0.37]})["g"]["elastic"]
    assert fake.calls == 1 and rep["intervals"] == 7 and rep["skipped"] == 1 and rep["above"] == 1
    assert rep["worst"] == 0.25 and rep["interval"] == [x0[5], x0[6]] and (rep["group"], rep["order"]) == (0, 1)
    assert rep["at_breakpoint"] and rep["above_intervals"] == [[x0[5], x0[6]]]


# ---- argument checks of the two entry points (before the device) -------------------------------------
def test_grid_error_bad_arguments(hip):
    lib = hip.load()
    x, xm = np.array([1.0, 4.0, 16.0]), np.array([2.0, 8.0])
    y, ym = np.ones((3, 2, 2)), np.ones((2, 2, 2))
    err, arg = np.zeros(2), np.zeros(2, dtype=np.int32)
    good = [2, 2, 3, dp(x), dp(y), dp(xm), dp(ym), dp(err), ip(arg)]
    for pos in range(3, 9):
        a = list(good)
        a[pos] = None
        assert lib.ndpp_grid_error(*a) == -22, pos
    for pos, v in ((0, 0), (1, 0), (2, 1), (2, 0), (0, -3)):
        a = list(good)
        a[pos] = v
        assert lib.ndpp_grid_error(*a) == -22, (pos, v)
    assert b"grid_error" in lib.ndpp_last_error()
    if lib.ndpp_device_count() == 0:
        assert lib.ndpp_grid_error(*good) == -5
        with pytest.raises(hip.NdppError) as e:
            hip.grid_error(x, y, xm, ym)
        assert e.value.code == -5
    with pytest.raises(ValueError):
        hip.grid_error(x, y, xm[:1], ym)


def test_scatt_library_at_bad_arguments(hip):
    from synth import nuclide_case
    lib = hip.load()
    c = nuclide_case()
    nuc = hip.AceNuclide.from_desc(c)
    p = hip.Params.default(c["order"] + 1, c["mu_bins"])
    bins = np.ascontiguousarray(c["bins"], dtype=np.float64)
    res = hip.lib.ScattResult()
    PP = C.POINTER(C.c_double)

    def call(el, inel, p_=p, nuc_=nuc, bins_=bins, res_=res, n=1, n_el=None, n_inel=None, null_list=False):
        el, inel = np.ascontiguousarray(el, dtype=np.float64), np.ascontiguousarray(inel, dtype=np.float64)
        ne = np.array([len(el) if n_el is None else n_el], dtype=np.int32)
        ni = np.array([len(inel) if n_inel is None else n_inel], dtype=np.int32)
        pe = (PP * 1)(None if null_list else dp(el))
        pi = (PP * 1)(dp(inel))
        return lib.ndpp_scatt_library_at(C.byref(p_) if p_ is not None else None, n,
                                         C.byref(nuc_) if nuc_ is not None else None, len(bins), dp(bins_) if bins_ is not None else None,
                                         1, ip(ne), pe, ip(ni), pi, C.byref(res_) if res_ is not None else None)

    good = np.array([1e-9, 1e-8, 1e-8, 1e-6])
    assert call(good, [], p_=None) == -22
    assert call(good, [], nuc_=None) == -22
    assert call(good, [], bins_=None) == -22
    assert call(good, [], res_=None) == -22
    assert call(good, [], n=-1) == -22
    assert call(good, [], n_el=-1) == -22
    assert call(good, [], null_list=True) == -22
    assert call([1e-8, 1e-9], []) == -22 and b"decrease" in lib.ndpp_last_error()
    assert call(good, [1e-3, 1e-4]) == -22
    for bad in (np.nan, np.inf, 0.0, -1e-8):
        assert call([1e-9, bad], []) == -22, bad
        assert call(good, [bad]) == -22, bad
    assert b"not positive and finite" in lib.ndpp_last_error()
    # a list that starts above the top group edge has no row to copy
    assert call([bins[-1] * 1.001, bins[-1] * 1.002], []) == -22 and b"above the top group edge" in lib.ndpp_last_error()
    assert call(good, [bins[-1] * 1.001]) == -22
    # the pointer arrays themselves
    ne = np.array([1], dtype=np.int32)
    assert lib.ndpp_scatt_library_at(C.byref(p), 1, C.byref(nuc), len(bins), dp(bins), 1, ip(ne), None, ip(ne), None,
                                     C.byref(res)) == -22
    assert lib.ndpp_scatt_library_at(C.byref(p), 1, C.byref(nuc), len(bins), dp(bins), 1, None, None, None, None,
                                     C.byref(res)) == -22
    # no nuclide: an empty, successful call; a good call without a device: the device error, nothing kept
    assert lib.ndpp_scatt_library_at(C.byref(p), 0, None, len(bins), dp(bins), 1, None, None, None, None, None) == 0
    if lib.ndpp_device_count() == 0:
        assert call(good, []) == -5
        assert not res.ein_el and not res.el_mat and res.n_el == 0
        with pytest.raises(hip.NdppError) as e:
            hip.scatt_library_at(p, [c], bins, [good], [None], True)
        assert e.value.code == -5


# ---- driver ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [
    (("--refine-grid", "0"), "positive"),
    (("--refine-grid=-1e-3",), "positive"),
    (("--refine-grid", "x"), "not a number"),
    (("--refine-grid", "nan"), "positive"),
    (("--refine-grid", "1e-3", "--max-growth", "0.5"), "--max-growth"),
    (("--check-grid", "--check-tol", "0"), "positive"),
    (("--check-tol", "1e-3"), "--check-grid"),
    (("--refine-grid", "1e-3", "--check-tol", "1e-3"), "--check-grid"),
])
def test_bad_grid_flags_exit_2_and_write_nothing(tmp_path, extra, msg):
    r = case1(tmp_path / "run")
    before = listing(r)
    rc, out = drive(r, *extra, "--json", str(tmp_path / "run.json"))
    assert rc == 2 and msg in out, out
    assert listing(r) == before and not (tmp_path / "run.json").exists()


@pytest.mark.parametrize("extra", [("--check-grid",), ("--refine-grid", "1e-3"), ("--check-grid", "--refine-grid", "1e-3")])
def test_tabular_with_a_grid_flag_exits_2_and_writes_nothing(tmp_path, extra):
    r = case1(tmp_path / "run")
    set_tag(r, "scatt_type", "tabular")
    set_tag(r, "scatt_order", "8")
    before = listing(r)
    rc, out = drive(r, *extra)
    assert rc == 2 and "Legendre output only" in out, out
    assert listing(r) == before


def test_check_grid_without_a_device_exit_3_and_no_partial_files(hip, tmp_path):
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a device is present: the GPU tests run the check to completion")
    for make in (case1, write_case2):
        for extra in (("--check-grid",), ("--refine-grid", "1e-3")):
            r = tmp_path / (make.__name__ + extra[0])
            make(r)
            before = listing(r)
            js = tmp_path / f"{make.__name__}.json"
            rc, out = drive(r, *extra, "--json", str(js))
            assert rc == 3 and "NDPP_EDEVICE" not in out and "error -5" in out, out
            assert listing(r) == before and not js.exists()


def test_table_breakpoints_names_cutoff_and_scattering_thresholds():
    d = dict(freegas_cutoff=1e-6, energy=np.array([1e-11, 1e-3, 1.0, 5.0, 20.0]),
             reactions=[dict(MT=2, thr=1), dict(MT=51, thr=3), dict(MT=52, thr=4), dict(MT=18, thr=2),
                        dict(MT=102, thr=1), dict(MT=16, thr=4)])
    assert gc().table_breakpoints(d) == [1e-6, 1.0, 5.0]
    d["freegas_cutoff"] = math.inf
    assert gc().table_breakpoints(d) == [1.0, 5.0]
