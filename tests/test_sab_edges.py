"""The thermal S(alpha,beta) kernels (ndpp_amd/csrc/sab_kernels.hip) against the Fortran across modes,
orders, group structures and table edges: the cases of synth.sab_edge_cases(), their goldens from
calc_scattsab's Legendre path (tests/golden/sab_edges.npz, written by `make_golden.py sab_edges`),
the C oracle, the gfx950 kernels and their tabular twins; apply_tol_scatt on
synth.apply_tol_edge_inputs().

Each case exists for one condition, stated in its `why`; test_case_condition computes that condition
from the case's inputs alone (P0 per group through the numpy restatement thermal_tab_ref at one bin,
which shares nothing with the kernels), so that an edit of the generator cannot empty a case unnoticed.
A condition that asks for a table per mode, or per kind of elastic data, has one case per table
(VARIANTS)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import thermal_tab_ref as tab_ref
from conftest import OracleParams, dp, load_golden, oracle_params
from synth import (SAB_EDGE_EXTEND_PTS, SAB_EDGE_TOL, SAB_G8, SAB_MODE_SEEDS, apply_tol_edge_inputs, sab_edge_cases,
                   sab_groups_bins, sab_revisit_table)

CASES = sab_edge_cases()
NAMES = list(CASES)
TOL_INPUTS = apply_tol_edge_inputs()
KEYS = ("el", "inel", "mat")
MODES3 = ("m0", "m1", "m2")
VARIANTS = {"orders_1": MODES3, "orders_11": MODES3, "groups_1": MODES3, "groups_70": MODES3, "groups_300": MODES3,
            "cont_first_eout_positive": ("",), "cont_edges_on_points": ("",), "cont_two_point_rows": ("",),
            "skewed_min": ("",), "top_inside": MODES3, "bottom_above_zero": MODES3,
            "elastic_edges": ("coherent", "incoherent"), "inel_edges": MODES3, "thresholds_el_below": ("",),
            "thresholds_el_above": ("",), "exact_with_cosines": ("",), "two_energies": ("",),
            "eout_revisits_group": ("m0", "m1")}


@pytest.fixture(scope="module")
def golden():
    return load_golden("sab_edges")


def _gold(golden, name):
    return [golden[f"{name}_{k}"] for k in KEYS]


def _same(a, b):
    """every bit, the NaN pattern included"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


# ---- the inputs -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _p0(name):
    """(el, inel) P0 [NE][G] of a case from its inputs: the restatement at one bin"""
    c = CASES[name]
    _, el, inel, status = tab_ref.sab_tab(c["table"], c["ein"], c["bins"], 1)
    assert not status.any()
    return el[:, :, 0], inel[:, :, 0]


def _plain(x):
    s = 0.0
    for v in x:
        s = s + float(v)
    return s


def _kahan(x):
    s = c = 0.0
    for v in x:
        y = float(v) - c
        t = s + y
        c = (t - s) - y
        s = t
    return s


def _rows(t):
    """the outgoing energies of each continuous row"""
    return [t["ce_out"][a:b] for a, b in zip(t["cptr"][:-1], t["cptr"][1:])]


def _has_nbrs(ein, v):
    return {float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))} <= set(ein.tolist())


def _mode_of(name):
    return int(name[-1])


def _cond_orders(name, c, L):
    t = c["table"]
    assert c["L"] == L and len(c["bins"]) - 1 == 8 and t["mode"] == _mode_of(name)
    assert t["el_mode"] == 3 and t["NMUe"] > 0 and t["threshold_elastic"] > 0


def _cond_groups(name, c, G):
    t, bins = c["table"], c["bins"]
    same = CASES[f"orders_1_m{_mode_of(name)}"]["table"]
    assert all(np.array_equal(t[k], same[k]) for k in t) and t["mode"] == _mode_of(name)
    assert len(bins) - 1 == G and bins[0] == 0.0 and bins[-1] == 20.0 and np.array_equal(bins, sab_groups_bins(G))
    assert np.array_equal(c["ein"], CASES[f"groups_1_m{_mode_of(name)}"]["ein"])
    if G > 1:
        r = bins[2:] / bins[1:-1]
        assert np.allclose(r[:-1], r[0], rtol=1e-9)                    # log-spaced
        el, inel = _p0(name)
        differ = [i for i, row in enumerate(el + inel) if _plain(row) != _kahan(row)]
        assert differ, "no row tells a plain sum over the groups from the compensated one"


def _cond_cont_first(name, c):
    t, bins = c["table"], c["bins"]
    assert t["mode"] == 2
    pos = [r for r in _rows(t) if r[0] > 0]
    assert len(pos) >= 2 and len(pos) < t["NEi"]
    for r in pos:
        assert (np.diff(r) > 0).all() and (bins < r[0]).sum() >= 3           # both edges of a group below Eout(1) ...
        assert ((bins[:-1] < r[0]) & (bins[1:] >= r[0]) & (bins[1:] < r[-1])).any()   # ... and a group that straddles it


def _cond_cont_on_points(name, c):
    t, inner = c["table"], c["bins"][1:-1]
    assert t["mode"] == 2 and all((np.diff(r) > 0).all() for r in _rows(t))
    rows = _rows(t)
    assert sum(np.isin(inner, r[1:-1]).any() for r in rows) >= 2            # f_lo = f_hi = 0
    assert any(r[0] > 0 and r[0] in inner for r in rows)
    assert any(r[-1] in inner for r in rows)


def _cond_two_point(name, c):
    t = c["table"]
    n = np.diff(t["cptr"])
    assert t["mode"] == 2 and t["NMU"] == 1 and n.min() == 2 and (n == 2).sum() >= 2 and (n > 2).any()


def _cond_skewed_min(name, c):
    t = c["table"]
    assert t["mode"] == 1 and t["NEo"] == 5 and t["NMU"] == 1


def _coherent(t):
    return t["el_mode"] == 4 and t["NMUe"] == 0 and t["NEe"] >= 2 and t["threshold_elastic"] > 0


def _cond_top_inside(name, c):
    t, bins, ein = c["table"], c["bins"], c["ein"]
    top = bins[-1]
    assert _coherent(t) and t["mode"] == _mode_of(name) and bins[0] == 0.0
    assert top < min(t["threshold_inelastic"], t["threshold_elastic"]) and _has_nbrs(ein, top)
    assert t["ee"][0] < top                                                  # elastic data reach the top edge
    if t["mode"] != 2:
        assert (t["e_out"] >= top).any() and (t["e_out"] < top).any()
    el, inel = _p0(name)
    tot = (el + inel).sum(axis=1)
    assert (tot[:-1] == 0).any() and (tot > 0).any()                         # rows that end with no mass
    assert el[ein == top].sum() > 0 and el[ein > top].sum() == 0


def _cond_bottom_above(name, c):
    t, bins, ein = c["table"], c["bins"], c["ein"]
    same = CASES[f"top_inside_m{_mode_of(name)}"]["table"]
    assert all(np.array_equal(t[k], same[k]) for k in t)
    assert bins[0] > 0 and _has_nbrs(ein, bins[0])
    assert ((ein >= t["ee"][0]) & (ein < bins[0])).sum() >= 2                 # elastic: Ein < e_bins(1)
    if t["mode"] != 2:
        assert (t["e_out"] < bins[0]).any() and (t["e_out"] > bins[0]).any()


def _cond_elastic_edges(name, c):
    t, ein = c["table"], c["ein"]
    kind = name.rsplit("_", 1)[1]
    assert _coherent(t) if kind == "coherent" else (t["el_mode"] == 3 and t["NMUe"] > 0)
    ee = t["ee"]
    assert t["threshold_elastic"] == ee[-1] and all(_has_nbrs(ein, e) for e in ee)
    assert len(ein) == 3 * len(ee) + 1 and (ein < np.nextafter(ee[0], -np.inf)).sum() == 1


def _cond_inel_edges(name, c):
    t, ein = c["table"], c["ein"]
    ei = t["ei"]
    assert t["mode"] == _mode_of(name) and t["threshold_inelastic"] == ei[-1]
    assert all(_has_nbrs(ein, e) for e in ei) and len(ein) == 3 * len(ei) + 2
    assert (ein < np.nextafter(ei[0], -np.inf)).sum() == 2


def _cond_thresholds(name, c, below):
    t, ein = c["table"], c["ein"]
    te, ti = t["threshold_elastic"], t["threshold_inelastic"]
    assert _coherent(t) and te == t["ee"][-1] and ti == t["ei"][-1]
    assert (te < ti) if below else (te > ti)
    between = (ein > min(te, ti)) & (ein < max(te, ti))
    assert between.sum() >= 3 and _has_nbrs(ein, te)
    el, inel = (a.sum(axis=1) for a in _p0(name))
    if below:
        assert (el[between] == 0).all() and (inel[between] > 0).all()         # inelastic only
    else:
        assert (inel[between] == 0).all() and (el[between] > 0).all()         # elastic only
    assert ((el > 0) & (inel > 0)).any()


def _cond_exact_cosines(name, c):
    t, ein = c["table"], c["ein"]
    assert t["el_mode"] == 4 and t["NMUe"] > 0 and t["threshold_elastic"] == t["ee"][-1]
    assert ((ein >= t["ee"][0]) & (ein < t["threshold_elastic"])).sum() >= 10
    assert not _p0(name)[0].any()                                            # sig * 0


def _cond_two_energies(name, c):
    assert len(c["ein"]) == 2 and (_p0(name)[1].sum(axis=1) > 0).all()


def _group_runs(t, bins, E):
    """the groups (1-based) the discrete outgoing energies of incoming energy E fall into, in the table's
    order, consecutive repeats taken once (sab.F90:196-242: the row's bracket, the blend, the group search)"""
    ei, NEi = t["ei"], t["NEi"]
    eo = t["e_out"].reshape(NEi, t["NEo"])
    if E < ei[0]:
        isab, f = 1, 0.0
    elif E > t["threshold_inelastic"]:
        return []
    elif E == t["threshold_inelastic"]:
        isab, f = NEi - 1, 1.0
    else:
        isab = int(tab_ref.bracket(ei, E))
        f = (E - ei[isab - 1]) / (ei[isab] - ei[isab - 1])
    Eout = (1.0 - f) * eo[isab - 1] + f * eo[isab]
    g = tab_ref.bracket(bins, Eout)[(Eout >= bins[0]) & (Eout < bins[-1])]
    return [int(v) for k, v in enumerate(g) if k == 0 or v != g[k - 1]]


def _cond_eout_revisits(name, c):
    t, bins, ein = c["table"], c["bins"], c["ein"]
    assert t["mode"] == _mode_of(name) and t["NEo"] == 9 and np.array_equal(bins, SAB_G8)
    eo = t["e_out"].reshape(t["NEi"], 9)
    order = np.argsort(eo, axis=1)
    assert (order == order[0]).all() and (np.diff(np.sort(eo, axis=1), axis=1) > 0).all()   # one order in every row
    most = 0
    for E in ein:
        runs = _group_runs(t, bins, float(E))
        assert len(runs) > len(set(runs)), (float(E), runs)              # a group in two separate runs
        most = max(most, max(runs.count(g) for g in set(runs)))
    assert most >= 3                                                     # left and come back to at least twice
    assert len({g for E in ein for g in _group_runs(t, bins, float(E))}) >= 3


CONDITIONS = {"orders_1": lambda n, c: _cond_orders(n, c, 1), "orders_11": lambda n, c: _cond_orders(n, c, 11),
              "groups_1": lambda n, c: _cond_groups(n, c, 1), "groups_70": lambda n, c: _cond_groups(n, c, 70),
              "groups_300": lambda n, c: _cond_groups(n, c, 300), "cont_first_eout_positive": _cond_cont_first,
              "cont_edges_on_points": _cond_cont_on_points, "cont_two_point_rows": _cond_two_point,
              "skewed_min": _cond_skewed_min, "top_inside": _cond_top_inside, "bottom_above_zero": _cond_bottom_above,
              "elastic_edges": _cond_elastic_edges, "inel_edges": _cond_inel_edges,
              "thresholds_el_below": lambda n, c: _cond_thresholds(n, c, True),
              "thresholds_el_above": lambda n, c: _cond_thresholds(n, c, False),
              "exact_with_cosines": _cond_exact_cosines, "two_energies": _cond_two_energies,
              "eout_revisits_group": _cond_eout_revisits}


def test_case_names_are_the_condition_names():
    assert set(CONDITIONS) == set(VARIANTS) == {c["cond"] for c in CASES.values()}
    want = [f"{cond}_{v}" if v else cond for cond, vs in VARIANTS.items() for v in vs]
    assert sorted(want) == sorted(NAMES)
    assert all(n == c["cond"] or n.startswith(c["cond"] + "_") for n, c in CASES.items())
    assert set(SAB_MODE_SEEDS) == {0, 1, 2}


@pytest.mark.parametrize("name", NAMES)
def test_case_condition(name):
    """The condition each case exists for, from its inputs; and what every case keeps: the size limits
    and the two rules (nothing makes the reference stop, the case brings its own grid)."""
    c = CASES[name]
    t, bins, ein, L = c["table"], c["bins"], c["ein"], c["L"]
    G = len(bins) - 1
    assert c["why"] and set(c) == {"cond", "table", "bins", "ein", "L", "why", "egrid"}
    assert t["NEi"] <= 8 and len(t["ei"]) == t["NEi"] and t["NEe"] <= 8 and 2 <= len(ein) <= 140
    assert (t["NEo"] <= 9) if t["mode"] != 2 else (np.diff(t["cptr"]).max() <= 9 and np.diff(t["cptr"]).min() >= 2)
    assert 1 <= L <= 11 and (L < 11 or G <= 8) and (G < 300 or L <= 2)
    assert (np.diff(ein) > 0).all() and (np.diff(bins) > 0).all() and (np.diff(t["ei"]) > 0).all()
    # binary_search stops the reference on a value outside its array (search.F90:36): no incoming energy
    # lies between a table's last energy and its threshold
    assert t["threshold_inelastic"] == t["ei"][-1]
    if t["threshold_elastic"] != 0.0:
        assert t["threshold_elastic"] == t["ee"][-1] and (np.diff(t["ee"]) > 0).all()
    assert c["egrid"] == (bins[0] == 0.0 and bins[-1] >= 19.99)
    if c["cond"].startswith(("groups_", "orders_")):
        assert c["egrid"]
    CONDITIONS[c["cond"]](name, c)


@pytest.mark.parametrize("name", ["eout_revisits_group_m0", "eout_revisits_group_m1"])
def test_eout_revisits_needs_the_permutation(name):
    """With the outgoing energies back in sorted order the groups are visited once each: the check fails."""
    c = dict(CASES[name], table=sab_revisit_table(_mode_of(name), perm=range(9)))
    assert all(len(set(r)) == len(r) for r in (_group_runs(c["table"], c["bins"], float(E)) for E in c["ein"]))
    with pytest.raises(AssertionError):
        _cond_eout_revisits(name, c)


def test_apply_tol_inputs_hold_the_rows_asked_for():
    assert [a.shape for a in TOL_INPUTS.values()] == [(1, 1, 1), (129, 8, 11), (40, 70, 2), (40, 300, 2)]
    tol = SAB_EDGE_TOL
    for name, a in TOL_INPUTS.items():
        p0 = a[:, :, 0]
        if len(a) == 1:
            assert 0 < p0[0, 0] < tol
            continue
        assert not a[1].any()
        assert ((p0[2] > 0).sum() >= 2) and (p0[2][p0[2] > 0] < tol).all() and (p0[2] >= 0).all()
        assert (p0 == tol).any() and (p0 < 0).any() and np.count_nonzero(a[5]) == a.shape[2] and a[5].max() > tol
        assert p0[6].sum() < 0
        live = p0[7:]
        assert ((live > 0) & (live < tol)).any() and (live > tol).any() and (live == 0).any()


# ---- the oracle and the host grid against the Fortran (CPU) ---------------------------------------
def _oracle(oracle, hip, c, ein=None):
    ein = np.ascontiguousarray(c["ein"] if ein is None else ein)
    bins = np.ascontiguousarray(c["bins"])
    flat = hip.SabFlat.from_dict(c["table"])
    p = oracle_params(oracle, c["L"], 2001)
    G = len(bins) - 1
    el, inel, mat = (np.zeros((len(ein), G, c["L"])) for _ in range(3))
    oracle.oracle_calc_scattsab.restype = C.c_int
    oracle.oracle_calc_scattsab.argtypes = [C.POINTER(OracleParams), C.c_void_p, C.c_int,
                                            C.POINTER(C.c_double), C.c_int] + [C.POINTER(C.c_double)] * 4
    assert oracle.oracle_calc_scattsab(C.byref(p), C.byref(flat), len(ein), dp(ein), G, dp(bins),
                                       dp(el), dp(inel), dp(mat)) == 0
    return el, inel, mat


@pytest.mark.parametrize("name", NAMES)
def test_oracle_vs_golden(oracle, hip, golden, name):
    c = CASES[name]
    assert np.array_equal(golden[f"{name}_ein"], c["ein"]) and np.array_equal(golden[f"{name}_bins"], c["bins"])
    ref = _gold(golden, name)
    for k, a, b in zip(KEYS, _oracle(oracle, hip, c), ref):
        assert _same(a, b), (name, k)
    el, inel, mat = ref
    assert not any(np.isnan(a).any() for a in ref)
    assert np.array_equal(mat[-1], mat[-2])                          # combine_sab_grid, sab.F90:452
    p0 = mat[:, :, 0].sum(axis=1)
    assert np.all((np.abs(p0 - 1) < 1e-14) | (p0 == 0)) and (p0 > 0).any()
    # the golden holds what the condition was computed from: P0 of the restatement, bit for bit
    rel, rinel = _p0(name)
    assert np.array_equal(el[:, :, 0], rel) and np.array_equal(inel[:, :, 0], rinel)
    if c["cond"] == "groups_1":
        # P0 = x * (1 / x): 1, or its neighbour where the reciprocal's rounding shows (the Fortran's own arithmetic)
        assert (p0 == 0).any() or c["table"]["mode"] != 2
        assert (np.abs(p0[p0 != 0] - 1.0) <= 2.0 ** -52).all() and (p0 == 1.0).any()
    if c["cond"] in ("groups_70", "groups_300"):
        # the rows that tell the two sums apart: normalised by the plain sum they would differ from the Fortran
        tot = el + inel
        rows = [i for i in range(len(tot) - 1) if _plain(tot[i, :, 0]) != _kahan(tot[i, :, 0])]
        assert rows
        assert all(np.array_equal(mat[i], tot[i] * (1.0 / _kahan(tot[i, :, 0]))) for i in rows)
        assert any(not np.array_equal(mat[i], tot[i] * (1.0 / _plain(tot[i, :, 0]))) for i in rows)
    if c["egrid"]:
        grid = golden[f"{name}_egrid"]
        p = hip.Params.default(c["L"], 2001)
        p.extend_pts = SAB_EDGE_EXTEND_PTS
        assert np.array_equal(hip.sab_egrid(c["table"], c["bins"], extend_pts=SAB_EDGE_EXTEND_PTS), grid)
        assert np.array_equal(hip.sab_egrid_lib(p, c["table"], c["bins"]), grid)
    else:
        assert f"{name}_egrid" not in golden


@pytest.fixture(scope="module")
def ref_sab(ref, tmp_path_factory):
    """The reference build with the shim's thermal entries.  conftest's `ref` builds only when no
    library is there; one built from an older shim is rebuilt as conftest builds it and loaded from a
    copy (the linker replaces the file; the old one stays mapped under its name)."""
    if all(hasattr(ref, k) for k in ("ref_calc_scattsab", "ref_sab_egrid", "ref_apply_tol_scatt")):
        return ref
    import shutil
    from conftest import REF_SO, ROOT, _make
    _make(ROOT / "oracle", "ref")
    fresh = tmp_path_factory.mktemp("ref") / "libndpp_ref_fresh.so"
    shutil.copy(REF_SO, fresh)
    R = C.CDLL(str(fresh))
    R.ref_set_params.argtypes = ref.ref_set_params.argtypes
    return R


def test_golden_is_what_the_reference_gives(ref_sab, golden, tmp_path):
    """Where the reference build exists: sab_edge_goldens writes the stored file again, array for array."""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, str(GOLDEN))
    from make_golden import sab_edge_goldens
    out = tmp_path / "sab_edges.npz"
    sab_edge_goldens(ref_sab, out=out)
    z = np.load(out)
    assert set(z.files) == set(golden)
    for k in z.files:
        assert _same(z[k], golden[k]), k
    assert (GOLDEN / "sab_edges.npz").stat().st_size <= (GOLDEN / "sweep_ref_g70_seed4242.npz").stat().st_size


def _apply_tol_py(data, tol, total):
    """apply_tol_scatt (scatt.F90:786-818) in numpy, the two sum()s taken by `total`"""
    out = data.copy()
    for row in out:
        orig = total(row[:, 0])
        row[(row[:, 0] > 0.0) & (row[:, 0] < tol)] = 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            norm = np.float64(orig) / np.float64(total(row[:, 0])) if orig > 0.0 else 0.0
            row *= norm
    return out


@pytest.mark.parametrize("name", list(TOL_INPUTS))
def test_apply_tol_golden_needs_the_compensated_sum(golden, name):
    """The routine restated with compensated sums is the golden bit for bit; with plain sums it is not,
    from 8 groups on: the goldens tell the two apart."""
    data, want = TOL_INPUTS[name], golden[f"tol_{name}_out"]
    assert _same(_apply_tol_py(data, SAB_EDGE_TOL, _kahan), want)
    if data.shape[1] >= 8:
        assert not _same(_apply_tol_py(data, SAB_EDGE_TOL, _plain), want)


@pytest.mark.parametrize("name", list(TOL_INPUTS))
def test_apply_tol_oracle_vs_golden(oracle, golden, name):
    data = TOL_INPUTS[name]
    assert np.array_equal(golden[f"tol_{name}_in"], data)
    n, G, L = data.shape
    got = data.copy()
    oracle.oracle_apply_tol_scatt.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double]
    oracle.oracle_apply_tol_scatt(L, G, n, dp(got), SAB_EDGE_TOL)
    want = golden[f"tol_{name}_out"]
    assert _same(got, want)
    nan_rows = np.isnan(want).any(axis=(1, 2))
    if n == 1:
        assert nan_rows.all()
        return
    # NaN = 0 * (orig / 0): the rows with a positive total of which nothing is kept
    p0 = data[:, :, 0]
    emptied = (p0.sum(axis=1) > 0) & ~((p0 >= SAB_EDGE_TOL) | (p0 < 0)).any(axis=1)
    assert np.array_equal(nan_rows, emptied) and nan_rows[2] and np.isnan(want[nan_rows]).all()
    assert not want[1].any() and not want[6].any()
    assert want[3, 0, 0] > 0 and want[4, 0, 0] < 0 and np.array_equal(want[5], data[5])
    keep = ~nan_rows
    keep[6] = False
    assert np.allclose(want[keep][:, :, 0].sum(axis=1), data[keep][:, :, 0].sum(axis=1), rtol=1e-14)
    assert np.count_nonzero(want[keep]) < np.count_nonzero(data[keep])


# ---- the kernels (GPU) -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_sab_edges_vs_golden(hip, golden, name):
    """The file's own claim: every bit of el, inel and scatt_mat is the Fortran's."""
    c = CASES[name]
    mat, el, inel = hip.sab_batch(hip.Params.default(c["L"], 2001), c["table"], c["ein"], c["bins"], want_parts=True)
    for k, a in zip(KEYS, (el, inel, mat)):
        assert _same(a, golden[f"{name}_{k}"]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_sab_edges_tabular_one_bin(hip, golden, name):
    """One bin is the Legendre path's order 0: the same masses in the same order."""
    c = CASES[name]
    mat, el, inel, status = hip.sab_tab_batch(hip.Params.default(1, 2001), 1, c["table"], c["ein"], c["bins"],
                                              want_parts=True, want_status=True)
    for k, a in zip(KEYS, (el, inel, mat)):
        assert _same(a, golden[f"{name}_{k}"][..., :1]), (name, k)
    assert not status.any()                                          # every table here is finite


def _combine_as_defined(el, inel):
    """scatt_mat from el and inel as include/ndpp_hip.h defines it for the tabular output: rows scaled by
    1 / s, s the compensated sum of el + inel over the row in storage order; the last row copies its
    neighbour.  (thermal_tab_ref.combine takes the exactly rounded sum, math.fsum.)"""
    tot = el + inel
    mat = np.zeros_like(tot)
    for i in range(len(tot)):
        s = _kahan(tot[i].ravel())
        if s > 0.0:
            mat[i] = tot[i] * (1.0 / s)
    if len(mat) >= 2:
        mat[-1] = mat[-2]
    return mat


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_sab_edges_tabular_restatement(hip, name):
    """Eight bins against the numpy restatement.  el and inel bit for bit: the restatement drops the
    masses of a bin in the kernels' order (np.add.at is sequential).  scatt_mat bit for bit against the
    restatement's rows under the sum the interface defines, and against thermal_tab_ref.combine (the
    exactly rounded sum) wherever the two sums of the row agree.  Elsewhere: the compensated sum is within
    2^-52 s of the exact one and math.fsum within 2^-53 s, 1 / s and the product round once on each side
    (4 * 2^-53), together 3.5 * 2^-52 < 2^-50 relative to the row's largest entry."""
    c = CASES[name]
    N = 8
    mat, el, inel, status = hip.sab_tab_batch(hip.Params.default(1, 2001), N, c["table"], c["ein"], c["bins"],
                                              want_parts=True, want_status=True)
    rmat, rel, rinel, rstatus = tab_ref.sab_tab(c["table"], c["ein"], c["bins"], N)
    assert _same(el, rel) and _same(inel, rinel) and np.array_equal(status, rstatus) and not status.any()
    assert _same(mat, _combine_as_defined(rel, rinel))
    tot = rel + rinel
    agree = np.array([_kahan(r.ravel()) == math.fsum(r.ravel()) for r in tot])
    agree[-1] = agree[-2] if len(agree) >= 2 else agree[-1]
    print(f"sab_edges {name}: {int((~agree).sum())} of {len(agree)} rows whose compensated sum is not the exact one")
    assert np.array_equal(mat[agree], rmat[agree])
    assert (np.abs(mat - rmat).max(axis=(1, 2)) <= 2.0 ** -50 * rmat.max(axis=(1, 2))).all()


def _padded(ein, n):
    """ein with midpoints put in until it has n points, cut to n"""
    e = np.asarray(ein, dtype=np.float64)
    while len(e) < n:
        e = np.unique(np.concatenate([e, 0.5 * (e[1:] + e[:-1])]))
    return np.ascontiguousarray(e[:n])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["orders_11_m0", "orders_11_m2"])
def test_gpu_sab_launch_shape(hip, name):
    """Thread per (E_in, order) in blocks of 128 at L = 11: prefixes of 2, 11, 12, 13 (the first block ends
    inside incoming energy 12) and 129 energies, and the grid reversed.  A row of el and inel depends on
    its energy alone; so does a row of scatt_mat, but the last row of every run is the copy of its
    neighbour (combine_sab_grid, sab.F90:452)."""
    c = CASES[name]
    assert c["L"] == 11
    grid = _padded(c["ein"], 129)
    run = lambda e: hip.sab_batch(hip.Params.default(11, 2001), c["table"], e, c["bins"], want_parts=True)
    mat, el, inel = run(grid)
    assert len(grid) == 129 and len({a.tobytes() for a in inel}) > 100 and np.array_equal(mat[-1], mat[-2])
    for n in (2, 11, 12, 13, 129):
        m, e, q = run(grid[:n].copy())
        assert np.array_equal(e, el[:n]) and np.array_equal(q, inel[:n]), n
        assert np.array_equal(m[:n - 1], mat[:n - 1]) and np.array_equal(m[n - 1], mat[n - 2]), n
    m, e, q = run(grid[::-1].copy())
    assert np.array_equal(e[::-1], el) and np.array_equal(q[::-1], inel)
    assert np.array_equal(m[1:128][::-1], mat[1:128]) and np.array_equal(m[128], m[127])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TOL_INPUTS))
def test_gpu_apply_tol_edges(hip, golden, name):
    assert _same(hip.apply_tol_scatt(TOL_INPUTS[name], SAB_EDGE_TOL), golden[f"tol_{name}_out"])
