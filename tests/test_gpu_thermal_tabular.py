"""GPU: tabular output of thermal S(alpha,beta) tables (ndpp_sab_tab_batch, include/ndpp_hip.h)
against the numpy restatement tests/thermal_tab_ref.py bin by bin, against ndpp_sab_batch (the
Legendre path, pinned to the Fortran) at N = 1, in the bin sums and through the enclosure of its
moments, and the driver's --thermal-tabular.

The bar on |GPU - restatement| per bin is 4 n 2^-53 relative to the E_in's largest group P0
(tabular_ref.p0_scale), n the largest number of masses one bin can receive in the case: the
standard bound on two summation orders of n non-negative terms."""
import functools
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
import tabular_ref
import thermal_tab_ref as ref
from synth import sab_ein_grid, sab_table
from test_e2e_reference import CASE2, case2_tables

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)
ELASTIC = (None, "coherent", "incoherent")
NS = (1, 2, 3, 7, 32, 128)
U = 2.0 ** -53
# Nine groups in the thermal range.  The discrete modes' outgoing energies run from 1.2e-9 to 7.2e-6
# and the continuous rows' from 0 to 3 E_in + 12 kT (3e-7 .. 1.2e-5): some fall below the first edge
# and some above the last; nothing falls into the group of width 1e-15 in the discrete modes, and in
# the continuous mode the low rows end below the upper groups, so that a row has edges inside and
# outside its range (asserted in test_the_case_is_the_one_asked_for).
BINS = np.array([2e-9, 1e-8, 2.5e-8, 6e-8, 1.5e-7, 4e-7, 1e-6, 1e-6 * (1 + 1e-9), 2.5e-6, 5e-6])


@functools.lru_cache(maxsize=None)
def table(mode, elastic):
    return sab_table(mode, seed=1000 + mode, elastic=elastic)


@functools.lru_cache(maxsize=None)
def grid(mode, elastic):
    e = sab_ein_grid(table(mode, elastic))
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def restated(mode, elastic, N):
    out = ref.sab_tab(table(mode, elastic), grid(mode, elastic), BINS, N)
    for a in out:
        a.setflags(write=False)
    return out


_GPU = {}


def gpu(hip, mode, elastic, N):
    """(scatt_mat, el, inel, status) of one call, computed once"""
    key = (mode, elastic, N)
    if key not in _GPU:
        p = hip.Params.default(1, 2001)
        _GPU[key] = hip.sab_tab_batch(p, N, table(mode, elastic), grid(mode, elastic), BINS, want_parts=True,
                                      want_status=True)
    return _GPU[key]


def legendre(hip, mode, elastic, L):
    key = (mode, elastic, -L)
    if key not in _GPU:
        _GPU[key] = hip.sab_batch(hip.Params.default(L, 2001), table(mode, elastic), grid(mode, elastic), BINS,
                                  want_parts=True)
    return _GPU[key]


def bars(t):
    """the bar of scatt_mat / inel and of el"""
    n_in, n_el = ref.masses_per_bin(t)
    return 4 * n_in * U, 4 * max(n_el, 1) * U


def check_against(got, want, bar, label):
    p0 = want.sum(axis=2)
    err, at = tabular_ref.bin_err(got, want, p0)
    print(f"{label}: worst bin {err:.3e} at {at} (bar {bar:.3e})")
    assert np.array_equal(got == 0, want == 0), label
    assert err <= bar, label


def test_the_case_is_the_one_asked_for():
    assert 5 <= len(BINS) - 1 <= 12
    for mode in MODES:
        t = table(mode, None)
        e = grid(mode, None)
        assert 40 <= len(e) <= 50 and e[0] < t["ei"][0] and e[-1] > t["threshold_inelastic"]
        assert np.isin(t["ei"][[0, 3, -1]], e).all()
        _, _, inel, _ = restated(mode, None, 1)
        p0 = inel[:, :, 0]
        if mode == 2:
            n = np.diff(t["cptr"])
            assert n.min() >= 10 and n.max() <= 30
            top = t["ce_out"][t["cptr"][1:] - 1]
            assert (top > BINS[-1]).any() and t["ce_out"][t["cptr"][0]] < BINS[0]
            inside = (BINS[None, :] < top[:, None]).sum(axis=1)
            assert ((inside > 0) & (inside < len(BINS))).any()          # one edge inside, one outside
            assert ((p0 == 0).any(axis=1) & (p0 > 0).any(axis=1)).any()  # a group of a live row receives nothing
        else:
            eo = t["e_out"]
            assert (eo < BINS[0]).any() and (eo >= BINS[-1]).any()
            assert (p0[:, 5] > 0).any() and (p0[:, 6] == 0).all() and (p0[:, 7] > 0).any()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("elastic", ELASTIC)
@pytest.mark.parametrize("mode", MODES)
def test_bin_by_bin_against_the_restatement(hip, mode, elastic, N):
    t = table(mode, elastic)
    mat, el, inel, status = gpu(hip, mode, elastic, N)
    rmat, rel, rinel, rstatus = restated(mode, elastic, N)
    bar_in, bar_el = bars(t)
    assert mat.shape == (len(grid(mode, elastic)), len(BINS) - 1, N)
    check_against(inel, rinel, bar_in, f"mode {mode} {elastic} N={N} inel")
    check_against(el, rel, bar_el, f"mode {mode} {elastic} N={N} el")
    check_against(mat, rmat, bar_in, f"mode {mode} {elastic} N={N} scatt_mat")
    assert np.array_equal(status, rstatus) and (status == 0).all()
    assert (mat >= 0).all() and (inel.sum(axis=(1, 2)) > 0).sum() >= 40


@pytest.mark.parametrize("elastic", ELASTIC)
@pytest.mark.parametrize("mode", MODES)
def test_one_bin_is_the_legendre_path_at_order_one(hip, mode, elastic):
    mat, el, inel, _ = gpu(hip, mode, elastic, 1)
    lmat, lel, linel = legendre(hip, mode, elastic, 1)
    assert np.array_equal(mat, lmat) and np.array_equal(el, lel) and np.array_equal(inel, linel)
    assert mat.any() and inel.any() and (elastic is None or el.any())


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("elastic", ELASTIC)
@pytest.mark.parametrize("mode", MODES)
def test_bins_sum_to_p0(hip, mode, elastic, N):
    bar_in, bar_el = bars(table(mode, elastic))
    for name, got, want, bar in zip(("scatt_mat", "el", "inel"), gpu(hip, mode, elastic, N),
                                    legendre(hip, mode, elastic, 1), (bar_in, bar_el, bar_in)):
        p0 = want[:, :, 0]
        err = float((np.abs(got.sum(axis=2) - p0) / tabular_ref.p0_scale(p0)[:, None]).max())
        print(f"mode {mode} {elastic} N={N} {name}: |sum_k T - P0| {err:.3e} (bar {bar:.3e})")
        assert err <= bar


@pytest.mark.parametrize("N", (1, 16, 64, 3))
@pytest.mark.parametrize("elastic", ELASTIC)
@pytest.mark.parametrize("mode", MODES)
def test_refinement_keeps_every_mass_in_its_pair(hip, mode, elastic, N):
    bar_in, bar_el = bars(table(mode, elastic))
    coarse, fine = gpu(hip, mode, elastic, N), gpu(hip, mode, elastic, 2 * N)
    for name, c, f, bar in zip(("scatt_mat", "el", "inel"), coarse, fine, (bar_in, bar_el, bar_in)):
        pairs = f.reshape(f.shape[0], f.shape[1], N, 2).sum(axis=3)
        err, at = tabular_ref.bin_err(pairs, c, c.sum(axis=2))
        print(f"mode {mode} {elastic} {2 * N} -> {N} {name}: {err:.3e} at {at} (bar {bar:.3e})")
        assert np.array_equal(pairs == 0, c == 0) and err <= bar


@pytest.mark.parametrize("N", (32, 128))
@pytest.mark.parametrize("elastic", ELASTIC)
@pytest.mark.parametrize("mode", MODES)
def test_bins_enclose_the_moments(hip, mode, elastic, N):
    for name, tab, leg in zip(("scatt_mat", "el", "inel"), gpu(hip, mode, elastic, N), legendre(hip, mode, elastic, 6)):
        v = tabular_ref.enclosure_violation(tab, leg, lmax=5)
        print(f"mode {mode} {elastic} N={N} {name}: enclosure violation {v:.3e}")
        assert v <= 1e-12


# ---- the rule at its edges -------------------------------------------------------------------
EDGE_MU = np.array([-1.0, -0.5, 0.0, 0.5, 1.0, np.nextafter(0.5, 0.0), 1.0 + 1e-12, -1.0 - 1e-12])
# The bin is the value of the floating-point expression, not of the real-number one: the cosine one
# ulp below the edge 0.5 gives mu + 1.0 = 1.5 exactly (the sum rounds to even) and goes up with it.
EDGE_BIN = {4: [0, 1, 2, 3, 3, 3, 3, 0], 8: [0, 2, 4, 6, 7, 6, 7, 0]}


def test_the_edge_bins_are_the_definitions():
    import math
    for N, want in EDGE_BIN.items():
        assert [min(max(math.floor((float(m) + 1.0) * (0.5 * N)), 0), N - 1) for m in EDGE_MU] == want


def edge_table():
    """Two table energies, eight outgoing energies of one cosine each (equal weights 1/8, sigma 1), each
    outgoing energy in a group of its own: the mass of cosine j is the only entry of group j."""
    t = sab_table(0, seed=1, NEi=2, NEo=8, NMU=1)
    t["ei"], t["sig"] = np.array([1e-9, 1e-6]), np.ones(2)
    t["threshold_inelastic"] = 1e-6
    t["e_out"] = np.tile(1e-8 * (1.0 + np.arange(8)), 2)
    t["mu"] = np.tile(EDGE_MU, 2)
    return t, 1e-8 * (0.5 + np.arange(9))


@pytest.mark.parametrize("N", (4, 8))
def test_every_edge_mass_sits_in_the_bin_the_definition_names(hip, N):
    t, bins = edge_table()
    # below the table: f = 0, the cosines are the table's own (1 * mu + 0 * mu)
    mat, el, inel, status = hip.sab_tab_batch(hip.Params.default(1, 2001), N, t, np.array([5e-10, 8e-10]), bins,
                                              want_parts=True, want_status=True)
    want = np.zeros((8, N))
    want[np.arange(8), EDGE_BIN[N]] = 0.125
    assert np.array_equal(inel[0], want) and np.array_equal(inel[1], want) and not el.any() and not status.any()
    assert np.array_equal(mat[0], want) and np.array_equal(ref.bin_of(EDGE_MU, N), EDGE_BIN[N])


# ---- a cosine that is not finite -------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_nan_cosine_is_dropped_and_flagged_where_it_was_read(hip, mode):
    N, row = 7, 9
    clean = table(mode, None)
    t = dict(clean)
    e = grid(mode, None)
    ei = clean["ei"]
    if mode == 2:
        at = int(clean["cptr"][row]) + 4                       # an interior outgoing point of table row 9
        mu = clean["cmu"].copy()
        mu[at * clean["NMU"] + 2] = np.nan
        t["cmu"] = mu
        pdfw = clean["cpdf"][at] * (clean["ce_out"][at + 1] - clean["ce_out"][at])
        assert BINS[0] < clean["ce_out"][at] < BINS[-1] and pdfw > 0
    else:
        io = 5
        mu = clean["mu"].copy()
        mu[(row * clean["NEo"] + io) * clean["NMU"] + 2] = np.nan
        t["mu"] = mu
    read = (e >= ei[row - 1]) & (e < ei[row + 1])               # the brackets that hold table row 9
    assert 2 <= read.sum() < len(e) - 2
    p = hip.Params.default(1, 2001)
    mat, el, inel, status = hip.sab_tab_batch(p, N, t, e, BINS, want_parts=True, want_status=True)
    base = gpu(hip, mode, None, N)
    _, _, rinel, rstatus = ref.sab_tab(t, e, BINS, N)
    assert np.array_equal(status, rstatus)
    assert np.array_equal(status != 0, read) and (status[read] == hip.ST_NONFINITE).all()
    keep = ~read
    keep[-1] = keep[-2]                                       # the last row of scatt_mat copies its neighbour
    assert np.array_equal(inel[~read], base[2][~read]) and np.array_equal(mat[keep], base[0][keep])
    check_against(inel, rinel, bars(clean)[0], f"mode {mode} NaN cosine inel")
    # the Legendre path counts the mass (P0 of a NaN cosine is 1): the bins fall short of it by that mass
    _, _, linel = hip.sab_batch(p, t, e, BINS, want_parts=True)
    short = linel[:, :, 0] - inel.sum(axis=2)
    scale = tabular_ref.p0_scale(linel[:, :, 0])
    assert (np.abs(short[~read]) <= bars(clean)[0] * scale[~read, None]).all()
    lost = short[read].sum(axis=1)
    print(f"mode {mode}: {read.sum()} E_in read the NaN cosine; missing mass {lost}")
    if mode == 2:
        assert (lost > 0).any() and (lost >= -bars(clean)[0] * scale[read]).all()
    else:
        w = ref.weights(clean)[io]
        isab = ref.bracket(ei, e[read])
        f = (e[read] - ei[isab - 1]) / (ei[isab] - ei[isab - 1])
        sig = (1.0 - f) * clean["sig"][isab - 1] + f * clean["sig"][isab]
        assert (np.abs(lost - sig * w) <= bars(clean)[0] * scale[read]).all()


# ---- edge energies ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,NEo", [(0, 16), (1, 16), (1, 5), (2, 16)])
def test_edge_energies(hip, mode, NEo):
    t = sab_table(mode, seed=77, NEo=NEo, elastic="incoherent")
    ei, thr = t["ei"], t["threshold_inelastic"]
    e = np.array([0.5 * ei[0], ei[0], ei[7], 0.5 * (ei[7] + ei[8]), thr, np.nextafter(thr, 1.0), 1.5 * thr])
    N = 7
    p = hip.Params.default(1, 2001)
    mat, el, inel, status = hip.sab_tab_batch(p, N, t, e, BINS, want_parts=True, want_status=True)
    rmat, rel, rinel, rstatus = ref.sab_tab(t, e, BINS, N)
    bar_in, bar_el = bars(t)
    check_against(inel, rinel, bar_in, f"mode {mode} NEo {NEo} inel")
    check_against(el, rel, bar_el, f"mode {mode} NEo {NEo} el")
    check_against(mat, rmat, bar_in, f"mode {mode} NEo {NEo} scatt_mat")
    assert np.array_equal(status, rstatus) and not status.any()
    assert inel[0].any() and inel[1].any() and not inel[5].any() and not inel[6].any()
    assert inel[4].any() == (mode != 2)          # E_in == threshold: the discrete modes take the last row
    assert np.array_equal(mat[-1], mat[-2])
    one = hip.sab_tab_batch(p, 1, t, e, BINS, want_parts=True)
    leg = hip.sab_batch(p, t, e, BINS, want_parts=True)
    assert all(np.array_equal(a, b) for a, b in zip(one, leg))


def test_two_calls_give_the_same_bits(hip):
    p = hip.Params.default(1, 2001)
    for mode in MODES:
        t, e = table(mode, "incoherent"), grid(mode, "incoherent")
        a = hip.sab_tab_batch(p, 128, t, e, BINS, want_parts=True, want_status=True)
        b = gpu(hip, mode, "incoherent", 128)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the driver ------------------------------------------------------------------------------
def set_tag(run, tag, value):
    f = Path(run) / "ndpp.xml"
    s = re.sub(rf"\s*<{tag}>.*?</{tag}>", "", f.read_text(), flags=re.S)
    f.write_text(s.replace("</ndpp>", f"  <{tag}>{value}</{tag}>\n</ndpp>"))


def test_driver_writes_a_thermal_table_in_bins(hip, tmp_path):
    """two tables, the fissionable nuclide and the continuous thermal table of the second end-to-end
    case, scatt_type tabular with 8 bins"""
    from ndpp_amd import grid as host_grid, reader, run as drv
    run = tmp_path / "run"
    ace_synth.write_inputs_multi(run, case2_tables()[:2], CASE2["bins"], scatt_order=CASE2["scatt_order"],
                                 mu_bins=CASE2["mu_bins"], threads=1, extend_pts=CASE2["extend_pts"],
                                 inel_extend_pts=CASE2["inel_extend_pts"], integrate_chi=True, freegas_cutoff_kT=0.0)
    set_tag(run, "scatt_type", "tabular")
    set_tag(run, "scatt_order", "8")
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), "--thermal-tabular", "--json",
                        str(tmp_path / "run.json")], cwd=ROOT, capture_output=True, text=True, timeout=250)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    name = CASE2["thermal"][0][0]
    data = (run / f"{name}.g7").read_bytes()
    m = reader.read_binary(data)
    assert m.scatt_type == 1 and m.scatt_order == 8 and m.elastic.mat.shape[2] == 8 and not m.nuscatter
    assert not m.chi_present and m.inelastic is None
    assert (m.elastic.mat >= 0).all()
    sums = m.elastic.mat.sum(axis=(1, 2))
    assert (sums > 0).sum() > 10 and (np.abs(sums[sums > 0] - 1.0) <= 1e-14).all()
    s = drv.read_ndpp_xml(run)
    tables = drv.load_tables(s, drv.read_cross_sections(s["cross_sections"]))
    p, o, bins = drv.params_of(s), drv.options_of(s), s["energy_bins"]
    d = tables[1]["data"]
    ein = host_grid.add_one_more_point(hip.sab_egrid_lib(p, d, bins))
    res = dict(ein_el=ein, el_mat=hip.sab_tab_batch(p, 8, d, ein, bins), ein_inel=None, inel_mat=None, nuinel_mat=None)
    fin, _ = hip.finish_scatt(o, res, bins)
    assert np.array_equal(m.elastic.ein, fin["ein_el"]) and np.array_equal(m.elastic.mat, fin["el_mat"])
    assert data == hip.nuclide_file(o, d["name"], d["kT"], fin, bins, is_sab=2)
    rec = json.loads((tmp_path / "run.json").read_text())["tables"]
    assert [t["kind"] for t in rec] == ["neutron", "thermal"] and rec[1]["bins"] == 8 and rec[1]["device_ms"] > 0
    v = subprocess.run([sys.executable, "-m", "ndpp_amd.validate", str(run)], cwd=ROOT, capture_output=True, text=True,
                       timeout=200)
    print(v.stdout[-2000:], v.stderr[-2000:])
    assert v.returncode == 0 and v.stdout.count("tabular") == 2
