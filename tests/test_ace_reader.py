"""CPU: the ACE reader (ndpp_amd.ace) against the tables tests/ace_synth.py writes -- every array
equal bit for bit to the quantised dicts, ASCII and binary, several tables in one file picked by
`location` -- and its refusals of broken tables; the grids the host builds from the parsed tables
(sab_egrid_lib, chi_egrid_lib) equal the ones the reference executable wrote (tests/golden/e2e)."""
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from test_e2e_reference import CASE, CASE2, case2_tables, chi_inputs, e2e_fissionable, e2e_nuclide

GOLD = Path(__file__).resolve().parent / "golden" / "e2e"


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _same_law(got, want):
    assert got["law"] == want["law"]
    assert _same(got["data"], want["data"]) and _same(got["pv_x"], want["pv_x"]) and _same(got["pv_y"], want["pv_y"])
    for k in ("pv_nbt", "pv_int"):
        assert list(got.get(k) or []) == list(want.get(k) or []), k


def _same_adist(got, want):
    """ace_synth's angular data start with one pad word (locations are offsets into it); the
    reader returns XSS as it is, so its locations are one smaller where they point at a table"""
    if want is None:
        assert got is None
        return
    e, t, loc, data = want
    ge, gt, gloc, gdata = got
    assert _same(ge, e) and _same(gt, t)
    assert _same(gloc, np.where(np.asarray(loc) != 0, np.asarray(loc) - 1, 0))
    assert _same(gdata, np.asarray(data)[1:])


def check_neutron(got, want):
    for k in ("awr", "kT"):
        assert got[k] == want[k], k
    assert _same(got["energy"], want["energy"]) and _same(got["elastic"], want["elastic"])
    by_mt = {r["MT"]: r for r in got["reactions"]}
    assert sorted(by_mt) == sorted(r["MT"] for r in want["reactions"])
    assert got["reactions"][0]["MT"] == 2
    for w in want["reactions"]:
        g = by_mt[w["MT"]]
        for k in ("Q", "mult", "thr", "in_cm"):
            assert g[k] == w[k], (w["MT"], k)
        assert (g["sigma"] is None) == (w["sigma"] is None) and (w["sigma"] is None or _same(g["sigma"], w["sigma"]))
        if w["mult"] != 0:
            _same_adist(g["adist"], w["adist"])
            assert len(g["edists"]) == len(w["edists"]), w["MT"]
            for ge, we in zip(g["edists"], w["edists"]):
                _same_law(ge, we)
    if want.get("nu") is None:
        assert not got["fissionable"] or got["nu"] is None
        return
    nu, gnu = want["nu"], got["nu"]
    for k in ("nu_t_type", "nu_d_type", "n_prec"):
        assert gnu[k] == nu[k], k
    for k in ("nu_t_data", "nu_d_data", "prec_data"):
        assert _same(gnu[k], nu[k]), k
    assert len(gnu["delayed"]) == len(nu["delayed"])
    for ge, we in zip(gnu["delayed"], nu["delayed"]):
        _same_law(ge, we)


def check_thermal(got, want):
    for k in ("awr", "kT", "threshold_inelastic", "threshold_elastic", "NEi", "NMU", "mode", "NEe", "NMUe"):
        assert got[k] == want[k], k
    for k in ("ei", "sig"):
        assert _same(got[k], want[k]), k
    if want["mode"] in (0, 1):
        assert got["NEo"] == want["NEo"]
        for k in ("e_out", "mu"):
            assert _same(got[k], want[k]), k
    else:
        assert _same(got["cptr"], want["cptr"])
        for k in ("ce_out", "cpdf", "cmu"):
            assert _same(got[k], want[k]), k
    if want["NEe"] > 0:
        assert got["el_mode"] == want["el_mode"]
        for k in ("ee", "eP") + (("emu",) if want["NMUe"] > 0 else ()):
            assert _same(got[k], want[k]), k


def write_all(path):
    """the U-238-like nuclide, then the four CASE2 tables, in ONE ASCII file: [(kind, name, dict, location)]"""
    out = [("neutron", CASE["name"], e2e_nuclide(), ace_synth.write_ace(path, CASE["name"], e2e_nuclide()))]
    for tb in case2_tables():
        if tb["kind"] == "neutron":
            loc = ace_synth.write_ace(path, tb["name"], tb["data"], zaid=tb["zaid"], append=True)
        else:
            loc = ace_synth.write_thermal_ace(path, tb["name"], tb["data"], zaids=(tb["zaid"],), append=True)
        out.append((tb["kind"], tb["name"], tb["data"], loc))
    return out


def test_round_trip_ascii_tables_picked_by_location(tmp_path):
    from ndpp_amd import ace
    f = tmp_path / "lib.ace"
    tabs = write_all(f)
    assert [t[3] for t in tabs][0] == 1 and len({t[3] for t in tabs}) == len(tabs)
    for kind, name, want, loc in reversed(tabs):          # any order: each table is found by its line
        t = ace.read_table(f, loc, expect_name=name)
        assert t.name == "%10s" % name and t.kind == kind
        if kind == "neutron":
            got = ace.neutron(t)
            check_neutron(got, want)
            assert got["fissionable"] == (want.get("nu") is not None)
        else:
            check_thermal(ace.thermal(t), want)


def test_round_trip_binary_equals_ascii(tmp_path):
    from ndpp_amd import ace
    f = tmp_path / "lib.ace"
    tabs = write_all(f)
    ascii_tables = [ace.read_table(f, loc, expect_name=name) for _, name, _, loc in tabs]
    b = tmp_path / "lib.bin"
    locs = ace.write_binary(b, ascii_tables, record_length=4096, entries=512)
    for (kind, name, want, _), t, loc in zip(tabs, ascii_tables, locs):
        bt = ace.read_table(b, loc, "binary", 4096, 512, expect_name=name)
        assert bt.name == t.name and bt.awr == t.awr and bt.kT == t.kT and bt.nxs == t.nxs and bt.jxs == t.jxs
        assert _same(bt.xss, t.xss)
        if kind == "neutron":
            check_neutron(ace.neutron(bt), want)
        else:
            check_thermal(ace.thermal(bt), want)


def test_chi_inputs_of_the_parsed_table_equal_the_test_layout(tmp_path):
    """chi_case of the parsed fissionable table == tests' chi_inputs of the dict it was written from"""
    from ndpp_amd import ace
    f = tmp_path / "pu.ace"
    c = e2e_fissionable()
    ace_synth.write_ace(f, CASE2["fiss"], c, zaid=94239)
    got = ace.chi_case(ace.neutron(ace.read_table(f, 1)))
    want = chi_inputs(c)
    for k in ("n_grid", "nu_t_type", "nu_d_type", "n_prec", "mts", "thr", "nnest"):
        assert got[k] == want[k], k
    for k in ("energy", "fission", "nu_t_data", "nu_d_data", "prec_data"):
        assert _same(got[k], want[k]), k
    for gs, ws in zip(got["sig"], want["sig"]):
        assert _same(gs, ws)
    for (gl, gd, ge), (wl, wd, we) in zip(got["spectra"] + got["delayed"], want["spectra"] + want["delayed"]):
        assert gl == wl and _same(gd, wd)
        _same_law(ge, we)


def test_grids_of_the_parsed_tables_equal_the_reference_executables(hip, tmp_path):
    """chi_egrid_lib and sab_egrid_lib (+ the extra top point) on the parsed CASE2 tables give the
    incoming grids the reference executable wrote into tests/golden/e2e/chi_sab, bit for bit"""
    from ndpp_amd import ace, reader
    f = tmp_path / "lib.ace"
    tabs = write_all(f)
    p = hip.Params.default(CASE2["scatt_order"] + 1, CASE2["mu_bins"])
    p.extend_pts, p.inel_extend_pts = CASE2["extend_pts"], CASE2["inel_extend_pts"]
    for kind, name, _, loc in tabs[1:]:
        t = reader.read_binary((GOLD / "chi_sab" / f"{name}.g7").read_bytes())
        if kind == "neutron":
            got = hip.chi_egrid_lib(ace.chi_case(ace.neutron(ace.read_table(f, loc))))
            assert _same(got, t.chi["e_grid"])
        else:
            got = hip.add_one_more_point(hip.sab_egrid_lib(p, ace.thermal(ace.read_table(f, loc)), CASE2["bins"]))
            assert _same(got, t.elastic.ein)


# ---- refusals ------------------------------------------------------------------------------------
def _one(tmp_path):
    f = tmp_path / "u.ace"
    ace_synth.write_ace(f, CASE["name"], e2e_nuclide())
    return f


def test_truncated_xss_is_refused(tmp_path):
    from ndpp_amd import ace
    f = _one(tmp_path)
    lines = f.read_text().splitlines(keepends=True)
    f.write_text("".join(lines[:len(lines) // 2]))
    with pytest.raises(ValueError, match=r"92238\.71c: XSS: .*truncated"):
        ace.read_table(f, 1, expect_name=CASE["name"])


def test_pointer_outside_xss_is_refused(tmp_path):
    from ndpp_amd import ace
    t = ace.read_table(_one(tmp_path), 1)
    t.jxs[10] = len(t.xss) + 7                              # DLW past the end
    with pytest.raises(ValueError, match=r"92238\.71c: DLW.*outside XSS"):
        ace.neutron(t)
    t = ace.read_table(_one(tmp_path), 1)
    t.xss[t.jxs[5] - 1] = 1e6                               # a LSIG locator far outside SIG
    with pytest.raises(ValueError, match=r"92238\.71c: SIG"):
        ace.neutron(t)


def test_wrong_name_location_and_binary_settings_are_refused(tmp_path):
    from ndpp_amd import ace
    f = _one(tmp_path)
    with pytest.raises(ValueError, match="found at location 1 instead"):
        ace.read_table(f, 1, expect_name="1001.71c")
    with pytest.raises(ValueError, match="header"):
        ace.read_table(f, 10 ** 6, expect_name=CASE["name"])
    with pytest.raises(ValueError, match="record_length"):
        ace.read_table(f, 1, "binary", 0, 0)
    with pytest.raises(ValueError, match="unknown filetype"):
        ace.read_table(f, 1, "hdf5")


def test_corrupt_thermal_mode_is_refused(tmp_path):
    from ndpp_amd import ace
    f = tmp_path / "t.ace"
    tb = case2_tables()[1]
    ace_synth.write_thermal_ace(f, tb["name"], tb["data"])
    t = ace.read_table(f, 1)
    t.nxs[6] = 7
    with pytest.raises(ValueError, match=r"hh2o\.10t: NXS: secondary mode"):
        ace.thermal(t)
