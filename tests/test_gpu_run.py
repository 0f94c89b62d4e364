"""GPU: the standalone driver `python -m ndpp_amd.run` end to end, in a fresh child process under a
time limit, on the run directories tests/ace_synth.py writes for the two end-to-end cases --
against what the reference executable wrote (tests/golden/e2e, the bars of test_e2e_reference),
against the per-table chain of the C ABI on the same parsed tables (byte for byte), and in
tabular mode through `python -m ndpp_amd.validate`."""
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from conftest import scale_rel_err
from test_e2e_reference import CASE, CASE2, case2_tables, e2e_nuclide, write_case2

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "e2e"
pytestmark = pytest.mark.gpu


def drive(run, *extra, timeout=270):
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), *extra], cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r.returncode


def set_tag(run, tag, value):
    f = Path(run) / "ndpp.xml"
    s = re.sub(rf"\s*<{tag}>.*?</{tag}>", "", f.read_text(), flags=re.S)
    f.write_text(s.replace("</ndpp>", f"  <{tag}>{value}</{tag}>\n</ndpp>"))


def compare_section(a, b, label):
    assert np.array_equal(a.ein, b.ein) and np.array_equal(a.group_index, b.group_index), label
    err = scale_rel_err(a.mat, b.mat)
    diff = float(np.mean((a.gmin != b.gmin) | (a.gmax != b.gmax)))
    print(f"{label}: {len(a.ein)} E_in, moments vs the reference executable {err:.2e}, rows with another extent {diff:.3f}")
    assert err < 1e-10 and diff < 0.02, label


def test_gpu_driver_against_the_reference_executable_u238(tmp_path):
    from ndpp_amd import reader
    run = tmp_path / "run"
    ace_synth.write_inputs(run, CASE["name"], e2e_nuclide(), scatt_order=CASE["scatt_order"], mu_bins=CASE["mu_bins"],
                           extend_pts=CASE["extend_pts"], inel_extend_pts=CASE["inel_extend_pts"], threads=1)
    assert drive(run, "--json", str(tmp_path / "run.json")) == 0
    raw = (GOLD / f"{CASE['name']}.g2").read_bytes()
    mine = (run / f"{CASE['name']}.g2").read_bytes()
    t, m = reader.read_binary(raw), reader.read_binary(mine)
    assert mine[:64] == raw[:64]
    for name in ("elastic", "inelastic", "nuinelastic"):
        compare_section(getattr(m, name), getattr(t, name), f"driver {name}")
    assert (run / "ndpp_lib.xml").read_text() == (GOLD / "ndpp_lib.xml").read_text().replace("RUNDIR", str(run.resolve()))
    rep = json.loads((tmp_path / "run.json").read_text())
    assert len(rep["tables"]) == 1 and rep["tables"][0]["kind"] == "neutron"
    r0 = rep["tables"][0]
    assert r0["energies"] == dict(elastic=len(t.elastic.ein), inelastic=len(t.inelastic.ein))
    assert r0["batch"]["call"] == "scatt_library" and r0["batch"]["device_ms"] > 0 and r0["batch"]["wall_s"] > 0


def test_gpu_ein_grids_of_the_parsed_table_against_the_reference_executable(hip, tmp_path):
    """create_ein_grid on the ScattData grids of the parsed ACE table (convert_distro per reaction
    and law) gives both incoming grids the reference executable wrote, bit for bit"""
    from ndpp_amd import ace, reader
    f = tmp_path / "u.ace"
    c = e2e_nuclide()
    ace_synth.write_ace(f, CASE["name"], c)
    n = ace.neutron(ace.read_table(f, 1, expect_name=CASE["name"]))
    p = hip.Params.default(CASE["scatt_order"] + 1, CASE["mu_bins"])
    p.extend_pts, p.inel_extend_pts = CASE["extend_pts"], CASE["inel_extend_pts"]
    sds, thr = [], 20.0
    for r in n["reactions"]:
        for ed in (r["edists"] or [None]):
            a = hip.AceReaction.make(r["MT"], ed["law"] if ed else 0, r["adist"], ed["data"] if ed else None,
                                     n["energy"][r["thr"] - 1])
            cd = hip.convert_distro(a, c["bins"], CASE["mu_bins"])
            sds.append((cd is not None, r["MT"], r["Q"], cd["e_grid"] if cd is not None else np.zeros(1)))
            if cd is not None and r["MT"] != 2:
                thr = min(thr, n["energy"][r["thr"] - 1])
    el, inel = hip.create_ein_grid(p, sds, c["bins"], n["energy"], n["awr"], n["kT"], 4.0 * n["kT"], thr)
    t = reader.read_binary((GOLD / f"{CASE['name']}.g2").read_bytes())
    assert np.array_equal(el, t.elastic.ein) and np.array_equal(inel, t.inelastic.ein)


def test_gpu_driver_against_the_reference_executable_chi_and_thermal(tmp_path):
    from ndpp_amd import reader
    run = tmp_path / "run"
    write_case2(run)
    assert drive(run, "--json", str(tmp_path / "run.json")) == 0
    raw = (GOLD / "chi_sab" / f"{CASE2['fiss']}.g7").read_bytes()
    mine = (run / f"{CASE2['fiss']}.g7").read_bytes()
    t, m = reader.read_binary(raw), reader.read_binary(mine)
    assert m.chi_present and np.array_equal(m.chi["e_grid"], t.chi["e_grid"])
    compare_section(m.elastic, t.elastic, "driver fissionable elastic")
    e_chi = max(scale_rel_err(m.chi["total"], t.chi["total"]), scale_rel_err(m.chi["prompt"], t.chi["prompt"]),
                max(scale_rel_err(m.chi["delayed"][j], t.chi["delayed"][j]) for j in range(3)))
    print(f"driver chi vs the reference executable {e_chi:.2e}")
    assert e_chi < 1e-10 and len(mine) == len(raw)
    for name, _, _ in CASE2["thermal"]:
        raw = (GOLD / "chi_sab" / f"{name}.g7").read_bytes()
        mine = (run / f"{name}.g7").read_bytes()
        assert mine[:114] == raw[:114]
        compare_section(reader.read_binary(mine).elastic, reader.read_binary(raw).elastic, f"driver thermal {name}")
    want = (GOLD / "chi_sab" / "ndpp_lib.xml").read_text().replace("RUNDIR", str(run.resolve()))
    assert (run / "ndpp_lib.xml").read_text() == want
    rep = json.loads((tmp_path / "run.json").read_text())
    assert [r["kind"] for r in rep["tables"]] == ["neutron", "thermal", "thermal", "thermal"]
    assert rep["tables"][0]["chi"]["energies"] == len(t.chi["e_grid"])
    assert all(r["device_ms"] > 0 for r in rep["tables"][1:])


def multi_run(run, fmt, nuscatter):
    """one library batch with two neutron tables (the U-238-like nuclide and the fissionable one)
    and the three thermal tables, at the CASE2 settings"""
    tabs = case2_tables()
    tabs.insert(1, dict(kind="neutron", name=CASE["name"], alias="Synth-1", data=e2e_nuclide(), zaid=92238))
    ace_synth.write_inputs_multi(run, tabs, CASE2["bins"], scatt_order=CASE2["scatt_order"], mu_bins=CASE2["mu_bins"],
                                 threads=1, extend_pts=CASE2["extend_pts"], inel_extend_pts=CASE2["inel_extend_pts"],
                                 integrate_chi=True, freegas_cutoff_kT=4.0, nuscatter=nuscatter, output_format=fmt)


@pytest.mark.parametrize("fmt,nuscatter", [("binary", True), ("binary", False), ("ascii", True), ("ascii", False)])
def test_gpu_driver_equals_the_per_table_chain(hip, tmp_path, fmt, nuscatter):
    """the driver's files == scatt_nuclide -> finish_scatt -> nuclide_file (+ chi_batch) and
    sab_batch -> finish_scatt -> nuclide_file on the same parsed tables, byte for byte"""
    from ndpp_amd import ace, grid, run as drv
    run = tmp_path / "run"
    multi_run(run, fmt, nuscatter)
    assert drive(run, "--json", str(tmp_path / "run.json")) == 0
    s = drv.read_ndpp_xml(run)
    tables = drv.load_tables(s, drv.read_cross_sections(s["cross_sections"]))
    p, o, bins = drv.params_of(s), drv.options_of(s), s["energy_bins"]
    assert [t["kind"] for t in tables].count("neutron") == 2
    for t in tables:
        d = t["data"]
        if t["kind"] == "neutron":
            r = hip.scatt_nuclide(p, d, bins, nuscatt=nuscatter)
            chi = None
            if d["fissionable"]:
                case = ace.chi_case(d)
                e = hip.chi_egrid_lib(case)
                chi = (e,) + tuple(hip.chi_batch(case, bins, e))
            fin, _ = hip.finish_scatt(o, r, bins)
            want = hip.nuclide_file(o, d["name"], d["kT"], fin, bins, chi=chi)
        else:
            ein = grid.add_one_more_point(hip.sab_egrid_lib(p, d, bins))
            res = dict(ein_el=ein, el_mat=hip.sab_batch(p, d, ein, bins), ein_inel=None, inel_mat=None, nuinel_mat=None)
            fin, _ = hip.finish_scatt(o, res, bins)
            want = hip.nuclide_file(o, d["name"], d["kT"], fin, bins, is_sab=True)
        got = (run / t["file"]).read_bytes()
        print(f"{fmt} nuscatter={nuscatter} {t['file']}: {len(got)} bytes, identical {got == want}")
        assert got == want, t["file"]
    assert len(json.loads((tmp_path / "run.json").read_text())["tables"]) == len(tables)


def test_gpu_tabular_run_validates(tmp_path):
    from ndpp_amd import reader
    run = tmp_path / "run"
    ace_synth.write_inputs(run, CASE["name"], e2e_nuclide(), scatt_order=CASE["scatt_order"], mu_bins=CASE["mu_bins"],
                           extend_pts=CASE["extend_pts"], inel_extend_pts=CASE["inel_extend_pts"], threads=1)
    set_tag(run, "scatt_type", "tabular")
    set_tag(run, "scatt_order", "8")
    assert drive(run, "--json", str(tmp_path / "run.json")) == 0
    m = reader.read_binary((run / f"{CASE['name']}.g2").read_bytes())
    assert m.scatt_type == 1 and m.scatt_order == 8 and m.elastic.mat.shape[2] == 8
    g = reader.read_binary((GOLD / f"{CASE['name']}.g2").read_bytes())
    assert np.array_equal(m.elastic.ein, g.elastic.ein) and np.array_equal(m.inelastic.ein, g.inelastic.ein)
    rep = json.loads((tmp_path / "run.json").read_text())
    assert len(rep["tables"]) == 1 and rep["tables"][0]["batch"]["call"] == "scatt_library_tab"
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.validate", str(run)], cwd=ROOT, capture_output=True,
                       text=True, timeout=200)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
