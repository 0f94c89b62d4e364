"""CPU: the standalone driver's input side (ndpp_amd.run) -- ndpp.xml / cross_sections.xml with
the reference's defaults and refusals, ndpp_lib.xml from the parsed inputs against the reference
executable's (tests/golden/e2e), and the exit statuses: 2 on an input error, 3 without a device,
nothing written in either case."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from test_e2e_reference import CASE, e2e_nuclide, write_case2

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "e2e"


def case1(run):
    ace_synth.write_inputs(run, CASE["name"], e2e_nuclide(), scatt_order=CASE["scatt_order"], mu_bins=CASE["mu_bins"],
                           extend_pts=CASE["extend_pts"], inel_extend_pts=CASE["inel_extend_pts"], threads=1)
    return run


def drive(run, *extra, timeout=250):
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), *extra], cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    return r.returncode, r.stdout + r.stderr


def listing(run):
    return sorted(p.name for p in Path(run).iterdir())


def set_tag(run, tag, value):
    """replace (or add) <tag> in ndpp.xml; value None removes it"""
    f = Path(run) / "ndpp.xml"
    s = re.sub(rf"\s*<{tag}>.*?</{tag}>", "", f.read_text(), flags=re.S)
    if value is not None:
        s = s.replace("</ndpp>", f"  <{tag}>{value}</{tag}>\n</ndpp>")
    f.write_text(s)


def test_defaults_and_values_of_ndpp_xml(tmp_path):
    from ndpp_amd import run
    r = case1(tmp_path / "run")
    s = run.read_ndpp_xml(r)
    assert s["scatt_type"] == "legendre" and s["scatt_order"] == 5 and s["nuscatter"] and not s["integrate_chi"]
    assert s["mu_bins"] == 513 and s["extend_pts"] == 10 and s["inel_extend_pts"] == 5 and s["print_tol"] == 1e-10
    assert s["library_name"] == ".g2" and s["lib_format"] == 2 and s["thin_tol"] == 0.0
    assert np.array_equal(s["energy_bins"], e2e_nuclide()["bins"])
    for tag in ("scatt_type", "scatt_order", "nuscatter", "integrate_chi", "output_format", "print_tol", "mu_bins",
                "threads", "freegas_cutoff", "extend_pts", "inel_extend_pts", "thinning_tol"):
        set_tag(r, tag, None)
    s = run.read_ndpp_xml(r)
    for k, v in run.DEFAULTS.items():
        if k not in ("output_format", "freegas_cutoff"):
            assert s[k] == v, k
    assert s["freegas_cutoff"] == 400.0 and s["output_format"] == "binary"
    set_tag(r, "freegas_cutoff", "-1")
    set_tag(r, "thinning_tol", "2.5")
    set_tag(r, "scatt_type", "TABULAR")
    set_tag(r, "scatt_order", "64")
    set_tag(r, "adaptive_mu_its", "9")
    set_tag(r, "sab_epts_per_bin", "0")
    set_tag(r, "threads", "64")
    s = run.read_ndpp_xml(r)
    assert s["freegas_cutoff"] == float("inf") and s["thin_tol"] == 0.025 and s["scatt_type"] == "tabular"
    p = run.params_of(s)
    assert p.adaptive_mu_its == 9 and p.sab_epts_per_bin == 0 and p.mu_bins == 2001 and p.order == 1
    xs = run.read_cross_sections(s["cross_sections"])
    assert xs["filetype"] == "ascii" and len(xs["listings"]) == 1
    lst = xs["listings"][0]
    assert lst["type"] == "neutron" and lst["freegas_cutoff"] == -2.0 and lst["path"].endswith("synth.ace")


def test_per_table_freegas_cutoff_attribute(tmp_path):
    from ndpp_amd import run
    r = case1(tmp_path / "run")
    xml = r / "cross_sections.xml"
    base = xml.read_text()
    for attr, want in (("", 4.0), ('freegas_cutoff="-2"', 4.0), ('freegas_cutoff="7.5"', 7.5),
                       ('freegas_cutoff="-1"', None)):
        xml.write_text(base.replace('zaid="92238"', f'zaid="92238" {attr}'))
        s = run.read_ndpp_xml(r)
        t = run.load_tables(s, run.read_cross_sections(s["cross_sections"]))[0]
        fc = t["data"]["freegas_cutoff"]
        assert fc == float("inf") if want is None else fc == want * t["data"]["kT"]
    xml.write_text(base.replace('zaid="92238"', 'zaid="92238" freegas_cutoff="-3"'))
    s = run.read_ndpp_xml(r)
    with pytest.raises(run.InputError, match="freegas_cutoff"):
        run.read_cross_sections(s["cross_sections"])


def test_lib_xml_from_the_parsed_inputs_equals_the_reference_executables(hip, tmp_path):
    from ndpp_amd import run
    for make, gold in ((case1, GOLD / "ndpp_lib.xml"), (write_case2, GOLD / "chi_sab" / "ndpp_lib.xml")):
        r = tmp_path / gold.parent.name
        make(r)
        s = run.read_ndpp_xml(r)
        tables = run.load_tables(s, run.read_cross_sections(s["cross_sections"]))
        got = run.lib_xml_of(s, r, tables).decode()
        assert got == gold.read_text().replace("RUNDIR", str(r.resolve()))
        assert [t["file"] for t in tables] == [re.search(r'path="([^"]+)"', ln).group(1)
                                              for ln in gold.read_text().splitlines() if "<ndpp_table" in ln]


@pytest.mark.parametrize("tag,value,msg", [
    ("output_format", "hdf5", "hdf5 is not supported"),
    ("output_format", "HUMAN", "human is not supported"),
    ("scatt_order", "0", "Invalid negative or zero scatt_order"),
    ("scatt_order", "11", "Legendre orders go up to 10"),
    ("mu_bins", "1", "Mu_bins must be two or greater"),
    ("energy_bins", "1e-11 1.0 20.0", "Bottom of Lowest Group"),
    ("energy_bins", "0.0 1.0 1.0 20.0", "increasing order"),
    ("energy_bins", None, "No energy group structure"),
    ("freegas_cutoff", "-5", "Invalid negative value of <freegas_cutoff>"),
    ("adaptive_mu_its", "-1", "adaptive_mu_its"),
    ("adaptive_eout_its", "40", "0..31"),
    ("extend_pts", "-2", "extend_pts"),
    ("scatt_order", "five", "not an integer"),
])
def test_bad_ndpp_xml_exits_2_and_writes_nothing(tmp_path, tag, value, msg):
    r = case1(tmp_path / "run")
    set_tag(r, tag, value)
    before = listing(r)
    rc, out = drive(r)
    assert rc == 2 and msg in out, out
    assert listing(r) == before


def test_bad_inputs_exit_2_and_write_nothing(tmp_path):
    r = case1(tmp_path / "run")
    before = listing(r)
    ace = r / "synth.ace"
    good = ace.read_text()
    lines = good.splitlines(keepends=True)
    ace.write_text("".join(lines[:40]))                               # truncated XSS
    rc, out = drive(r)
    assert rc == 2 and "92238.71c: XSS" in out and "truncated" in out, out
    ace.write_text(good.replace("92238.71c", "92235.71c", 1))          # the listing finds another table
    rc, out = drive(r)
    assert rc == 2 and "92235.71c' found at location 1 instead" in out, out
    ace.write_text(good)
    xs = r / "cross_sections.xml"
    xs.write_text(xs.read_text().replace("<filetype>ascii</filetype>", "<filetype>hdf5</filetype>"))
    rc, out = drive(r)
    assert rc == 2 and "Unknown filetype" in out, out
    xs.unlink()
    rc, out = drive(r)
    assert rc == 2 and "does not exist" in out, out
    assert listing(r) == [n for n in before if n != "cross_sections.xml"]


def test_tabular_with_a_thermal_table_exits_2_before_any_device_work(tmp_path):
    r = tmp_path / "run"
    write_case2(r)
    set_tag(r, "scatt_type", "tabular")
    set_tag(r, "scatt_order", "8")
    before = listing(r)
    rc, out = drive(r)
    assert rc == 2 and "tabular output of thermal S(alpha,beta) tables is not supported" in out, out
    assert listing(r) == before


def test_without_a_device_exit_3_and_no_partial_files(hip, tmp_path):
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a device is present: the GPU tests run the driver to completion")
    for make in (case1, write_case2):
        r = tmp_path / make.__name__
        make(r)
        before = listing(r)
        rc, out = drive(r, "--json", str(tmp_path / f"{make.__name__}.json"))
        assert rc == 3 and "NDPP_EDEVICE" not in out and "error -5" in out, out
        assert listing(r) == before and not (tmp_path / f"{make.__name__}.json").exists()
