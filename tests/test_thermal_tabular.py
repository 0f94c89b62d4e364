"""Tabular output of thermal S(alpha,beta) tables, host side (no GPU): the checks of
ndpp_sab_tab_batch before the device is asked for, the no-device path, the writer's third is_sab
value read back with reader.py and through validate, the driver's --thermal-tabular inputs, and the
numpy restatement (tests/thermal_tab_ref.py) at one bin against the C oracle of the Legendre path."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import OracleParams, dp, oracle_params
from ndpp_amd import reader, validate
from synth import sab_ein_grid, sab_table
from test_e2e_reference import write_case2
from test_run_inputs import listing, set_tag

import thermal_tab_ref as ref

ROOT = Path(__file__).resolve().parent.parent
BINS = np.array([2e-9, 1e-8, 2.5e-8, 6e-8, 1.5e-7, 4e-7, 1e-6, 1e-6 * (1 + 1e-9), 2.5e-6, 5e-6])
EINVAL, EDEVICE = -22, -5


def call(hip, t, n_tab, ein=(1e-8, 1e-7), null_table=False):
    """ndpp_sab_tab_batch on table dict t; returns (code, message)"""
    lib = hip.load()
    p = hip.Params.default(1, 2001)
    p.order = -7                                     # not read: only n_tab sizes the rows
    flat = hip.SabFlat.from_dict(t)
    ein = np.array(ein)
    n = max(n_tab, 1)
    mat = np.zeros(len(ein) * (len(BINS) - 1) * n)
    rc = lib.ndpp_sab_tab_batch(C.byref(p), None if null_table else C.byref(flat), n_tab, len(ein), dp(ein),
                                len(BINS) - 1, dp(BINS), None, None, dp(mat), None)
    return rc, lib.ndpp_last_error().decode()


@pytest.mark.parametrize("n_tab", (0, 129))
def test_bin_count_outside_the_range_refused(hip, n_tab):
    rc, msg = call(hip, sab_table(0, 1), n_tab)
    assert rc == EINVAL and f"n_tab={n_tab} outside 1..128" in msg
    with pytest.raises(hip.NdppError, match="-22"):
        hip.sab_tab_batch(hip.Params.default(1, 2001), n_tab, sab_table(0, 1), [1e-8], BINS)


def test_bad_tables_refused_before_the_device(hip):
    rc, msg = call(hip, sab_table(0, 1), 8, null_table=True)
    assert rc == EINVAL and "NULL params/table" in msg
    bad = sab_table(0, 1)
    bad["mode"] = 7
    rc, msg = call(hip, bad, 8)
    assert rc == EINVAL and "secondary_mode=7" in msg
    rc, msg = call(hip, sab_table(1, 1, NEo=4), 8)
    assert rc == EINVAL and "skewed weighting needs more than 4 outgoing energies" in msg
    lib = hip.load()
    flat = hip.SabFlat.from_dict(sab_table(2, 1))
    flat.cont_ptr = None
    p, ein, mat = hip.Params.default(1, 2001), np.array([1e-8]), np.zeros(9 * 8)
    rc = lib.ndpp_sab_tab_batch(C.byref(p), C.byref(flat), 8, 1, dp(ein), 9, dp(BINS), None, None, dp(mat), None)
    assert rc == EINVAL and b"continuous mode without cont_ptr" in lib.ndpp_last_error()
    # as in ndpp_sab_batch: no energies is no work, and the arrays may then be absent
    assert lib.ndpp_sab_tab_batch(C.byref(p), C.byref(flat), 8, 0, None, 9, None, None, None, None, None) == 0
    flat = hip.SabFlat.from_dict(sab_table(0, 1))
    assert lib.ndpp_sab_tab_batch(C.byref(p), C.byref(flat), 8, 1, dp(ein), 9, dp(BINS), None, None, None,
                                  None) == EINVAL
    assert b"NULL array argument" in lib.ndpp_last_error()


def test_no_device_path(hip):
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a device is present: the compute path runs (tests/test_gpu_thermal_tabular.py)")
    for mode in (0, 1, 2):
        rc, _ = call(hip, sab_table(mode, 1, elastic="coherent"), 8)
        assert rc == EDEVICE
    with pytest.raises(hip.NdppError, match="-5"):
        hip.sab_tab_batch(hip.Params.default(1, 2001), 8, sab_table(0, 1), [1e-8], BINS, want_parts=True,
                          want_status=True)


# ---- the writer ------------------------------------------------------------------------------
N, G = 4, 4
NAME = "%10s" % "hh2o.71t"          # the A10 field of the ACE header line
WBINS = np.array([0.0, 1e-8, 1e-7, 1e-6, 20.0])


def thermal_result():
    """a thermal table's result: one section, rows normalised to 1 over groups and bins, one row empty"""
    m = np.zeros((3, G, N))
    m[0, 0] = [0.0, 0.125, 0.25, 0.125]
    m[0, 1] = [0.25, 0.0, 0.0, 0.25]
    m[1, 2] = [0.5, 0.25, 0.125, 0.125]
    return dict(ein_el=np.array([1e-9, 1e-7, 5e-6]), el_mat=m, ein_inel=None, inel_mat=None, nuinel_mat=None)


def opts(hip, fmt):
    return hip.OutputOptions(lib_format=fmt, scatt_type=1, scatt_order=N, nuscatter=1, integrate_chi=1, mu_bins=2001,
                             print_tol=0.0, thin_tol=0.0)


@pytest.mark.parametrize("fmt", ["binary", "ascii"])
def test_thermal_tabular_file_round_trip(hip, fmt, tmp_path, capsys):
    f = hip.FMT_BINARY if fmt == "binary" else hip.FMT_ASCII
    r = thermal_result()
    data = hip.nuclide_file(opts(hip, f), NAME, 2.53e-8, r, WBINS, is_sab=2)
    t = (reader.read_binary if fmt == "binary" else reader.read_ascii)(data)
    assert t.scatt_type == 1 and t.scatt_order == N and t.moments == N and t.groups == G
    assert not t.nuscatter and not t.chi_present
    assert np.array_equal(t.elastic.ein, r["ein_el"]) and np.array_equal(t.elastic.mat, r["el_mat"])
    assert list(t.elastic.gmin) == [1, 3, 0] and list(t.elastic.gmax) == [2, 3, 0]
    assert t.inelastic is None
    # is_sab = 1 is refused as before, and for Legendre output 1 and 2 write the same file
    with pytest.raises(hip.NdppError, match="S\\(alpha,beta\\)"):
        hip.nuclide_file(opts(hip, f), NAME, 2.53e-8, r, WBINS, is_sab=1)
    with pytest.raises(hip.NdppError, match="S\\(alpha,beta\\)"):
        hip.nuclide_file(opts(hip, f), NAME, 2.53e-8, r, WBINS, is_sab=True)
    leg = opts(hip, f)
    leg.scatt_type, leg.scatt_order = 0, N - 1
    assert hip.nuclide_file(leg, NAME, 2.53e-8, r, WBINS, is_sab=2) == \
        hip.nuclide_file(leg, NAME, 2.53e-8, r, WBINS, is_sab=1)
    # validate counts the thermal table's bins like any other tabular table's
    (tmp_path / "hh2o.71t.g4").write_bytes(data)
    (tmp_path / "ndpp_lib.xml").write_bytes(hip.lib_xml(
        str(tmp_path), f, [dict(alias="hh2o.71t", awr=0.99917, name="hh2o.71t", path="hh2o.71t.g4", kT=2.53e-8,
                                zaid=1001, metastable=0, freegas_cutoff=-2.0)], WBINS, 1, N, 2001, 1, 1, 0.0, 0.0))
    assert validate.main([str(tmp_path)]) == 0
    out = capsys.readouterr().out
    assert f"tabular, {G} groups, {N} bins" in out and f"rows {3 * G:7d}  negative       0" in out
    rep = validate.tab_positivity(t)
    assert rep.positive and rep.n_moments == N and rep.sections["elastic"].rows == 3 * G


# ---- the driver's inputs ---------------------------------------------------------------------
def drive(run, *extra):
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), *extra], cwd=ROOT, capture_output=True,
                       text=True, timeout=250)
    return r.returncode, r.stdout + r.stderr


def test_thermal_tabular_needs_a_tabular_run(tmp_path):
    r = tmp_path / "run"
    write_case2(r)
    before = listing(r)
    rc, out = drive(r, "--thermal-tabular")
    assert rc == 2 and "--thermal-tabular" in out and "input error" in out, out
    assert listing(r) == before


def test_a_tabular_run_without_the_flag_is_refused_as_before(tmp_path):
    r = tmp_path / "run"
    write_case2(r)
    set_tag(r, "scatt_type", "tabular")
    set_tag(r, "scatt_order", "8")
    before = listing(r)
    rc, out = drive(r)
    assert rc == 2 and "tabular output of thermal S(alpha,beta) tables is not supported" in out, out
    assert listing(r) == before


def test_with_the_flag_the_run_reaches_the_device(hip, tmp_path):
    """without a device the flagged run gets past the inputs and the refusal and stops at the first
    device call: exit 3, nothing written"""
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a device is present: tests/test_gpu_thermal_tabular.py runs the driver to completion")
    r = tmp_path / "run"
    write_case2(r)
    set_tag(r, "scatt_type", "tabular")
    set_tag(r, "scatt_order", "8")
    before = listing(r)
    rc, out = drive(r, "--thermal-tabular")
    assert rc == 3 and "error -5" in out and "not supported" not in out, out
    assert listing(r) == before


# ---- the restatement against the oracle of the Legendre path ----------------------------------
@pytest.mark.parametrize("elastic", (None, "coherent", "incoherent"))
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_restatement_at_one_bin_is_the_oracles_p0(oracle, hip, mode, elastic):
    """N = 1: every mass falls into the one bin, so the restatement must give the P0 of the C oracle of
    calc_scattsab (pinned to the Fortran by tests/golden/sab.npz) up to the order of its sums; and at
    any N the bins sum to it."""
    t = sab_table(mode, seed=1000 + mode, elastic=elastic)
    ein = sab_ein_grid(t)
    flat = hip.SabFlat.from_dict(t)
    G = len(BINS) - 1
    el, inel, mat = (np.zeros((len(ein), G, 1)) for _ in range(3))
    oracle.oracle_calc_scattsab.restype = C.c_int
    oracle.oracle_calc_scattsab.argtypes = [C.POINTER(OracleParams), C.c_void_p, C.c_int,
                                            C.POINTER(C.c_double), C.c_int] + [C.POINTER(C.c_double)] * 4
    p = oracle_params(oracle, 1, 2001)
    assert oracle.oracle_calc_scattsab(C.byref(p), C.byref(flat), len(ein), dp(ein), G, dp(BINS), dp(el), dp(inel),
                                       dp(mat)) == 0
    n_in, n_el = ref.masses_per_bin(t)
    for N in (1, 7):
        rmat, rel, rinel, status = ref.sab_tab(t, ein, BINS, N)
        assert not status.any()
        for got, want, n in ((rmat, mat, n_in), (rel, el, max(n_el, 1)), (rinel, inel, n_in)):
            scale = np.abs(want[:, :, 0]).max(axis=1)
            scale[scale == 0] = 1.0
            err = (np.abs(got.sum(axis=2) - want[:, :, 0]) / scale[:, None]).max()
            assert err <= 4 * n * 2.0 ** -53
            assert np.array_equal(got.sum(axis=2) == 0, want[:, :, 0] == 0)
