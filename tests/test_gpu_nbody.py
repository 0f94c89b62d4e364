"""GPU: ACE law 66 (N-body phase space).  ndpp_nbody_leg_batch against its host restatement
(tests/nbody_ref.py: nbody_numpy) bit for bit, in both builds; the whole-nuclide driver with the
option off (nothing changes) and on (the reaction's rows, scaled and summed in the driver's order,
through the host-side and the device-side reaction sum); ndpp_scatt_nuclide with its own grids and the
tabular refusal; and `python -m ndpp_amd.run --nbody` end to end."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from nbody_ref import nbody_nuclide, nbody_numpy, threshold
from synth import same_bits

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

# n: (Q, Ap); the two targets of every n
KIN = {3: {1.9968: (-2.2246, 2.9986), 236.0: (-6.2, 3.0)}, 4: {1.9968: (-1.6, 4.0), 236.0: (-1.6, 4.0)},
       5: {1.9968: (-7.0, 5.0), 236.0: (-7.0, 5.0)}}
B70 = np.concatenate([[0.0], np.geomspace(1e-11, 20.0, 70)])
E_EDGE = 15.0          # above every threshold of KIN: the energy whose E0 is made a group edge


def batch_case(shape, n, A):
    """(ein, e_bins, L) of one shape"""
    Q, Ap = KIN[n][A]
    thr = threshold(A, Q)
    up = float(np.nextafter(thr, np.inf))
    n_ein, G, L = shape
    if shape == (1, 1, 1):                                   # a top edge below the lab maximum
        return np.array([14.0]), np.array([0.0, 0.5]), L
    if shape == (7, 5, 11):
        E0 = E_EDGE / ((A + 1.0) * (A + 1.0))                # an edge equal to E0: Tb = 0 above it, below it
        bins = np.array([0.0, 1e-5, E0, 2.0, 8.0, 20.0])     # (and the lowest group starts at 0: duplicates)
        return np.array([0.9 * thr, thr, up, E_EDGE, 20.0, np.nan, -1.0]), bins, L
    return np.array([up, 6.0, 10.0, 14.0, 20.0]), B70, L


@pytest.mark.parametrize("A", [1.9968, 236.0])
@pytest.mark.parametrize("n", [3, 4, 5])
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 5, 11), (5, 70, 6)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_nbody_batch_equals_the_restatement_in_every_bit(hip, shape, n, A):
    Q, Ap = KIN[n][A]
    ein, bins, L = batch_case(shape, n, A)
    assert (len(ein), len(bins) - 1) == shape[:2]
    out, st = hip.nbody_leg_batch(hip.Params.default(L, 65), A, Q, n, Ap, ein, bins)
    ref, ref_st = nbody_numpy(A, Q, n, Ap, ein, bins, L)
    diff = np.abs(out - ref).max()
    print(f"n={n} A={A} {shape}: max |device - restatement| {diff:.3e}; row sums {out[:, :, 0].sum(axis=1)}; status {st}")
    assert np.array_equal(st, ref_st)
    assert same_bits(out, ref)
    if shape == (7, 5, 11):
        assert st.tolist() == [0, 0, 0, 0, 0, hip.ST_RANGE, hip.ST_RANGE]
        assert not out[[0, 1, 5, 6]].any() and out[2].any() and out[3].any()
    if shape == (1, 1, 1):
        assert 0.0 < out[0, 0, 0] < 1.0


def test_gpu_nbody_batch_empty_call(hip):
    out, st = hip.nbody_leg_batch(hip.Params.default(4, 65), 1.9968, -2.2246, 3, 2.9986, np.zeros(0), B70)
    assert out.shape == (0, 70, 4) and st.shape == (0,)


# ---- the whole nuclide -------------------------------------------------------------------------------
EIN_EL = np.array([1e-3, 2.0, 20.0])
EIN_INEL = np.array([0.5, 1.2, 3.4, 3.4000001, 5.0, 14.0, 20.0])     # 3.4: the threshold energy of MT 16


def library_at(hip, nuc, L=4):
    p = hip.Params.default(L, nuc["mu_bins"])
    (r,) = hip.scatt_library_at(p, [nuc], nuc["bins"], [EIN_EL], [EIN_INEL], nuscatt=True)
    return r


@pytest.fixture(scope="module")
def off_rows(hip):
    """option off: the nuclide without MT 16, and the same nuclide with it"""
    assert hip.get_nbody() is False
    return library_at(hip, nbody_nuclide(with_mt16=False)), library_at(hip, nbody_nuclide())


def test_gpu_option_off_changes_nothing(off_rows):
    without, with16 = off_rows
    for k in ("el_mat", "inel_mat", "nuinel_mat", "ein_el", "ein_inel"):
        assert same_bits(without[k], with16[k]), k


def sigma_and_pvalid(nuc, rx, E):
    """scatt_interp_distro's cross section and p_valid of one reaction at E, in its operations"""
    en, sig, thr = nuc["energy"], rx["sigma"], rx["thr"]
    if E >= en[-1]:
        s = sig[-1]
    else:
        i = int(np.searchsorted(en, E, side="right")) - 1
        fr = (E - en[i]) / (en[i + 1] - en[i])
        k = i - (thr - 1)
        s = (1.0 - fr) * sig[k] + fr * sig[k + 1]
    x, y = rx["edists"][0]["pv_x"], rx["edists"][0]["pv_y"]
    r = (E - x[0]) / (x[1] - x[0])
    return s, (1.0 - r) * y[0] + r * y[1]


@pytest.mark.parametrize("dev_sum_min", ["0", str(1 << 60)], ids=["device_sum", "host_sum"])
def test_gpu_option_on_adds_the_scaled_rows(hip, off_rows, monkeypatch, dev_sum_min):
    monkeypatch.setenv("NDPP_HIP_DEV_SUM_MIN", dev_sum_min)
    nuc = nbody_nuclide()
    off = off_rows[0]
    before = hip.set_nbody(True)
    try:
        on = library_at(hip, nuc)
    finally:
        hip.set_nbody(before)
    assert same_bits(on["el_mat"], off["el_mat"]) and same_bits(on["ein_inel"], off["ein_inel"])
    rx = nuc["reactions"][-1]
    n, Ap = rx["edists"][0]["data"]
    rows, st = nbody_numpy(nuc["awr"], rx["Q"], int(n), Ap, EIN_INEL, nuc["bins"], 4)
    assert not st.any()
    e_thr = nuc["energy"][rx["thr"] - 1]
    changed = 0
    for i, E in enumerate(EIN_INEL):
        if E <= e_thr:                                       # at or below the threshold energy: unchanged
            assert same_bits(on["inel_mat"][i], off["inel_mat"][i]) and same_bits(on["nuinel_mat"][i], off["nuinel_mat"][i])
            continue
        s, pv = sigma_and_pvalid(nuc, rx, E)
        t = rows[i] * s * pv
        assert same_bits(on["inel_mat"][i], off["inel_mat"][i] + t), E
        assert same_bits(on["nuinel_mat"][i], off["nuinel_mat"][i] + 2.0 * t), E
        changed += int(not same_bits(on["inel_mat"][i], off["inel_mat"][i]))
    assert changed == int((EIN_INEL > e_thr).sum()) == 4


def test_gpu_scatt_nuclide_own_grids_and_the_tabular_refusal(hip):
    nuc = nbody_nuclide()
    p = hip.Params.default(4, nuc["mu_bins"])
    e_thr = nuc["energy"][nuc["reactions"][-1]["thr"] - 1]
    before = hip.set_nbody(True)
    try:
        r = hip.scatt_nuclide(p, nuc, nuc["bins"])
        with pytest.raises(hip.NdppError) as err:
            hip.scatt_nuclide_tab(p, 8, nuc, nuc["bins"])
    finally:
        hip.set_nbody(before)
    assert e_thr in r["ein_inel"]
    assert np.isfinite(r["inel_mat"]).all() and r["inel_mat"][r["ein_inel"] > e_thr, :, 0].sum(axis=1).min() > 0.0
    assert err.value.code == -22 and "law 66" in str(err.value) and "Legendre output only" in str(err.value)
    assert hip.scatt_nuclide_tab(p, 8, nuc, nuc["bins"])["inel_mat"] is not None      # option off: as before


def test_gpu_run_with_the_flag(tmp_path):
    from ndpp_amd import reader
    nuc = ace_synth.quantise(nbody_nuclide(p_valid=False))
    sums, grids, reps = {}, {}, {}
    for tag, extra in (("off", []), ("on", ["--nbody"])):
        run = tmp_path / tag
        ace_synth.write_inputs(run, "1002.80c", nuc, scatt_order=3, mu_bins=nuc["mu_bins"], threads=1,
                               print_tol=1e-30)
        r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), "--json", str(run / "run.json"), *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=270)
        print(r.stdout[-2000:], r.stderr[-2000:])
        assert r.returncode == 0
        t = reader.read_binary((run / "1002.80c.g5").read_bytes())
        grids[tag], sums[tag] = t.inelastic.ein, t.inelastic.mat[:, :, 0].sum(axis=1)
        reps[tag] = json.loads((run / "run.json").read_text())
    assert "nbody" not in reps["off"] and reps["on"]["nbody"] == dict(reactions=1, tables={"1002.80c": 1})
    rx = nuc["reactions"][-1]
    e_thr = nuc["energy"][rx["thr"] - 1]
    assert e_thr in grids["on"]
    # a grid point of the nuclide above the threshold, in both grids: sigma is the tabulated value there
    common = [E for E in nuc["energy"][rx["thr"]:] if E in grids["on"] and E in grids["off"] and E < 20.0]
    assert common
    for E in common:
        sig = rx["sigma"][int(np.where(nuc["energy"] == E)[0][0]) - (rx["thr"] - 1)]
        s_on = sums["on"][np.where(grids["on"] == E)[0][0]]
        s_off = sums["off"][np.where(grids["off"] == E)[0][0]]
        print(f"E = {E}: sum P0 {s_off:.15g} -> {s_on:.15g}, sigma16 {sig:.15g}, miss {abs(s_on - s_off - sig):.3e}")
        assert abs((s_on - s_off) - sig) <= 1e-12 * s_on
