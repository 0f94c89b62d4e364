"""GPU: ACE law 66 (N-body phase space) in lab-cosine bins.  ndpp_nbody_tab_batch against its host
restatement (tests/nbody_tab_ref.py: nbody_tab_numpy) bit for bit, in both builds; the tabular
whole-nuclide call with both options on (the reaction's bins, scaled and summed in the driver's order,
through the device-side and the host-side reaction sum) and with ndpp_set_nbody alone (the old refusal);
and `python -m ndpp_amd.run --nbody-tabular` end to end."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from nbody_ref import nbody_nuclide, threshold
from nbody_tab_ref import nbody_tab_numpy
from synth import same_bits

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

# n: (Q, Ap); the two targets of every n (tests/test_gpu_nbody.py: KIN)
KIN = {3: {1.9968: (-2.2246, 2.9986), 236.0: (-6.2, 3.0)}, 4: {1.9968: (-1.6, 4.0), 236.0: (-1.6, 4.0)},
       5: {1.9968: (-7.0, 5.0), 236.0: (-7.0, 5.0)}}
B5 = np.array([0.0, 1e-3, 0.1, 1.0, 5.0, 20.0])
B70 = np.concatenate([[0.0], np.geomspace(1e-11, 20.0, 70)])
E_EDGE = 15.0          # above every threshold of KIN: the energy whose E0 is made a group edge


def batch_case(shape, n, A):
    """(ein, e_bins) of one shape (n_ein, G, N)"""
    Q, Ap = KIN[n][A]
    thr = threshold(A, Q)
    up = float(np.nextafter(thr, np.inf))
    if shape == (1, 1, 1):                                   # a top edge below the lab maximum
        return np.array([14.0]), np.array([0.0, 0.5])
    if shape == (7, 5, 7):
        E0 = E_EDGE / ((A + 1.0) * (A + 1.0))                # an edge equal to E0 of 15 MeV, the lowest group from 0
        return np.array([0.9 * thr, thr, up, E_EDGE, 20.0, np.nan, -1.0]), np.array([0.0, 1e-5, E0, 2.0, 8.0, 20.0])
    if shape == (2, 5, 128):
        return np.array([up, 14.0]), B5
    if shape == (3, 5, 32):                                  # Emax = 0.25, 0.5, 0.9 E0: both roots of a bin edge
        f = (Ap - 1.0) / Ap                                  # inside the range, which no other shape reaches
        return np.array([-Q * f / (f * A / (A + 1.0) - r / (A + 1.0) ** 2) for r in (0.25, 0.5, 0.9)]), B5
    return np.array([up, 6.0, 10.0, 14.0, 20.0]), B70


@pytest.mark.parametrize("A", [1.9968, 236.0])
@pytest.mark.parametrize("n", [3, 4, 5])
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 5, 7), (5, 70, 32), (2, 5, 128), (3, 5, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gpu_nbody_tab_batch_equals_the_restatement_in_every_bit(hip, shape, n, A):
    Q, Ap = KIN[n][A]
    ein, bins = batch_case(shape, n, A)
    N = shape[2]
    assert (len(ein), len(bins) - 1) == shape[:2]
    out, st = hip.nbody_tab_batch(hip.Params.default(4, 65), N, A, Q, n, Ap, ein, bins)
    ref, ref_st = nbody_tab_numpy(A, Q, n, Ap, ein, bins, N)
    diff = np.abs(out - ref).max()
    print(f"n={n} A={A} {shape}: max |device - restatement| {diff:.3e}; row sums {out.sum(axis=(1, 2))}; status {st}")
    assert out.shape == (shape[0], shape[1], N)
    assert np.array_equal(st, ref_st)
    assert same_bits(out, ref)
    assert (out >= 0.0).all()
    if shape == (7, 5, 7):
        assert st.tolist() == [0, 0, 0, 0, 0, hip.ST_RANGE, hip.ST_RANGE]
        assert not out[[0, 1, 5, 6]].any() and out[2].any() and out[3].any()
    if shape == (1, 1, 1):
        assert 0.0 < out[0, 0, 0] < 1.0


def test_gpu_nbody_tab_batch_empty_call(hip):
    out, st = hip.nbody_tab_batch(hip.Params.default(4, 65), 8, 1.9968, -2.2246, 3, 2.9986, np.zeros(0), B70)
    assert out.shape == (0, 70, 8) and st.shape == (0,)


# ---- the whole nuclide -------------------------------------------------------------------------------
N_TAB = 8


@pytest.fixture(scope="module")
def off_result(hip):
    """both options off: the tabular call leaves law 66 out, as the reference does"""
    assert hip.get_nbody() is False and hip.get_nbody_tab() is False
    nuc = nbody_nuclide()
    return hip.scatt_nuclide_tab(hip.Params.default(4, nuc["mu_bins"]), N_TAB, nuc, nuc["bins"], nuscatt=True)


def sigma_and_pvalid(nuc, rx, E):
    """scatt_interp_distro's cross section and p_valid of one reaction at E, in its operations
    (tests/test_gpu_nbody.py)"""
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
def test_gpu_both_options_on_add_the_scaled_bins(hip, off_result, monkeypatch, dev_sum_min):
    monkeypatch.setenv("NDPP_HIP_DEV_SUM_MIN", dev_sum_min)
    nuc = nbody_nuclide()
    p = hip.Params.default(4, nuc["mu_bins"])
    off = off_result
    before, before_tab = hip.set_nbody(True), hip.set_nbody_tab(True)
    try:
        on = hip.scatt_nuclide_tab(p, N_TAB, nuc, nuc["bins"], nuscatt=True)
    finally:
        hip.set_nbody_tab(before_tab)
        hip.set_nbody(before)
    assert same_bits(on["ein_el"], off["ein_el"]) and same_bits(on["el_mat"], off["el_mat"])
    rx = nuc["reactions"][-1]
    n, Ap = rx["edists"][0]["data"]
    e_thr = nuc["energy"][rx["thr"] - 1]
    common = [E for E in on["ein_inel"] if E in off["ein_inel"]]
    rows, st = nbody_tab_numpy(nuc["awr"], rx["Q"], int(n), Ap, common, nuc["bins"], N_TAB)
    assert not st.any() and (on["inel_mat"] >= 0.0).all()
    above = 0
    for k, E in enumerate(common):
        i, j = int(np.where(on["ein_inel"] == E)[0][0]), int(np.where(off["ein_inel"] == E)[0][0])
        if E <= e_thr:                                       # at or below the threshold energy: unchanged
            assert same_bits(on["inel_mat"][i], off["inel_mat"][j]), E
            assert same_bits(on["nuinel_mat"][i], off["nuinel_mat"][j]), E
            continue
        if E > nuc["bins"][-1]:                              # the extra point above the top edge: a copy
            assert same_bits(on["inel_mat"][i], on["inel_mat"][i - 1]), E
            assert same_bits(on["nuinel_mat"][i], on["nuinel_mat"][i - 1]), E
            continue
        s, pv = sigma_and_pvalid(nuc, rx, E)
        t = rows[k] * s * pv
        assert same_bits(on["inel_mat"][i], off["inel_mat"][j] + t), E
        assert same_bits(on["nuinel_mat"][i], off["nuinel_mat"][j] + 2.0 * t), E
        assert not same_bits(on["inel_mat"][i], off["inel_mat"][j]), E
        above += 1
    print(f"{len(common)} common energies, {above} above the threshold {e_thr}")
    assert above >= 4 and above < len(common)


def test_gpu_nbody_alone_keeps_the_tabular_refusal(hip):
    nuc = nbody_nuclide()
    p = hip.Params.default(4, nuc["mu_bins"])
    before = hip.set_nbody(True)
    try:
        assert hip.get_nbody_tab() is False
        with pytest.raises(hip.NdppError) as err:
            hip.scatt_nuclide_tab(p, N_TAB, nuc, nuc["bins"])
    finally:
        hip.set_nbody(before)
    assert err.value.code == -22 and "law 66" in str(err.value) and "Legendre output only" in str(err.value)
    before_tab = hip.set_nbody_tab(True)                     # the new option alone does nothing
    try:
        alone = hip.scatt_nuclide_tab(p, N_TAB, nuc, nuc["bins"])
    finally:
        hip.set_nbody_tab(before_tab)
    plain = hip.scatt_nuclide_tab(p, N_TAB, nuc, nuc["bins"])
    for k in ("ein_inel", "inel_mat", "ein_el", "el_mat"):
        assert same_bits(alone[k], plain[k]), k


def test_gpu_run_with_the_flag(tmp_path):
    from ndpp_amd import reader
    nuc = ace_synth.quantise(nbody_nuclide(p_valid=False))
    sec, reps = {}, {}
    for tag, extra in (("off", []), ("on", ["--nbody-tabular"])):
        run = tmp_path / tag
        ace_synth.write_inputs(run, "1002.80c", nuc, scatt_order=N_TAB, mu_bins=nuc["mu_bins"], threads=1,
                               print_tol=1e-30)
        xml = run / "ndpp.xml"
        xml.write_text(xml.read_text().replace("<scatt_type>legendre</scatt_type>", "<scatt_type>tabular</scatt_type>"))
        r = subprocess.run([sys.executable, "-m", "ndpp_amd.run", str(run), "--json", str(run / "run.json"), *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=270)
        print(r.stdout[-2000:], r.stderr[-2000:])
        assert r.returncode == 0
        sec[tag] = reader.read_binary((run / "1002.80c.g5").read_bytes()).inelastic
        reps[tag] = json.loads((run / "run.json").read_text())
    assert "nbody" not in reps["off"]
    assert reps["on"]["nbody"] == dict(reactions=1, tables={"1002.80c": 1}, tabular=True)
    assert sec["on"].mat.shape[2] == N_TAB and (sec["on"].mat >= 0.0).all()
    e_thr = nuc["energy"][nuc["reactions"][-1]["thr"] - 1]
    common = [E for E in sec["on"].ein if E in sec["off"].ein]
    above = 0
    for E in common:
        a = sec["on"].mat[np.where(sec["on"].ein == E)[0][0]]
        b = sec["off"].mat[np.where(sec["off"].ein == E)[0][0]]
        if E <= e_thr:
            assert same_bits(a, b), E
        else:
            assert (a >= b).all() and a.sum() > b.sum(), E
            above += 1
    assert above >= 1 and above < len(common)
