"""gfx950 free gas (and file 6) at non-default integration tunables against the reference's goldens
(tests/golden/freegas_tunables.npz, the grid of make_golden.tunable_points()), plus the device-only
paths those tunables move: the split walk below its depth, the sibling stack's global part, the
arena / chunking logic, the device-pointer entry point and the tabular free-gas kernel.  -m gpu"""
import numpy as np
import pytest

from conftest import load_golden, scale_rel_err
from test_tunables import IDS, POINTS, TABLES, TUN_DEFAULT, set_params, table

pytestmark = pytest.mark.gpu

# the bars of test_hostsim.test_pipeline_matches_reference: the product arithmetic, the reference's
BAR_FAST, BAR_STRICT = 1e-10, 5e-15
SETTINGS = {"default": {}, "walk": {"NDPP_HIP_GAUSS": "0"}, "strict": {"NDPP_HIP_STRICT_BELOW": "1e30"}}


@pytest.fixture(scope="module")
def gt():
    return load_golden("freegas_tunables")


def in_gauss_box(tun):
    return tun[3] >= 15 and tun[2] <= 1e-7


def leg(hip, g, t, tun, **kw):
    T = table(g, t)
    p = set_params(hip.Params.default(int(T["L"]), int(g["M"])), tun)
    return hip.elastic_leg_batch(p, float(T["A"]), float(g["kT"]), 1e300, 0.0, T["ein"], T["row_lo"],
                                 T["w_hi"], T["f_tab"], T["bins"], **kw)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("k", range(len(POINTS)), ids=IDS)
def test_leg_batch_matches_golden(hip, gt, monkeypatch, k, setting):
    """Every point of the grid, every table, in the shipped arithmetic, with the Gauss stage off and
    in the reference's arithmetic everywhere.  mu_its 20 and 31 run the global part of the sibling
    stack; mu_its below 4 walk trees shallower than the split walk's 16 pieces."""
    for name, v in SETTINGS[setting].items():
        monkeypatch.setenv(name, v)
    tun = POINTS[k]
    errs, gauss = {}, 0
    for t in TABLES:
        out, status, st = leg(hip, gt, t, tun, want_stats=True)
        assert (status == 0).all(), (t, status)
        errs[t] = scale_rel_err(out, gt[f"p{k}_{t}_out"])
        gauss += st.gauss_integrals
    print(f"{IDS[k]} [{setting}]: " + ", ".join(f"{t} {e:.2e}" for t, e in errs.items()) +
          f"; Gauss integrals {gauss}")
    assert max(errs.values()) < (BAR_STRICT if setting == "strict" else BAR_FAST), errs
    # the Gauss stage only inside the box of tunables where its parity was measured
    if setting != "default" or not in_gauss_box(tun):
        assert gauss == 0
    elif tun == TUN_DEFAULT:
        assert gauss > 0


@pytest.mark.parametrize("mu_its", [0, 1, 3, 4, 5])
def test_split_walk_below_its_depth(hip, gt, monkeypatch, mu_its):
    """The split walk hands an inner integral to 16 work items at depth 4; trees that stop at or
    above that depth must give the bits of the unsplit walk."""
    k = POINTS.index(TUN_DEFAULT[:3] + (mu_its,) + TUN_DEFAULT[4:])
    for t in TABLES:
        split, _ = leg(hip, gt, t, POINTS[k])
        monkeypatch.setenv("NDPP_HIP_NO_SPLIT", "1")
        whole, _ = leg(hip, gt, t, POINTS[k])
        monkeypatch.delenv("NDPP_HIP_NO_SPLIT")
        assert np.array_equal(split, whole), t


def test_chunking_at_a_tight_outer_tolerance(hip, gt, monkeypatch):
    """eout_tol 1e-10 grows the outer trees past the arena's guess per call: one chunk, chunks of
    one energy and a small arena guess (the overflow -> redo path) give the same bits, within the
    bar of the reference."""
    k = POINTS.index(TUN_DEFAULT[:4] + (1e-10,) + TUN_DEFAULT[5:])
    tun = POINTS[k]
    T = table(gt, "h1")
    p = set_params(hip.Params.default(int(T["L"]), int(gt["M"])), tun)
    # the golden's two energies first, then four more: a batch worth chunking
    ein = np.concatenate([T["ein"], T["ein"] * 1.5, T["ein"] * 0.7])
    E_grid = gt["E_grid"]
    row = (np.searchsorted(E_grid, ein, side="right") - 1).astype(np.int32)
    w = (ein - E_grid[row]) / (E_grid[row + 1] - E_grid[row])
    args = (float(T["A"]), float(gt["kT"]), 1e300, 0.0, ein, row, w, T["f_tab"], T["bins"])
    want, st0, s0 = hip.elastic_leg_batch(p, *args, want_stats=True)
    assert (st0 == 0).all()
    assert scale_rel_err(want[:2], gt[f"p{k}_h1_out"]) < BAR_FAST
    monkeypatch.setenv("NDPP_HIP_MAX_CHUNK_EIN", "1")
    got, _, s1 = hip.elastic_leg_batch(p, *args, want_stats=True)
    assert np.array_equal(got, want) and s1.mu_kernel_launches > s0.mu_kernel_launches
    monkeypatch.delenv("NDPP_HIP_MAX_CHUNK_EIN")
    monkeypatch.setenv("NDPP_HIP_NODES_PER_CALL", "400")
    got, _, s2 = hip.elastic_leg_batch(p, *args, want_stats=True)
    assert np.array_equal(got, want) and s2.mu_kernel_launches > s0.mu_kernel_launches


DEVICE_ENTRY = r"""
import sys
import torch                      # (before the library: it then binds to torch's HIP runtime)
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import ndpp_amd
from conftest import load_golden
from test_tunables import POINTS, TUN_DEFAULT, set_params, table
g = load_golden("freegas_tunables")
tun = TUN_DEFAULT[:3] + (10,) + TUN_DEFAULT[4:]
for t in ("h1", "u238"):
    T = table(g, t)
    p = set_params(ndpp_amd.Params.default(int(T["L"]), int(g["M"])), tun)
    args = (float(T["A"]), float(g["kT"]), 1e300, 0.0)
    host, status = ndpp_amd.elastic_leg_batch(p, *args, T["ein"], T["row_lo"], T["w_hi"], T["f_tab"], T["bins"])
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt, device="cuda")
    out_t = torch.zeros(host.shape, dtype=torch.float64, device="cuda")
    st_t = torch.zeros(len(T["ein"]), dtype=torch.int32, device="cuda")
    ndpp_amd.elastic_leg_batch_device(p, *args, dev(T["ein"]), dev(T["row_lo"], torch.int32), dev(T["w_hi"]),
                                      dev(T["f_tab"]), dev(T["bins"]), out_t, st_t)
    torch.cuda.synchronize()
    assert np.array_equal(out_t.cpu().numpy(), host), t
    assert np.array_equal(st_t.cpu().numpy(), status), t
print("DEVICE_ENTRY_OK")
"""


def test_device_entry_point_at_non_default_tunables(hip, gt):
    """ndpp_elastic_leg_batch_d gives the host entry point's bits (mu_its 10, outside the Gauss box).
    In a child process: torch has to be imported before the library is loaded, which this session
    has already done."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY, str(root)], cwd=root, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "DEVICE_ENTRY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("sab,brent", [(1e-3, 1e-6), (1e-10, 1e-6), (1e-6, 1e-3), (1e-6, 1e-9)])
def test_tabular_freegas_at_thresholds(hip, gt, sab, brent):
    """elastic_tab_batch at the find_FG_mu thresholds: the bins add up to the Legendre P0 of the same
    parameters (itself held to the reference's golden), and they agree with the scipy restatement at
    the same sab_threshold, at the bars DESIGN.md section 11 measured (2e-6 and 5e-6 of the largest
    value).  At sab_threshold 1e-3 the sum rule was measured at 2.4e-6 on an MI355X (bar 3e-6), and
    the scipy restatement is not used: its mu range (brentq on S - threshold) is 5.6e-4 away from
    bins whose sum matches the reference's P0 to 2.4e-6, i.e. it does not restate find_FG_mu closely
    enough once the cut-off carries a 1e-3 share of the integral."""
    from test_gpu_tabular import fg_scipy
    k = POINTS.index((sab, brent) + TUN_DEFAULT[2:])
    T = table(gt, "h1")
    p = set_params(hip.Params.default(int(T["L"]), int(gt["M"])), POINTS[k])
    N = 7
    args = (float(T["A"]), float(gt["kT"]), 1e300, 0.0, T["ein"], T["row_lo"], T["w_hi"], T["f_tab"], T["bins"])
    tab, st_t = hip.elastic_tab_batch(p, N, *args)
    leg_out, st_l = hip.elastic_leg_batch(p, *args)
    assert ((st_t & ~hip.lib.ST_TAB_UNSETTLED) == st_l).all() and (st_l == 0).all()
    assert scale_rel_err(leg_out, gt[f"p{k}_h1_out"]) < BAR_FAST
    scale = np.abs(leg_out[:, :, 0]).max(axis=1)
    sum_err = (np.abs(tab.sum(axis=2) - leg_out[:, :, 0]).max(axis=1) / scale).max()
    print(f"sab {sab:g} brent {brent:g}: sum rule {sum_err:.2e}")
    assert sum_err <= (3e-6 if sab > 1e-6 else 2e-6)
    if sab > 1e-6:
        return
    i = 0                                   # E_in = kT: fg_scipy's domain (E_in <= 100 kT)
    r = T["row_lo"][i]
    ref = fg_scipy(float(T["A"]), float(gt["kT"]), T["ein"][i], T["f_tab"][r], T["f_tab"][r + 1],
                   T["w_hi"][i], T["bins"], N, sab_threshold=sab)
    sp_err = np.abs(tab[i] - ref).max() / np.abs(ref).max()
    print(f"  tabular vs scipy {sp_err:.2e}")
    assert sp_err <= 5e-6


@pytest.mark.parametrize("ne", [2, 7, 40])
def test_file6_at_ne_per_grp(hip, gt, ne):
    """file6_leg_batch (CM and lab) at ne_per_grp 2, 7 and 40 against the reference, at the file-6
    bar of test_gpu_file6 (1e-10)."""
    from synth import kalbach_rows
    M, L = int(gt["M"]), int(gt["f6_L"])
    T = kalbach_rows(M, 6, 6, 14, 0.5, 20.0, seed=int(gt["f6_seed"]), dup_last=True, intt=2)
    p = hip.Params.default(L, M)
    p.ne_per_grp = ne
    args = (gt["f6_ein"], gt["f6_row"], T["e_grid"], T["row_ptr"], T["eout"], T["pdf"], T["intt"],
            T["f"], gt["f6_bins"])
    cm, st = hip.file6_leg_batch(p, 236.0058, 1, *args)
    lab, st2 = hip.file6_leg_batch(p, 236.0058, 0, *args)
    assert (st == 0).all() and (st2 == 0).all()
    e_cm, e_lab = scale_rel_err(cm, gt[f"f6_{ne}_cm"]), scale_rel_err(lab, gt[f"f6_{ne}_lab"])
    print(f"file6 ne_per_grp {ne}: cm {e_cm:.2e}, lab {e_lab:.2e}")
    assert e_cm < 1e-10 and e_lab < 1e-10
    if ne != 20:       # the parameter is read: the answer is not the default's
        p.ne_per_grp = 20
        cm20, _ = hip.file6_leg_batch(p, 236.0058, 1, *args)
        assert not np.array_equal(cm20, cm)
