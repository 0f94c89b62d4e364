"""Free gas at non-default integration tunables (ndpp.xml's adaptive_mu_its, adaptive_mu_tol,
adaptive_eout_its, adaptive_eout_tol, sab_threshold, brent_mu_thresh, ne_per_grp).  Every other
free-gas test runs at the defaults; here the reference (flang build, where it exists), the C oracle
and the product's stage functions on the CPU (tests/hostsim) are held against
tests/golden/freegas_tunables.npz at every point of make_golden.tunable_points(), and the C ABI's
refusal of tunables the reference cannot be given is checked.  The kernels themselves at the same
points: test_gpu_tunables.py."""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import GOLDEN, dp, ip, load_golden, oracle_params, scale_rel_err

sys.path.insert(0, str(GOLDEN))
from make_golden import TUN_DEFAULT, tunable_points  # noqa: E402

TABLES = ("h1", "u238", "curved")
POINTS = tunable_points()


def tun_id(t):
    names = ("sab", "brent", "mu_tol", "mu_its", "eout_tol", "eout_its", "ne")
    diff = [f"{n}={v:g}" for n, v, v0 in zip(names, t, TUN_DEFAULT) if v != v0]
    return ",".join(diff) or "default"


IDS = [tun_id(t) for t in POINTS]


def pin_tables(tun):
    """The tables the oracle is pinned on at a point: all, but at mu_its 31 (the oracle and the
    reference take a minute or more per table there) the curved one only."""
    return ("curved",) if tun[3] == 31 else TABLES


@pytest.fixture(scope="module")
def gt():
    g = load_golden("freegas_tunables")
    assert int(g["n_points"]) == len(POINTS)
    for k, t in enumerate(POINTS):           # the grid the golden was made on is the grid tested
        assert tuple(g[f"p{k}_tun"]) == t
    return g


def table(g, t):
    return {k: g[f"{t}_{k}"] for k in ("A", "L", "bins", "ein", "f_tab", "row_lo", "w_hi")}


def set_params(p, tun):
    """Write the seven tunables (make_golden.TUN_DEFAULT's order) into an ndpp_params / oracle_params."""
    sab, brent, mu_tol, mu_its, eout_tol, eout_its, ne = tun
    p.sab_threshold, p.brent_mu_thresh = sab, brent
    p.adaptive_mu_tol, p.adaptive_mu_its = mu_tol, int(mu_its)
    p.adaptive_eout_tol, p.adaptive_eout_its = eout_tol, int(eout_its)
    p.ne_per_grp = int(ne)
    return p


@pytest.fixture(scope="module")
def ref_tun(ref):
    """The session's reference library, given back its default parameters afterwards (the `ref`
    fixture is session-scoped: later tests must not run on this module's tunables)."""
    yield ref
    ref.ref_set_params(*TUN_DEFAULT, 10, 50, 30)


def oracle_rows(oracle, g, t, tun):
    T = table(g, t)
    M = int(g["M"])
    mu = np.empty(M)
    oracle.oracle_mu_grid(M, dp(mu))
    p = set_params(oracle_params(oracle, int(T["L"]), M), tun)
    G = len(T["bins"]) - 1
    lo = np.zeros((len(T["ein"]), G, int(T["L"])))
    hi = np.zeros_like(lo)
    for n, E in enumerate(T["ein"]):
        for r, dst in ((T["row_lo"][n], lo), (T["row_lo"][n] + 1, hi)):
            f = np.ascontiguousarray(T["f_tab"][r])
            oracle.oracle_integrate_freegas_leg(C.byref(p), E, float(T["A"]), float(g["kT"]), dp(f),
                                                dp(mu), dp(T["bins"]), G + 1, dp(dst[n]))
    return lo, hi


# ---- the checker: oracle == reference == golden, bit for bit -------------------------------------
@pytest.mark.parametrize("k", range(len(POINTS)), ids=IDS)
def test_oracle_matches_reference(oracle, ref_tun, gt, k):
    tun = POINTS[k]
    ref_tun.ref_set_params(*tun, 10, 50, 30)
    M = int(gt["M"])
    mu = np.empty(M)
    oracle.oracle_mu_grid(M, dp(mu))
    for t in pin_tables(tun):
        T = table(gt, t)
        G, L = len(T["bins"]) - 1, int(T["L"])
        lo_o, hi_o = oracle_rows(oracle, gt, t, tun)
        for n, E in enumerate(T["ein"]):
            for r, mine in ((T["row_lo"][n], lo_o[n]), (T["row_lo"][n] + 1, hi_o[n])):
                f = np.ascontiguousarray(T["f_tab"][r])
                out = np.zeros((G, L))
                ref_tun.ref_integrate_freegas_leg(E, float(T["A"]), float(gt["kT"]), dp(f), dp(mu), M,
                                                  dp(T["bins"]), G + 1, L, dp(out))
                assert np.array_equal(out, mine), (t, n, r)
    ref_tun.ref_set_params(*TUN_DEFAULT, 10, 50, 30)


@pytest.mark.parametrize("sab,brent", [(1e-3, 1e-6), (1e-10, 1e-6), (1e-6, 1e-3), (1e-6, 1e-9)])
def test_find_fg_mu_matches_reference_at_thresholds(oracle, ref_tun, sab, brent):
    p = oracle_params(oracle)
    p.sab_threshold, p.brent_mu_thresh = sab, brent
    ref_tun.ref_set_params(sab, brent, 1e-7, 15, 1e-8, 15, 20, 10, 50, 30)
    n_moved = 0
    for A in (0.999167, 15.8575, 236.0058):
        for Ein in (1e-11, 2.53e-8, 6.25e-7, 5e-6):
            for s in (1e-3, 0.3, 0.9, 1.0, 1.1, 2.5, 30.0):
                m0, m1, m2 = np.zeros(2), np.zeros(2), np.zeros(2)
                ref_tun.ref_find_fg_mu(A, 2.53e-8, Ein, Ein * s, dp(m0))
                oracle.oracle_find_fg_mu(C.byref(p), A, 2.53e-8, Ein, Ein * s, dp(m1))
                assert (m0 == m1).all(), (A, Ein, s)
                oracle.oracle_find_fg_mu(C.byref(oracle_params(oracle)), A, 2.53e-8, Ein, Ein * s, dp(m2))
                n_moved += int((m1 != m2).any())
    ref_tun.ref_set_params(*TUN_DEFAULT, 10, 50, 30)
    assert n_moved > 0          # the threshold is actually read


@pytest.mark.parametrize("k", range(len(POINTS)), ids=IDS)
def test_oracle_matches_golden(oracle, gt, k):
    """What pins the oracle where the reference is absent."""
    for t in pin_tables(POINTS[k]):
        lo, hi = oracle_rows(oracle, gt, t, POINTS[k])
        assert np.array_equal(lo, gt[f"p{k}_{t}_lo"]), t
        assert np.array_equal(hi, gt[f"p{k}_{t}_hi"]), t


def test_golden_points_differ():
    """Each tunable moves the reference's answer somewhere in the grid: a golden that ignored its
    tunables (a generator that did not set them) would look like this."""
    g = load_golden("freegas_tunables")
    base = POINTS.index(TUN_DEFAULT)
    for k in range(len(POINTS)):
        if k == base or POINTS[k][6] != TUN_DEFAULT[6]:
            continue
        moved = any(not np.array_equal(g[f"p{k}_{t}_out"], g[f"p{base}_{t}_out"]) for t in TABLES)
        # (mu_its 20 / 31 converge before the limit everywhere on these tables: same bits)
        assert moved or POINTS[k][3] in (20, 31), POINTS[k]


# ---- the product's stage functions on the CPU -----------------------------------------------------
def run_hostsim(hostsim, hip, g, t, tun, joint):
    T = table(g, t)
    L, M = int(T["L"]), int(g["M"])
    p = set_params(hip.Params.default(L, M), tun)
    bins = np.ascontiguousarray(T["bins"])
    G = len(bins) - 1
    n = len(T["ein"])
    row = np.empty(2 * n, dtype=np.int32)
    row[0::2] = T["row_lo"]
    row[1::2] = T["row_lo"] + 1
    if joint:
        ein, n_jobs, R = np.ascontiguousarray(T["ein"]), n, 2
    else:
        ein, n_jobs, R = np.ascontiguousarray(np.repeat(T["ein"], 2)), 2 * n, 1
    f_tab = np.ascontiguousarray(T["f_tab"])
    raw = np.zeros((2 * n, G, L))
    stats = (C.c_ulonglong * 4)()
    rc = hostsim.hostsim_freegas_jobs(C.byref(p), float(T["A"]), float(g["kT"]), n_jobs, R,
                                      dp(ein), ip(row), f_tab.shape[0], dp(f_tab), G, dp(bins),
                                      200000, dp(raw), stats, None)
    assert rc == 0
    return raw[0::2], raw[1::2], list(stats)


@pytest.mark.parametrize("k", range(len(POINTS)), ids=IDS)
def test_hostsim_matches_golden(hostsim, hip, gt, monkeypatch, k):
    """The bars of test_hostsim.test_pipeline_matches_reference: 1e-10 for the product arithmetic
    (with and without the Gauss stage, R = 1 and joint R = 2), 5e-15 for the reference order.
    Before the Gauss stage was boxed to the tunables where it was measured, the product arithmetic
    with it failed from mu_its 10 down (7.0e-9 at mu_its 10, 9.3e-2 at mu_its 0 on these tables)."""
    runs = ([("1", False), ("1", True), ("0", False), ("0", True)] if hostsim.variant == "fast"
            else [("0", False)])     # (joint rows and the Gauss stage belong to the product arithmetic)
    bar = 5e-15 if hostsim.variant == "strict" else 1e-10
    errs = {}
    for gauss, joint in runs:
        monkeypatch.setenv("HOSTSIM_GAUSS", gauss)
        for t in TABLES:
            lo, hi, _ = run_hostsim(hostsim, hip, gt, t, POINTS[k], joint)
            errs[(t, f"gauss={gauss}", f"R={1 + joint}")] = max(
                scale_rel_err(lo, gt[f"p{k}_{t}_lo"]), scale_rel_err(hi, gt[f"p{k}_{t}_hi"]))
    worst = max(errs, key=errs.get)
    print(f"{IDS[k]} [{hostsim.variant}]: worst {errs[worst]:.2e} at {worst}")
    assert errs[worst] < bar, {c: f"{e:.2e}" for c, e in errs.items() if e >= bar}


@pytest.mark.parametrize("k", [IDS.index(s) for s in ("mu_its=8", "mu_its=14", "mu_tol=1e-05", "default")],
                         ids=["mu_its=8", "mu_its=14", "mu_tol=1e-05", "default"])
def test_hostsim_gauss_stage_only_inside_its_box(hostsim, hip, gt, monkeypatch, k):
    """The Gauss stage runs at the default tunables and nowhere outside mu_its >= 15, mu_tol <= 1e-7:
    outside, HOSTSIM_GAUSS=1 gives the walk's bits."""
    if hostsim.variant != "fast":
        pytest.skip("the Gauss stage belongs to the product arithmetic")
    monkeypatch.setenv("HOSTSIM_GAUSS", "1")
    lo1, hi1, st1 = run_hostsim(hostsim, hip, gt, "h1", POINTS[k], True)
    monkeypatch.setenv("HOSTSIM_GAUSS", "0")
    lo0, hi0, st0 = run_hostsim(hostsim, hip, gt, "h1", POINTS[k], True)
    if POINTS[k] == TUN_DEFAULT:
        assert st1[2] < st0[2]                      # fewer integrals walked: the stage took some
    else:
        assert st1 == st0 and np.array_equal(lo1, lo0) and np.array_equal(hi1, hi0)


# ---- the C ABI refuses what the reference cannot be given ----------------------------------------
BAD = [("adaptive_mu_its", 32), ("adaptive_mu_its", -1), ("adaptive_eout_its", 32),
       ("adaptive_eout_its", -1)] + [
    (f, v) for f in ("sab_threshold", "brent_mu_thresh", "adaptive_mu_tol", "adaptive_eout_tol")
    for v in (-1e-7, -5e-324, float("nan"), float("inf"))]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v!r}" for f, v in BAD])
def test_bad_tunables_are_refused(hip, field, value):
    """NDPP_EINVAL before any device work (so without a GPU too), for the single-call and the
    batch entry points."""
    lib = hip.load()
    p = hip.Params.default(4, 257)
    setattr(p, field, value)
    f = np.full(257, 0.5)
    b = np.array([0.0, 6.25e-7, 20.0])
    out = np.zeros(8)
    rc = lib.ndpp_integrate_freegas_leg(C.byref(p), 2.53e-8, 0.999167, 2.5301e-8, dp(f), None, dp(b),
                                        3, dp(out))
    assert rc == -22, lib.ndpp_last_error()
    with pytest.raises(hip.NdppError) as e:
        hip.elastic_leg_batch(p, 0.999167, 2.5301e-8, 1e300, 0.0, np.array([2.53e-8]),
                              np.zeros(1, np.int32), np.zeros(1), np.stack([f, f]), b)
    assert e.value.code == -22


def test_zero_tolerances_are_accepted(hip):
    """0 is a value the reference takes (every test refines to the depth limit): not refused.
    (Without a device the call stops at NDPP_EDEVICE, after the argument checks.)"""
    lib = hip.load()
    if lib.ndpp_device_count() > 0:
        pytest.skip("a HIP device is present: this would compute (test_gpu_tunables covers it)")
    p = hip.Params.default(4, 257)
    p.adaptive_mu_tol = p.adaptive_eout_tol = p.sab_threshold = p.brent_mu_thresh = 0.0
    p.adaptive_mu_its = p.adaptive_eout_its = 31
    f = np.full(257, 0.5)
    b = np.array([0.0, 6.25e-7, 20.0])
    out = np.zeros(8)
    rc = lib.ndpp_integrate_freegas_leg(C.byref(p), 2.53e-8, 0.999167, 2.5301e-8, dp(f), None, dp(b),
                                        3, dp(out))
    assert rc == -5
