"""Library validation, host side (ndpp_amd.validate, ndpp_scatt_positivity / ndpp_expand_moments
argument checks): condensation bit for bit against the reference's loop order, the C ABI's
refusals before any device work, and the band / zero-row rules worked out by hand on an
independent numpy/scipy restatement that tests/test_gpu_validate.py holds the kernels to."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.special import eval_legendre

ROOT = Path(__file__).resolve().parent.parent


# ---- the independent restatement (numpy + scipy.special.eval_legendre) ------------------------
def np_basis(M, nm):
    mu = np.linspace(-1.0, 1.0, M)
    return np.array([(l + 0.5) * eval_legendre(l, mu) for l in range(nm)])        # (nm, M)


def np_positivity(mat, M=21, nm=None, chunk=20000):
    """The rules of ndpp_amd.validate on a dense (NE, G, L) section.  Returns dict(rows, negative
    [(iE, g)], min_value, min_row (iE, g), row_min (per offending row), scale (per offending
    row), plus for every checked row its (iE, g), min and scale Σ(l+½)|a_l| in `all_*`."""
    NE, G, L = mat.shape
    nm = L if nm is None else nm
    B = np_basis(M, nm)
    pos = mat[:, :, 0] > 0
    any_pos = pos.any(axis=1)
    gmin = np.where(any_pos, pos.argmax(axis=1), 0)
    gmax = np.where(any_pos, G - 1 - pos[:, ::-1].argmax(axis=1), -1)
    ie, gg = np.nonzero((np.arange(G)[None, :] >= gmin[:, None]) & (np.arange(G)[None, :] <= gmax[:, None]))
    a = mat[ie, gg, :nm]
    mins = np.empty(len(ie))
    negs = np.empty(len(ie), dtype=bool)
    for k in range(0, len(ie), chunk):
        F = a[k:k + chunk] @ B
        negs[k:k + chunk] = ~(F >= 0).all(axis=1)
        with np.errstate(invalid="ignore"):
            allnan = np.isnan(F).all(axis=1)
            F = np.where(np.isnan(F), np.inf, F)
        mins[k:k + chunk] = np.where(allnan, np.nan, F.min(axis=1))
    zero = np.nonzero(~any_pos)[0]
    # every checked row in (iE, g) order, zero rows as (iE, -1) with value 0.0
    all_ie = np.concatenate([ie, zero])
    all_g = np.concatenate([gg, np.full(len(zero), -1)])
    all_min = np.concatenate([mins, np.zeros(len(zero))])
    all_scale = np.concatenate([(np.abs(a) * (np.arange(nm) + 0.5)).sum(axis=1), np.zeros(len(zero))])
    all_neg = np.concatenate([negs, np.zeros(len(zero), dtype=bool)])
    order = np.lexsort((all_g, all_ie))
    all_ie, all_g, all_min, all_scale, all_neg = (x[order] for x in (all_ie, all_g, all_min, all_scale, all_neg))
    finite = ~np.isnan(all_min)
    if finite.any():
        k = np.flatnonzero(finite)[np.argmin(all_min[finite])]
        vmin, mrow = float(all_min[k]), (int(all_ie[k]), int(all_g[k]))
    else:
        vmin, mrow = np.inf, (-1, -1)
    return dict(rows=len(all_ie), negative=[(int(i), int(g)) for i, g in zip(all_ie[all_neg], all_g[all_neg])],
                min_value=vmin, min_row=mrow, row_min=all_min[all_neg], scale=all_scale[all_neg],
                all_rows=np.stack([all_ie, all_g], axis=1), all_min=all_min, all_scale=all_scale)


def np_expand(moments, M, nm=None):
    nm = moments.shape[1] if nm is None else nm
    return moments[:, :nm] @ np_basis(M, nm)


# ---- hand-made sections with the expected numbers worked out ----------------------------------
def hand_sections():
    """(name, mat (NE, G, L), M, expected dict(rows, negative, min_value, min_row)).
    L = 2: f(mu) = a0/2 + 3/2 a1 mu, minimum at mu = -1 (a1 > 0) of a0/2 - 3/2 a1."""
    G, L = 4, 2
    m = np.zeros((4, G, L))
    # E_in 0: band 1..2 (groups 0 and 3 have P0 = 0); row (0,1) = [1, 0.2]: min 0.2; (0,2) = [0.4, 0.3]: -0.25
    m[0, 1] = [1.0, 0.2]
    m[0, 2] = [0.4, 0.3]
    # E_in 1: no P0 > 0 anywhere (a negative P0 and a moment outside any band): one zero row
    m[1, 0] = [-0.5, 0.1]
    m[1, 3] = [0.0, 5.0]
    # E_in 2: band 0..3 with an interior row whose P0 <= 0 -- it is checked: (2,1) = [0, 0.1] -> -0.15
    m[2, 0] = [2.0, 0.0]
    m[2, 1] = [0.0, 0.1]
    m[2, 3] = [1.0, -0.2]          # a1 < 0: minimum at mu = +1: 0.5 - 0.3 = 0.2
    # E_in 3: a single-group band: [0.2, 0.1] -> min 0.1 - 0.15 = -0.05
    m[3, 2] = [0.2, 0.1]
    # rows: 2 + 1 (zero) + 4 + 1 = 8; negative (0,2), (2,1), (3,2); (2,2) = [0, 0] gives f = 0: not negative
    exp = dict(rows=8, negative=[(0, 2), (2, 1), (3, 2)], min_value=0.2 - 0.45, min_row=(0, 2))
    yield "band", m, 21, exp
    # every E_in all-zero: rows = NE, min 0.0 at the first E_in, group -1, nothing negative
    yield "all_zero", np.zeros((3, 5, 3)), 21, dict(rows=3, negative=[], min_value=0.0, min_row=(0, -1))
    # a NaN moment inside the band is negative; the row's other values are finite
    n = np.zeros((2, 2, 2))
    n[0, 0] = [1.0, 0.0]
    n[0, 1] = [1.0, np.nan]
    n[1, 1] = [1.0, 0.1]
    yield "nan", n, 21, dict(rows=3, negative=[(0, 1)], min_value=0.35, min_row=(1, 1))


@pytest.mark.parametrize("case", list(hand_sections()), ids=lambda c: c[0])
def test_band_and_zero_row_rules_of_the_restatement(case):
    name, mat, M, exp = case
    got = np_positivity(mat, M)
    assert got["rows"] == exp["rows"] and got["negative"] == exp["negative"]
    assert got["min_row"] == exp["min_row"] and abs(got["min_value"] - exp["min_value"]) < 1e-15


# ---- condense ---------------------------------------------------------------------------------
def _loop_condense(mat, groups):
    NE, G, L = mat.shape
    out = np.zeros((NE, L))
    for iE in range(NE):
        acc = np.zeros(L)
        for g in range(G):
            if g in groups:
                acc = acc + mat[iE, g]
        out[iE] = acc
    return out


def test_condense_bit_identical_to_ascending_loop():
    from ndpp_amd import reader, validate
    rng = np.random.default_rng(5)
    mat = rng.standard_normal((40, 7, 6)) * 10.0 ** rng.uniform(-12, 2, (40, 7, 1))
    mat[3] = 0.0                                                   # an all-zero E_in
    mat[9, :2] = 0.0
    for groups in (None, [0, 1, 2, 3, 4, 5, 6], [6, 2, 4], [2, 4, 6, 4], [3], [0], [6]):
        want = _loop_condense(mat, range(7) if groups is None else set(groups))
        got = validate.condense(mat, groups)
        assert got.shape == (40, 6) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), groups
    sec = reader.ScattSection(np.arange(40.0), np.zeros(8, np.int32), np.ones(40, np.int32), np.ones(40, np.int32), mat)
    assert np.array_equal(validate.condense(sec, [1, 5]), _loop_condense(mat, {1, 5}))
    assert not validate.condense(mat, [1])[3].any()
    with pytest.raises(ValueError):
        validate.condense(mat, [7])


# ---- the C ABI: refusals before the device ------------------------------------------------------
def _pos_call(lib, n_ein=2, G=3, L=4, mat=None, nm=4, mu=None, n_mu=None, cap=5, rows=True, summary=True):
    import ndpp_amd
    mat = np.ones((max(n_ein, 1), G if G > 0 else 1, max(L, 1))) if mat is None else mat
    mu = np.linspace(-1, 1, 21) if mu is None else mu
    n_mu = len(mu) if n_mu is None else n_mu
    nr = np.zeros((max(cap, 1), 2), np.int32)
    s = ndpp_amd.Positivity()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    return lib.ndpp_scatt_positivity(n_ein, G, L, dp(mat) if isinstance(mat, np.ndarray) else None, nm, n_mu,
                                     dp(mu) if isinstance(mu, np.ndarray) else None, cap,
                                     nr.ctypes.data_as(C.POINTER(C.c_int)) if rows else None, None, None,
                                     C.byref(s) if summary else None)


def _exp_call(lib, n_ein=2, L=4, mom=True, nm=4, mu=None, n_mu=None, out=True):
    mu = np.linspace(-1, 1, 21) if mu is None else mu
    n_mu = len(mu) if n_mu is None else n_mu
    m = np.ones((2, 11))
    o = np.zeros(2 * 21)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    return lib.ndpp_expand_moments(n_ein, L, dp(m) if mom else None, nm, n_mu,
                                   dp(mu) if isinstance(mu, np.ndarray) else None, dp(o) if out else None)


BAD_MU = [np.array([-1.0, np.nan, 1.0]), np.array([-1.0, np.inf]), np.array([-np.inf, 0.0]),
          np.array([-1.0, 1.5]), np.array([np.nextafter(-1.0, -2.0), 0.0])]


def test_positivity_rejects_bad_arguments(hip):
    lib = hip.load()
    big = (1 << 31) - 1
    cases = [dict(L=0), dict(L=12, nm=4), dict(nm=0), dict(nm=5), dict(L=3, nm=4), dict(n_mu=0), dict(mu="null"),
             dict(mat="null"), dict(summary=False), dict(cap=-1), dict(rows=False), dict(n_ein=-1), dict(G=0),
             dict(n_ein=big, G=big, L=11, nm=11, mat=np.ones((1, 1, 11)))]
    cases += [dict(mu=m) for m in BAD_MU]
    for kw in cases:
        assert _pos_call(lib, **kw) == -22, kw
        assert lib.ndpp_last_error().startswith(b"scatt_positivity:"), (kw, lib.ndpp_last_error())
    # a cap whose output bytes overflow (the buffer behind neg_rows is never reached)
    import ndpp_amd
    mat, mu, nr, s = np.ones((1, 1, 4)), np.linspace(-1, 1, 3), np.zeros((1, 2), np.int32), ndpp_amd.Positivity()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ndpp_scatt_positivity(1, 1, 4, dp(mat), 4, 3, dp(mu), 1 << 62, nr.ctypes.data_as(C.POINTER(C.c_int)),
                                     None, None, C.byref(s)) == -22
    assert b"overflow" in lib.ndpp_last_error()


def test_expand_rejects_bad_arguments(hip):
    lib = hip.load()
    big = (1 << 31) - 1
    cases = [dict(L=0), dict(L=12), dict(nm=0), dict(nm=5), dict(n_mu=0), dict(mu="null"), dict(mom=False),
             dict(out=False), dict(n_ein=-1), dict(n_ein=big, n_mu=big, mu=np.linspace(-1, 1, 21))]
    cases += [dict(mu=m) for m in BAD_MU]
    for kw in cases:
        if kw.get("n_mu") == big:       # refused on its sizes before the 21-point grid is read
            rc = _exp_call(lib, n_ein=big, n_mu=big)
            assert b"overflow" in lib.ndpp_last_error()
        else:
            rc = _exp_call(lib, **kw)
        assert rc == -22, kw
        assert lib.ndpp_last_error().startswith(b"expand_moments:"), (kw, lib.ndpp_last_error())


def test_empty_section_needs_no_device(hip):
    """n_ein = 0 is a successful empty call: no rows, min +inf, no row named."""
    s, rows, rmin, rmu = hip.scatt_positivity(np.zeros((0, 3, 4)))
    assert (s.rows, s.negative, s.min_value, s.min_ein, s.min_group) == (0, 0, np.inf, -1, -1)
    assert rows.shape == (0, 2)
    f, mu = hip.expand_moments(np.zeros((0, 4)), mu_points=5)
    assert f.shape == (0, 5) and np.array_equal(mu, np.linspace(-1, 1, 5))


def test_no_device_no_fallback(hip):
    lib = hip.load()
    if lib.ndpp_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert _pos_call(lib) == -5
    assert _exp_call(lib) == -5
    with pytest.raises(hip.NdppError) as e:
        hip.scatt_positivity(np.ones((2, 3, 4)))
    assert e.value.code == -5
    from ndpp_amd import validate
    with pytest.raises(hip.NdppError):
        validate.expand(np.ones((2, 4)))


def test_cli_input_errors_exit_2(tmp_path):
    run = lambda *a: subprocess.run([sys.executable, "-m", "ndpp_amd.validate", *a], cwd=ROOT, capture_output=True,
                                    text=True, timeout=120)
    r = run(str(tmp_path / "missing"))
    assert r.returncode == 2 and "cannot read" in r.stderr
    (tmp_path / "ndpp_lib.xml").write_text('<ndpp_lib><filetype> hdf5 </filetype>\n'
                                           '<ndpp_table name="x" path="x.g2"/></ndpp_lib>')
    r = run(str(tmp_path))
    assert r.returncode == 2 and "hdf5" in r.stderr
    (tmp_path / "ndpp_lib.xml").write_text('<ndpp_lib><filetype> binary </filetype>\n'
                                           '<ndpp_table name="x" path="x.g2"/></ndpp_lib>')
    r = run(str(tmp_path))
    assert r.returncode == 2 and "x.g2" in r.stderr
    assert run(str(tmp_path), "--mu-points", "0").returncode == 2


def test_cli_without_device_exits_2(hip):
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a HIP device is present")
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.validate", str(ROOT / "tests/golden/e2e/chi_sab")], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error -5" in r.stderr
