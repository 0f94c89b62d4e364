"""Certified positivity, host side (ndpp_scatt_minimum's argument checks, ndpp_amd.validate's
minimum_reference and the --certified flag): the C ABI's refusals before any device work, the host
reference on rows whose minimum is known in closed form, and the command line's own refusals.
tests/test_gpu_minimum.py holds the kernel to minimum_reference."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

# f(mu) = (mu - 0.05)^2 - 1e-4 as moments: +0.0024 at its smallest value on linspace(-1, 1, 21),
# -1e-4 at mu = 0.05
PLANTED = np.array([2 / 3 + 2 * (0.0025 - 1e-4), -0.2 / 3, 4 / 15])


def _min_call(lib, n_ein=2, G=3, L=4, nm=4, rel_tol=1e-10, mat=True, lo=True, hi=True, mu=True, cls=True,
              summary=True, evals=None):
    import ndpp_amd
    n = max(n_ein, 1) * max(G, 1) if n_ein < 1000 else 1
    m = np.ones((n, max(L, 1)))
    a_lo, a_hi, a_mu, a_cls = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    s = ndpp_amd.Minimum()
    dp = lambda a, on: a.ctypes.data_as(C.POINTER(C.c_double)) if on else None
    args = [n_ein, G, L, dp(m, mat), nm, rel_tol, dp(a_lo, lo), dp(a_hi, hi), dp(a_mu, mu),
            a_cls.ctypes.data_as(C.POINTER(C.c_int)) if cls else None]
    if evals is None:
        return lib.ndpp_scatt_minimum(*args, C.byref(s) if summary else None)
    a_ev = np.zeros(n, np.int32)
    return lib.ndpp_scatt_minimum_evals(*args, a_ev.ctypes.data_as(C.POINTER(C.c_int)) if evals else None,
                                        C.byref(s) if summary else None)


def test_minimum_rejects_bad_arguments(hip):
    lib = hip.load()
    big = (1 << 31) - 1
    cases = [(dict(L=0), b"L=0"), (dict(L=12, nm=4), b"L=12"), (dict(nm=0), b"n_moments=0"),
             (dict(nm=5), b"n_moments=5"), (dict(L=3, nm=4), b"n_moments=4"), (dict(G=0), b"G=0"),
             (dict(n_ein=-1), b"n_ein=-1"), (dict(rel_tol=-1e-12), b"rel_tol"), (dict(rel_tol=np.nan), b"rel_tol"),
             (dict(rel_tol=np.inf), b"rel_tol"), (dict(mat=False), b"NULL"), (dict(lo=False), b"NULL"),
             (dict(hi=False), b"NULL"), (dict(mu=False), b"NULL"), (dict(cls=False), b"NULL"),
             (dict(summary=False), b"NULL"), (dict(evals=False), b"NULL evals"),
             (dict(n_ein=big, G=big, L=11, nm=11), b"overflow")]
    for kw, word in cases:
        assert _min_call(lib, **kw) == -22, kw
        msg = lib.ndpp_last_error()
        assert msg.startswith(b"scatt_minimum:") and word in msg, (kw, msg)


def test_empty_section_needs_no_device(hip):
    """n_ein = 0 is a successful empty call: no rows, min_hi +inf, no row named."""
    s, lo, hi, mu_at, cls = hip.scatt_minimum(np.zeros((0, 3, 4)))
    assert (s.rows, s.negative, s.undecided, s.nonfinite, s.unsettled) == (0, 0, 0, 0, 0)
    assert (s.min_hi, s.min_mu, s.min_ein, s.min_group) == (np.inf, 0.0, -1, -1)
    assert lo.shape == hi.shape == mu_at.shape == cls.shape == (0, 3)
    assert hip.scatt_minimum(np.zeros((0, 3, 4)), rel_tol=0.0)[0].rows == 0       # rel_tol = 0 is legal


def test_no_device_no_fallback(hip):
    lib = hip.load()
    if lib.ndpp_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert _min_call(lib) == -5
    assert _min_call(lib, evals=True) == -5
    with pytest.raises(hip.NdppError) as e:
        hip.scatt_minimum(np.ones((2, 3, 4)))
    assert e.value.code == -5
    from ndpp_amd import validate
    with pytest.raises(hip.NdppError):
        validate.minimum(np.ones((2, 3, 4)))


def test_minimum_reference_on_known_rows():
    from ndpp_amd import validate
    # the planted dip: the 21-point grid sees +0.0024, the minimum is -1e-4 at 0.05
    from numpy.polynomial import legendre as leg
    c = (np.arange(3) + 0.5) * PLANTED
    grid = leg.legval(np.linspace(-1, 1, 21), c)
    assert abs(grid.min() - 0.0024) < 1e-12
    v, mu = validate.minimum_reference(PLANTED)
    assert abs(v + 1e-4) <= 1e-15 and abs(mu - 0.05) <= 1e-12
    # 1 + mu: c = [1, 1], a = [2, 2/3]: 0 at mu = -1
    assert validate.minimum_reference([2.0, 2.0 / 3.0]) == (0.0, -1.0)
    # a P0-only row: the constant itself, (l + 1/2) a_0 = a_0 / 2
    assert validate.minimum_reference([3.0]) == (1.5, -1.0)
    assert validate.minimum_reference([3.0, 0.0, 0.0]) == (1.5, -1.0)
    # truncation: only the first n_moments moments count
    assert validate.minimum_reference([2.0, 2.0 / 3.0, 9.0], n_moments=2) == (0.0, -1.0)
    # 1 - mu^2 = 2/3 P0 - 2/3 P2: interior maximum, the minimum 0 at both ends, the first reported
    v, mu = validate.minimum_reference([4.0 / 3.0, 0.0, -4.0 / 15.0])
    assert abs(v) <= 1e-15 and mu == -1.0


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "ndpp_amd.validate", *map(str, args)], cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


def test_cli_certified_refusals_exit_2():
    lib_dir = ROOT / "tests" / "golden" / "e2e" / "chi_sab"
    r = _cli(lib_dir, "--certified", "--mu-points", 21)
    assert r.returncode == 2 and "--mu-points" in r.stderr and r.stdout == ""
    r = _cli(lib_dir, "--rel-tol", 1e-8)
    assert r.returncode == 2 and "--certified" in r.stderr
    r = _cli(lib_dir, "--certified", "--rel-tol", -1)
    assert r.returncode == 2 and "--rel-tol" in r.stderr


def test_cli_certified_without_device_exits_2(hip):
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a HIP device is present")
    r = _cli(ROOT / "tests/golden/e2e/chi_sab", "--certified")
    assert r.returncode == 2 and "error -5" in r.stderr
