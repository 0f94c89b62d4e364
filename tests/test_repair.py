"""Repair of negative rows, host side (ndpp_scatt_repair's argument checks, ndpp_amd.repair.weights
and the command lines' refusals): the C ABI's refusals before any device work, the weights against
the multiplication order include/ndpp_hip.h writes down, and the exit statuses of the flags.
tests/test_gpu_repair.py holds the kernel to the certificate and to closed forms."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_run_inputs import case1, listing

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps


def _call(lib, n_ein=2, G=3, L=4, mode=0, steps=20, undecided=0, rel_tol=1e-10, mat=True, out=True, t=True,
          how=True, summary=True, evals=None):
    import ndpp_amd
    n = max(n_ein, 1) * max(G, 1) if n_ein < 1000 else 1
    m = np.ones((n, max(L, 1)))
    a_out, a_t, a_how = np.zeros((n, max(L, 1))), np.zeros(n), np.zeros(n, np.int32)
    s = ndpp_amd.Repair()
    dp = lambda a, on: a.ctypes.data_as(C.POINTER(C.c_double)) if on else None
    args = [n_ein, G, L, dp(m, mat), mode, steps, undecided, rel_tol, dp(a_out, out), dp(a_t, t),
            a_how.ctypes.data_as(C.POINTER(C.c_int)) if how else None]
    if evals is None:
        return lib.ndpp_scatt_repair(*args, C.byref(s) if summary else None)
    a_ev = np.zeros(n, np.int32)
    return lib.ndpp_scatt_repair_evals(*args, a_ev.ctypes.data_as(C.POINTER(C.c_int)) if evals else None,
                                       C.byref(s) if summary else None)


def test_repair_rejects_bad_arguments(hip):
    lib = hip.load()
    big = (1 << 31) - 1
    cases = [(dict(L=0), b"L=0"), (dict(L=12), b"L=12"), (dict(G=0), b"G=0"), (dict(n_ein=-1), b"n_ein=-1"),
             (dict(mode=3), b"mode=3"), (dict(mode=-1), b"mode=-1"), (dict(steps=0), b"steps=0"),
             (dict(steps=53), b"steps=53"), (dict(rel_tol=-1e-12), b"rel_tol"), (dict(rel_tol=np.nan), b"rel_tol"),
             (dict(rel_tol=np.inf), b"rel_tol"), (dict(mat=False), b"NULL"), (dict(out=False), b"NULL"),
             (dict(t=False), b"NULL"), (dict(how=False), b"NULL"), (dict(summary=False), b"NULL"),
             (dict(evals=False), b"NULL evals"), (dict(n_ein=big, G=big, L=11), b"overflow")]
    for kw, word in cases:
        assert _call(lib, **kw) == -22, kw
        msg = lib.ndpp_last_error()
        assert msg.startswith(b"scatt_repair:") and word in msg, (kw, msg)


def test_empty_section_needs_no_device(hip):
    s, out, t, how = hip.scatt_repair(np.zeros((0, 3, 4)))
    assert (s.rows, s.repaired, s.heat, s.uniform, s.unrepairable, s.nonfinite) == (0, 0, 0, 0, 0, 0)
    assert (s.min_t, s.min_ein, s.min_group) == (1.0, -1, -1)
    assert out.shape == (0, 3, 4) and t.shape == how.shape == (0, 3)
    for mode in (hip.REPAIR_BEST, hip.REPAIR_HEAT, hip.REPAIR_UNIFORM):
        assert hip.scatt_repair(np.zeros((0, 1, 1)), mode=mode, steps=52, rel_tol=0.0)[0].rows == 0


def test_no_device_no_fallback(hip):
    lib = hip.load()
    if lib.ndpp_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert _call(lib) == -5
    assert _call(lib, evals=True) == -5
    with pytest.raises(hip.NdppError) as e:
        hip.scatt_repair(np.ones((2, 3, 4)))
    assert e.value.code == -5
    from ndpp_amd import repair
    with pytest.raises(hip.NdppError):
        repair.repair_sections(np.ones((2, 3, 4)))


def _weights_by_hand(t, L, family):
    """the order of include/ndpp_hip.h, one Python float product at a time"""
    w = [1.0] * L
    if L > 1:
        w[1] = t
    p = t
    for l in range(2, L):
        if family == "heat":
            p = p * t
            w[l] = w[l - 1] * p
        else:
            w[l] = t
    return np.array(w)


def test_weights():
    from ndpp_amd import repair
    ts = [0.0, 0.5, 0.7310791015625, 1.0 - 2.0 ** -20, 0.1, 1.0]
    for L in (1, 2, 3, 11):
        for fam, how in (("heat", 1), ("uniform", 2)):
            assert (repair.weights(1.0, L, fam) == 1.0).all()
            for t in ts:
                w = repair.weights(t, L, fam)
                assert w.shape == (L,) and w[0] == 1.0
                assert w.tobytes() == _weights_by_hand(t, L, fam).tobytes(), (L, fam, t)
                assert w.tobytes() == repair.weights(t, L, how).tobytes()
            many = repair.weights(np.array(ts), L, fam)              # an array of t: one row each
            assert many.shape == (len(ts), L)
            assert all(many[k].tobytes() == repair.weights(t, L, fam).tobytes() for k, t in enumerate(ts))
    l = np.arange(11)
    tri = l * (l + 1) // 2
    w = repair.weights(0.5, 11, "heat")
    assert (np.abs(w - 0.5 ** tri) <= 4 * EPS * 0.5 ** tri).all()
    for t in (0.5, 0.25, 0.125):                                     # a power of two: every product is exact
        assert (repair.weights(t, 11, "heat") == t ** tri.astype(float)).all()
    assert (repair.weights(0.3, 11, "uniform")[1:] == 0.3).all()
    for bad in ("best", 0, 3, None):
        with pytest.raises(ValueError):
            repair.weights(0.5, 3, bad)
    with pytest.raises(ValueError):
        repair.weights(0.5, 0, "heat")


def test_largest_change_metric():
    from ndpp_amd import repair
    mat = np.zeros((2, 3, 2))
    mat[0, :, 0] = [1.0, -4.0, 2.0]
    mat[1, :, 0] = [0.0, 0.5, 0.0]
    out = mat.copy()
    assert repair.largest_change(mat, out) == (0.0, -1, -1)
    out[0, 2, 1] = 0.2          # 0.2 / max_g |P0| = 0.2 / 4
    out[1, 1, 1] = -0.01        # 0.01 / 0.5
    assert repair.largest_change(mat, out) == (0.05, 0, 2)
    out[1, 1, 1] = -0.1
    assert repair.largest_change(mat, out) == (0.2, 1, 1)
    assert repair.largest_change(np.zeros((0, 3, 2)), np.zeros((0, 3, 2))) == (0.0, -1, -1)


def _run(*args):
    return subprocess.run([sys.executable, "-m", "ndpp_amd.run", *map(str, args)], cwd=ROOT, capture_output=True,
                          text=True, timeout=120)


def test_run_refusals_exit_2_and_write_nothing(tmp_path):
    from test_run_inputs import set_tag
    run = case1(tmp_path / "run")
    before = listing(run)
    for flags, word in ((["--repair-mode", "heat"], "--repair-mode"), (["--repair-steps", 8], "--repair-steps"),
                        (["--repair-rel-tol", 1e-8], "--repair-rel-tol"), (["--repair-undecided"], "--repair-undecided"),
                        (["--repair-positivity", "--repair-steps", 0], "--repair-steps"),
                        (["--repair-positivity", "--repair-steps", 53], "--repair-steps"),
                        (["--repair-positivity", "--repair-rel-tol=-1e-12"], "--repair-rel-tol"),
                        (["--repair-positivity", "--repair-rel-tol", "nan"], "--repair-rel-tol"),
                        (["--repair-positivity", "--repair-rel-tol", "inf"], "--repair-rel-tol")):
        r = _run(run, *flags)
        assert r.returncode == 2 and word in r.stderr and "input error" in r.stderr, (flags, r.stderr)
        assert listing(run) == before
    r = _run(run, "--repair-positivity", "--repair-mode", "sharpest")     # argparse's own refusal
    assert r.returncode == 2 and listing(run) == before
    set_tag(run, "scatt_type", "tabular")
    r = _run(run, "--repair-positivity")
    assert r.returncode == 2 and "--repair-positivity" in r.stderr and "tabular" in r.stderr
    assert listing(run) == before


def test_validate_repair_report_needs_certified():
    lib_dir = ROOT / "tests" / "golden" / "e2e" / "chi_sab"
    cli = lambda *a: subprocess.run([sys.executable, "-m", "ndpp_amd.validate", str(lib_dir), *map(str, a)], cwd=ROOT,
                                    capture_output=True, text=True, timeout=120)
    r = cli("--repair-report")
    assert r.returncode == 2 and "--certified" in r.stderr and r.stdout == ""
    r = cli("--certified", "--repair-report", "--moments", 3)
    assert r.returncode == 2 and "--moments" in r.stderr and r.stdout == ""
