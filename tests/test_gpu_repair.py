"""Repair of negative rows on the GPU (ndpp_scatt_repair, ndpp_amd.repair, --repair-positivity).
Every judgement is made by an entry point that was there before and has its own tests
(ndpp_scatt_minimum, validate.minimum_reference, `validate --certified`, the reader) or by a closed
form, never by the code under test:

  certified  a repaired row, passed again through ndpp_scatt_minimum at the same rel_tol, is POSITIVE,
             and minimum_reference (the roots of f') finds its minimum >= -1e-13 S -- the tolerance
             of tests/test_gpu_minimum.py: legval at degree <= 10 rounds to about 2e-15 S
  tight      the row at t + 2^-steps, built with repair.weights in the same family, is not POSITIVE:
             the failing end of the last bracket
  exact      out == mat * weights(t, L, how) bit for bit on repaired rows, every other entry and the
             whole P0 column are the input's bits"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ace_synth
from synth import ace_adist
from test_minimum import PLANTED

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-13
HEAT, UNIFORM = 1, 2


def scale(rows):
    rows = np.asarray(rows, dtype=np.float64)
    return (np.abs(rows) * (np.arange(rows.shape[-1]) + 0.5)).sum(axis=-1)


def planted_section():
    """3 x 4 x 3, as in tests/test_gpu_minimum.py: the planted dip at (1, 2) among positive rows"""
    m = np.zeros((3, 4, 3))
    m[0, 1] = [1.0, 0.1, 0.0]
    m[0, 2] = [0.5, 0.0, 0.05]
    m[1, 0] = [0.3, 0.05, 0.0]
    m[1, 2] = PLANTED
    m[1, 3] = [2.0, -0.2, 0.1]
    m[2, 3] = [1.0, 0.0, 0.0]
    return m


@pytest.fixture(scope="module")
def seeded(hip):
    """64 E_in x 7 groups x 11 moments like test_gpu_minimum's p10 (every P0 > 0, a mix of positive and
    negative rows), with the classes ndpp_scatt_minimum gives them; read only"""
    rng = np.random.default_rng(20251018)
    mat = rng.standard_normal((64, 7, 11)) * np.exp(-0.3 * np.arange(11)) * rng.choice([0.05, 0.15, 0.5], (64, 7, 1))
    mat[:, :, 0] = np.abs(rng.standard_normal((64, 7))) + 0.05
    kind = hip.scatt_minimum(mat)[4] & 3
    assert 100 < (kind == hip.MIN_NEGATIVE).sum() < 400
    mat.setflags(write=False)
    kind.setflags(write=False)
    return mat, kind


def check_repair(hip, mat, res, steps=20, rel_tol=1e-10, undecided=False, family=None):
    """who is repaired, exact, certified and tight (module docstring); returns the mask of repaired rows"""
    from ndpp_amd import repair, validate
    s, out, t, how = res
    L = mat.shape[2]
    cls0 = hip.scatt_minimum(mat, rel_tol=rel_tol)[4]
    exam, kind0 = cls0 >= 0, cls0 & 3
    want = exam & ((kind0 == hip.MIN_NEGATIVE) | ((kind0 == hip.MIN_UNDECIDED) & bool(undecided)))
    rep = want & (mat[:, :, 0] >= 0.0)
    # who
    assert (((how == HEAT) | (how == UNIFORM)) == rep).all()
    assert ((how == 3) == (want & (mat[:, :, 0] < 0.0))).all()
    assert ((how == 4) == (exam & (kind0 == hip.MIN_NONFINITE))).all()
    assert ((how == -1) == ~exam).all() and (t[~exam] == -1.0).all()
    assert (t[exam & ~rep] == 1.0).all() and ((t[rep] >= 0.0) & (t[rep] < 1.0)).all()
    if family is not None:
        assert (how[rep] == family).all()
    assert (s.rows, s.repaired, s.heat, s.uniform, s.unrepairable, s.nonfinite) == (
        exam.sum(), rep.sum(), (how == HEAT).sum(), (how == UNIFORM).sum(), (how == 3).sum(), (how == 4).sum())
    if rep.any():
        k = np.argwhere(rep & (t == t[rep].min()))[0]
        assert (s.min_t, s.min_ein, s.min_group) == (t[rep].min(), k[0], k[1])
    else:
        assert (s.min_t, s.min_ein, s.min_group) == (1.0, -1, -1)
    # exact: the repaired rows are the products, everything else (and all of P0) the input's bits
    expect, probe = mat.copy(), None
    for fam in (HEAT, UNIFORM):
        m = how == fam
        expect[m] = mat[m] * repair.weights(t[m], L, fam)
    assert out.tobytes() == expect.tobytes()
    assert out[:, :, 0].tobytes() == mat[:, :, 0].tobytes()
    # certified, by the entry point that was there before and by the roots of f'
    cls1 = hip.scatt_minimum(out, rel_tol=rel_tol)[4]
    assert ((cls1[rep] & 3) == hip.MIN_POSITIVE).all()
    S = scale(out)
    for i, g in np.argwhere(rep):
        assert validate.minimum_reference(out[i, g])[0] >= -TOL * S[i, g], (i, g)
    # tight: one step up fails
    probe = out.copy()
    for fam in (HEAT, UNIFORM):
        m = how == fam
        probe[m] = mat[m] * repair.weights(t[m] + 2.0 ** -steps, L, fam)
    cls2 = hip.scatt_minimum(probe, rel_tol=rel_tol)[4]
    assert ((cls2[rep] & 3) != hip.MIN_POSITIVE).all()
    return rep


def test_planted_row_closed_form(hip):
    """uniform mode on f = (mu - 0.05)^2 - 1e-4: f_t = c_0 + t (f - c_0) has the minimum
    c_0 - t (c_0 + 1e-4), which is >= 0 up to s* = c_0 / (c_0 + 1e-4), c_0 = a_0 / 2.
    0 <= s* - t: a t above s* has a negative minimum and cannot be certified.  s* - t <= 2^-steps + 1e-8:
    the bracket's width plus the certificate's own margin -- it passes a row only when its minimum is
    above rel_tol S + E = 1e-10 S + 256 eps S with S = sum (l + 1/2)|a_l| < 1.2 here, i.e. 1.2e-10, which
    over the slope c_0 + 1e-4 = 0.336 is 3.6e-10 in t; 1e-8 covers it (derived, not tuned)."""
    m = planted_section()
    steps = 20
    res = hip.scatt_repair(m, mode=hip.REPAIR_UNIFORM, steps=steps)
    rep = check_repair(hip, m, res, steps=steps, family=UNIFORM)
    assert np.argwhere(rep).tolist() == [[1, 2]] and res[0].rows == 7
    c0 = PLANTED[0] / 2
    s_star = c0 / (c0 + 1e-4)
    t = res[2][1, 2]
    print(f"planted: t {t!r}, s* {s_star!r}, s* - t {s_star - t:.3e} (2^-steps {2.0 ** -steps:.3e})")
    assert 0.0 <= s_star - t <= 2.0 ** -steps + 1e-8
    # how, t and the other rows
    assert res[3].tolist() == [[-1, 0, 0, -1], [0, 0, UNIFORM, 0], [-1, -1, -1, 0]]
    # the report of the Python layer
    from ndpp_amd import repair
    secs, report = repair.repair_sections(m, mode="uniform", steps=steps)
    assert secs["section"]["mat"].tobytes() == res[1].tobytes()
    r = report.sections["section"]
    assert (r.rows, r.repaired, r.heat, r.uniform, r.min_ein, r.min_group) == (7, 1, 0, 1, 1, 2) and r.min_t == t
    change = np.abs(res[1][1, 2] - m[1, 2]).max() / 2.0               # max_g |P0| of E_in 1 is 2.0
    assert (r.max_change, r.max_change_ein, r.max_change_group) == (change, 1, 2)
    assert "repaired 1 of 7 rows" in repair.format_lines("planted", report)[0]


@pytest.mark.parametrize("L", [1, 2, 3, 6, 11])
def test_every_number_of_moments(hip, seeded, L):
    mat = np.ascontiguousarray(seeded[0][:24, :, :L])
    if L == 1:          # f = a_0 / 2: the only rows to act on are interior ones with P0 <= 0
        mat[3, 2, 0], mat[5, 4, 0] = -0.25, 0.0
    res = hip.scatt_repair(mat)
    rep = check_repair(hip, mat, res)
    print(f"L = {L}: {rep.sum()} of {rep.size} rows repaired, heat {res[0].heat}, uniform {res[0].uniform}, "
          f"smallest t {res[0].min_t:.6f}")
    assert rep.any() == (L > 1)
    if L == 1:
        assert res[3][3, 2] == 3 and res[3][5, 4] == 0 and res[0].unrepairable == 1


def test_seeded_section_and_repeatable_bits(hip, seeded):
    mat = seeded[0]
    a = hip.scatt_repair(mat, want_evals=True)
    rep = check_repair(hip, mat, a[:4])
    evals = a[4]
    print(f"seeded: {rep.sum()} rows repaired (heat {a[0].heat}, uniform {a[0].uniform}), smallest t {a[0].min_t:.6f}; "
          f"evaluations per repaired row mean {evals[rep].mean():.0f} max {evals[rep].max()}")
    assert a[0].heat > 0 and a[0].uniform > 0                          # neither family alone is right
    assert (evals[~rep] == 0).all() and (evals[rep] >= 2 * 20 * 130).all()
    assert (evals[rep] <= 2 * 20 * hip.MIN_MAX_EVALS).all()
    b = hip.scatt_repair(mat, want_evals=True)
    assert bytes(a[0]) == bytes(b[0])
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    assert hip.scatt_repair(mat)[1].tobytes() == a[1].tobytes()


def test_one_energy_of_seventy_groups(hip, seeded):
    mat = np.ascontiguousarray(seeded[0].reshape(-1, 11)[:70].reshape(1, 70, 11))
    res = hip.scatt_repair(mat)
    rep = check_repair(hip, mat, res)
    assert rep.sum() == (seeded[1].ravel()[:70] == hip.MIN_NEGATIVE).sum() > 0
    # a row's repair does not depend on where it sits
    tall = hip.scatt_repair(np.ascontiguousarray(mat.reshape(70, 1, 11)))
    assert tall[1].tobytes() == res[1].tobytes() and tall[2].tobytes() == res[2].tobytes()
    assert tall[3].tobytes() == res[3].tobytes()


@pytest.mark.parametrize("n_list", [1, 63, 64, 65])
def test_list_lengths_at_the_wave_boundary(hip, seeded, n_list):
    """the kernel takes one lane per LISTED row in blocks of one wave: lists that fill no wave, one wave
    less a lane, one wave exactly, and a wave and a lane"""
    rows, kind = seeded[0].reshape(-1, 11), seeded[1].ravel()
    neg, pos = np.flatnonzero(kind == hip.MIN_NEGATIVE)[:n_list], np.flatnonzero(kind == hip.MIN_POSITIVE)[:9]
    pick = np.sort(np.concatenate([neg, pos]))
    mat = np.ascontiguousarray(rows[pick].reshape(-1, 1, 11))
    res = hip.scatt_repair(mat)
    rep = check_repair(hip, mat, res)
    assert rep.sum() == n_list == res[0].repaired
    whole = hip.scatt_repair(seeded[0])                                 # the same rows inside the full section
    assert res[1].reshape(-1, 11).tobytes() == whole[1].reshape(-1, 11)[pick].tobytes()
    assert res[2].ravel().tobytes() == whole[2].ravel()[pick].tobytes()


def moments_by_quadrature(f, L):
    """a_l = integral of f P_l over [-1, 1], by 64-point Gauss-Legendre"""
    from numpy.polynomial import legendre as leg
    x, w = leg.leggauss(64)
    return np.array([np.sum(w * f(x) * leg.legval(x, np.eye(L)[l])) for l in range(L)])


def test_modes(hip, seeded):
    mat = seeded[0]
    best, heat, unif = (hip.scatt_repair(mat, mode=m) for m in (hip.REPAIR_BEST, hip.REPAIR_HEAT, hip.REPAIR_UNIFORM))
    rep = check_repair(hip, mat, heat, family=HEAT)
    assert (check_repair(hip, mat, unif, family=UNIFORM) == rep).all()
    take_u = unif[2] >= heat[2]                                       # uniform on a tie
    assert (best[3][rep] == np.where(take_u, UNIFORM, HEAT)[rep]).all()
    assert (best[2] == np.where(take_u, unif[2], heat[2])).all()
    assert best[1].tobytes() == np.where(take_u[:, :, None], unif[1], heat[1]).tobytes()
    # the first and third rows of DESIGN.md section 16's table: a mild ripple keeps more under the
    # uniform blend, a truncated peak under the heat kernel
    mild = moments_by_quadrature(lambda x: np.exp(10.0 * (x - 1.0)), 11).reshape(1, 1, 11)
    peak = moments_by_quadrature(lambda x: np.exp(30.0 * (x - 1.0)), 8).reshape(1, 1, 8)
    for m, fam in ((mild, UNIFORM), (peak, HEAT)):
        res = hip.scatt_repair(m)
        check_repair(hip, m, res, family=fam)
        h, u = hip.scatt_repair(m, mode=hip.REPAIR_HEAT)[2][0, 0], hip.scatt_repair(m, mode=hip.REPAIR_UNIFORM)[2][0, 0]
        print(f"L = {m.shape[2]}: P1 kept, heat {h:.4f}, uniform {u:.4f}")
        assert res[2][0, 0] == max(h, u) and (u >= h) == (fam == UNIFORM)


def test_classes(hip):
    L = 11
    row = lambda a: np.pad(np.asarray(a, dtype=np.float64), (0, L - len(a)))
    m = np.zeros((4, 4, L))
    m[0, 0] = row([1.0, 0.1])
    m[0, 1] = row([-0.5, 0.1, 0.02])               # a_0 < 0 inside the band: unrepairable
    m[0, 2] = row([0.0, 0.3, -0.1])                # a_0 = 0, negative somewhere: the zero row
    m[0, 3] = row([1.0, 0.2])
    m[1, 0] = row([1.0])
    m[1, 1] = row([1.0, 0.0, 0.0, np.nan])         # a NaN moment
    m[1, 2] = row([2.0, 2.0 / 3.0])                # 1 + mu: 0 at mu = -1, UNDECIDED
    m[1, 3] = row([1.0, 0.9])                      # 0.5 + 1.35 mu: negative
    m[2, 1] = row([0.0, 5.0])                      # E_in 2: no P0 > 0 anywhere
    m[3, 1] = row([1.0, 0.1])                      # E_in 3: band 1..2
    m[3, 2] = row([0.5, -0.1])
    m[3, 3] = row([0.0, 7.0])                      # outside the band
    kind = hip.scatt_minimum(m)[4] & 3
    assert kind[1, 2] == hip.MIN_UNDECIDED and kind[0, 2] == hip.MIN_NEGATIVE
    res = hip.scatt_repair(m)
    check_repair(hip, m, res)
    s, out, t, how = res
    assert how.tolist() == [[0, 3, UNIFORM, 0], [0, 4, 0, how[1, 3]], [0, -1, -1, -1], [-1, 0, 0, -1]]
    assert how[1, 3] in (HEAT, UNIFORM) and 0.0 < t[1, 3] < 1.0
    assert (s.rows, s.repaired, s.unrepairable, s.nonfinite) == (11, 2, 1, 1)
    assert t[0, 2] == 0.0 and not out[0, 2].any() and (s.min_t, s.min_ein, s.min_group) == (0.0, 0, 2)
    assert out[0, 1].tobytes() == m[0, 1].tobytes() and out[1, 1].tobytes() == m[1, 1].tobytes()
    assert out[2].tobytes() == m[2].tobytes() and out[3].tobytes() == m[3].tobytes()
    assert out[1, 2].tobytes() == m[1, 2].tobytes()
    # the zero row in the heat family too
    h = hip.scatt_repair(m, mode=hip.REPAIR_HEAT)
    assert h[3][0, 2] == HEAT and h[2][0, 2] == 0.0 and not h[1][0, 2].any()
    # the undecided row on request: repaired, and POSITIVE afterwards (check_repair)
    res = hip.scatt_repair(m, undecided=True)
    rep = check_repair(hip, m, res, undecided=True)
    assert rep[1, 2] and res[0].repaired == 3 and 0.0 < res[2][1, 2] < 1.0


@pytest.mark.parametrize("steps", [1, 52])
def test_fewest_and_most_steps(hip, seeded, steps):
    mat = np.ascontiguousarray(seeded[0][:12])
    res = hip.scatt_repair(mat, steps=steps)
    rep = check_repair(hip, mat, res, steps=steps)
    assert rep.any()
    if steps == 1:
        assert np.isin(res[2][rep], [0.0, 0.5]).all()


# ---- end to end: the driver with and without --repair-positivity, judged by `validate --certified` ----

H1 = "1001.71c"


def h1_like():
    """An H-1-like table: A = 0.999167, elastic scattering isotropic in the centre of mass off a target
    at rest (no free-gas range: the run stays cheap) and capture; two groups, P5.  Scattering off a
    target of the neutron's mass puts each outgoing group into a band of lab cosines
    (mu = sqrt(E'/E)), and a band truncated at P5 rings below zero.  extend_pts is the reference's
    default 50: at this mass the down-scatter points above a group edge are spaced by
    7 ln(1 / alpha) / extend_pts = 109 / extend_pts in ln E, and the grid builder refuses a run in which
    none of them lies below the next edge (ln(20 / 0.1) = 5.3: at least 21)."""
    kT = 2.5301e-8
    n_grid = 30
    energy = 1e-11 * (20.0 / 1e-11) ** (np.arange(n_grid) / (n_grid - 1.0))
    reactions = [dict(MT=2, Q=0.0, mult=1, thr=1, in_cm=1, sigma=None,
                      adist=ace_adist([1e-11, 20.0], ["iso", "iso"], seed=1), edists=[]),
                 dict(MT=102, Q=2.2, mult=0, thr=1, in_cm=0, sigma=0.3 / np.sqrt(energy / 1e-11), adist=None, edists=[])]
    return ace_synth.quantise(dict(awr=0.999167, kT=kT, freegas_cutoff=0.0, energy=energy,
                                   elastic=20.0 / (1.0 + energy), reactions=reactions,
                                   bins=np.array([0.0, 0.1, 20.0]), order=5, mu_bins=129, extend_pts=50,
                                   inel_extend_pts=3))


def _child(module, *args):
    r = subprocess.run([sys.executable, "-m", module, *map(str, args)], cwd=ROOT, capture_output=True, text=True,
                       timeout=240)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_driver_end_to_end(tmp_path):
    from ndpp_amd import reader
    runs = {}
    for name, flags in (("plain", []), ("repaired", ["--repair-positivity"])):
        run = tmp_path / name
        ace_synth.write_inputs(run, H1, h1_like(), scatt_order=5, mu_bins=129, extend_pts=50, inel_extend_pts=3,
                               nuscatter=False, threads=1)
        assert _child("ndpp_amd.run", run, *flags, "--json", tmp_path / f"{name}.json").returncode == 0
        runs[name] = run
    # the plain library has rows that go negative (so the test bites); the repaired one has none
    r = _child("ndpp_amd.validate", runs["plain"], "--certified", "--repair-report", "--json", tmp_path / "v0.json")
    assert r.returncode == 1 and "a repair (best, 20 steps) would change" in r.stdout
    v0 = json.loads((tmp_path / "v0.json").read_text())["tables"][H1]
    negative = sum(s["negative"] for s in v0["sections"].values())
    assert negative >= 1 and v0["repair"]["repaired"] == negative
    r = _child("ndpp_amd.validate", runs["repaired"], "--certified", "--json", tmp_path / "v1.json")
    assert r.returncode == 0
    v1 = json.loads((tmp_path / "v1.json").read_text())["tables"][H1]
    assert all(s["negative"] == 0 and s["nonfinite"] == 0 for s in v1["sections"].values())
    assert {k: s["rows"] for k, s in v1["sections"].items()} == {k: s["rows"] for k, s in v0["sections"].items()}
    # grids, gmin / gmax and every P0 are the plain library's bits; the header carries no mark
    a, b = ((runs[k] / f"{H1}.g2").read_bytes() for k in ("plain", "repaired"))
    ta, tb = reader.read_binary(a), reader.read_binary(b)
    assert len(a) == len(b) and a != b
    changed = 0
    for sec in ("elastic", "inelastic", "nuinelastic"):
        x, y = getattr(ta, sec), getattr(tb, sec)
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert x.ein.tobytes() == y.ein.tobytes() and x.group_index.tobytes() == y.group_index.tobytes()
        assert np.array_equal(x.gmin, y.gmin) and np.array_equal(x.gmax, y.gmax)
        assert x.mat[:, :, 0].tobytes() == y.mat[:, :, 0].tobytes()
        changed += int((x.mat != y.mat).any(axis=2).sum())
    assert changed == negative
    assert (runs["plain"] / "ndpp_lib.xml").read_text().replace(str(runs["plain"].resolve()), "RUN") == \
        (runs["repaired"] / "ndpp_lib.xml").read_text().replace(str(runs["repaired"].resolve()), "RUN")
    # --json carries the report, and only with the flag
    assert "repair" not in json.loads((tmp_path / "plain.json").read_text())
    rep = json.loads((tmp_path / "repaired.json").read_text())["repair"]
    assert (rep["mode"], rep["steps"], rep["rel_tol"], rep["undecided"]) == ("best", 20, 1e-10, False)
    assert [t["name"] for t in rep["tables"]] == [H1]
    el = rep["tables"][0]["sections"]["elastic"]
    assert sum(s["repaired"] for s in rep["tables"][0]["sections"].values()) == negative
    assert el["repaired"] == el["heat"] + el["uniform"] >= 1 and 0.0 <= el["min_t"] < 1.0 and el["max_change"] > 0.0
    assert rep["tables"][0]["repaired"] == negative
