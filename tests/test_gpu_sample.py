"""GPU: ndpp_scatt_sample (include/ndpp_hip.h) against its restatement
sample_numpy bit for bit, the consumer's identity -- the moments (or bins) of what is drawn are the
ones in the file -- on synthetic sections, on the golden Legendre table and on a tabular library the
driver writes, and the command-line tool on that library."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from numpy.polynomial import legendre

import ace_synth
from ndpp_amd import reader, sample
from ndpp_amd.sample import SAMPLE_BADROW, SAMPLE_NEGDENSITY, SAMPLE_OK, SAMPLE_SKIPPED, sample_numpy
from ndpp_amd.validate import minimum_reference
from test_e2e_reference import CASE, e2e_nuclide
from test_sample import (LEG, TAB, events, interior_negative_row, leg_section, overflowing_negative_row,
                         tab_section)

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "e2e"
pytestmark = pytest.mark.gpu
EVENTS = 200000
# elastic energies of the golden table strictly between two of its grid points, both of whose rows
# are positive in every group that scatters (minimum_reference, chosen on the CPU)
GOLDEN_ENERGIES = [2.5e-9, 7.9e-8, 6.44e-7, 2.6e-4, 6.5e-3, 0.96, 6.5]


def both(scatt_type, x, y, ein, ug, um):
    """the device and the restatement on the same events: equal in every bit"""
    got = sample.sample_section((x, y), scatt_type, ein, ug, um)
    want = sample_numpy(scatt_type, x, y, ein, ug, um)
    for name, a, b in zip(("group", "mu", "status"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        diff = np.flatnonzero(a != b)
        assert not len(diff), (f"{name}: {len(diff)} of {len(a)} events differ, the first at {diff[0]}: "
                               f"{a[diff[0]]!r} against {b[diff[0]]!r} (E {ein[diff[0]]!r}, u {ug[diff[0]]!r}, {um[diff[0]]!r})")
    return got


def one_and_none(scatt_type, x, y, ein, ug, um):
    both(scatt_type, x, y, ein[-1:], ug[-1:], um[-1:])
    g, mu, st = sample.sample_section((x, y), scatt_type, ein[:0], ug[:0], um[:0])
    assert len(g) == len(mu) == len(st) == 0


@pytest.mark.parametrize("n,G,L", [(2, 1, 1), (5, 3, 11), (4, 70, 6), (6, 7, 2)])
def test_gpu_sample_legendre_equals_the_restatement(hip, n, G, L):
    x, y = leg_section(n, G, L, 100 + L)
    for row in y.reshape(-1, L):
        assert row[0] == 0.0 or minimum_reference(row)[0] > 0.0
    ein, ug, um = events(x, 101)
    g, mu, st = both(LEG, x, y, ein, ug, um)
    assert set(np.unique(st)) == {SAMPLE_OK, SAMPLE_SKIPPED} and (st == SAMPLE_OK).sum() > 1000
    assert (g[st == SAMPLE_SKIPPED] == -1).all() and (G < 3 or (g != 1).all())
    one_and_none(LEG, x, y, ein, ug, um)


@pytest.mark.parametrize("G", [1, 3, 70])
@pytest.mark.parametrize("N", [1, 3, 7, 128])
def test_gpu_sample_tabular_equals_the_restatement(hip, N, G):
    x, y = tab_section(4, G, N, 200 + N + G)
    ein, ug, um = events(x, 201)
    g, mu, st = both(TAB, x, y, ein, ug, um)
    assert set(np.unique(st)) == {SAMPLE_OK, SAMPLE_SKIPPED} and (st == SAMPLE_OK).sum() > 1000
    assert (np.abs(mu) <= 1.0).all() and (G < 3 or (g != 1).all())
    one_and_none(TAB, x, y, ein, ug, um)


def test_gpu_sample_bad_zero_and_negative_rows_equal_the_restatement(hip):
    """every status on the device as in the restatement.  A row that is negative inside (-1, 1) is
    sampled without a flag: the bisection ends where F crosses the target upwards, where the density
    is not negative, so no event lands in the dip (tests/test_sample.py: test_negative_rows); the row
    whose density evaluates to inf - inf at the cosine drawn is the one that is flagged."""
    x, y = tab_section(5, 3, 7, 300, zero_group=False)
    y[3:] = 0.0
    y[0, 2, 4] = -1.0
    y[1, 0, 1] = np.nan
    ein, ug, um = events(x, 301)
    g, mu, st = both(TAB, x, y, ein, ug, um)
    assert set(np.unique(st)) == {0, 1, 2, 3}
    x, y = leg_section(5, 3, 4, 302, zero_group=False)
    y[3:] = 0.0
    y[0, 2, 0] = -1.0
    y[1, 0, 3] = np.inf
    g, mu, st = both(LEG, x, y, *events(x, 303))
    assert set(np.unique(st)) == {0, 1, 2, 3}
    um = np.random.default_rng(304).random(3000)
    x, y = interior_negative_row()
    g, mu, st = both(LEG, x, y, np.full(len(um), 1.5), np.zeros_like(um), um)
    assert (st == SAMPLE_OK).all() and (np.abs(mu) > 0.27).all()
    x, y = overflowing_negative_row()
    x, y = np.array([1.0, 2.0, 4.0]), np.concatenate((y, interior_negative_row()[1][:1]))
    ein = np.where(np.arange(len(um)) % 2 == 0, 1.0, 4.0)       # the row that overflows, the row with the dip
    g, mu, st = both(LEG, x, y, ein, np.zeros_like(um), um)
    assert (st[ein == 1.0] == SAMPLE_NEGDENSITY).all() and (st[ein == 4.0] == SAMPLE_OK).all() and (g == 0).all()


def check_drawn(section, scatt_type, e, g, mu, st, label):
    """the identity: per group the fraction drawn against w_g / W, and the means of P_l(mu) against
    a_l / a_0 (within 5 / sqrt(n_g): |P_l| <= 1) or the bin fractions against t_k / T, within 5
    binomial standard errors"""
    p, shape = sample.expectations(section, scatt_type, e)
    G, L = shape.shape
    n = len(g)
    worst_g = worst_s = 0.0
    for k in range(G):
        sel = g == k
        ng = int(sel.sum())
        se = np.sqrt(p[k] * (1.0 - p[k]) / n)
        if se == 0.0:
            assert ng == round(p[k] * n), (label, k)
            z = 0.0
        else:
            z = abs(ng / n - p[k]) / se
        worst_g = max(worst_g, z)
        assert z <= 5.0, (label, k, ng / n, p[k])
        if not ng:
            continue
        if scatt_type == LEG:
            for l in range(1, L):
                got = legendre.legval(mu[sel], np.eye(L)[l]).mean()
                zl = abs(got - shape[k, l]) * np.sqrt(ng)
                worst_s = max(worst_s, zl)
                assert zl <= 5.0, (label, k, l, got, shape[k, l])
        else:
            idx = np.minimum(np.floor((mu[sel] + 1.0) * (0.5 * L)).astype(int), L - 1)
            frac = np.bincount(idx, minlength=L) / ng
            se_k = np.sqrt(shape[k] * (1.0 - shape[k]) / ng)
            assert (frac[se_k == 0.0] == shape[k][se_k == 0.0]).all(), (label, k)
            zk = (np.abs(frac - shape[k])[se_k > 0.0] / se_k[se_k > 0.0]).max(initial=0.0)
            worst_s = max(worst_s, zk)
            assert zk <= 5.0, (label, k, frac, shape[k])
    print(f"{label} E = {e:.4e}: {n} events, group fractions within {worst_g:.2f} s.e., "
          f"{'moments' if scatt_type == LEG else 'bins'} within {worst_s:.2f}")


def draw(section, scatt_type, e, seed, events=EVENTS):
    rng = np.random.default_rng(seed)
    ug, um = rng.random(events), rng.random(events)
    return sample.sample_section(section, scatt_type, np.full(events, e), ug, um)


@pytest.mark.parametrize("scatt_type,L,seed", [(LEG, 6, 11), (TAB, 7, 12)])
def test_gpu_what_is_drawn_is_what_is_stored(hip, scatt_type, L, seed):
    x, y = (leg_section if scatt_type == LEG else tab_section)(4, 3, L, 400 + L, zero_group=False)
    e = float(np.sqrt(x[1] * x[2]) * 1.01)
    assert x[1] < e < x[2]
    g, mu, st = draw((x, y), scatt_type, e, seed)
    assert (st == SAMPLE_OK).all() and set(np.unique(g)) == {0, 1, 2}
    check_drawn((x, y), scatt_type, e, g, mu, st, "synthetic")


def test_gpu_sample_golden_legendre_table(hip):
    t = reader.read_binary((GOLD / f"{CASE['name']}.g2").read_bytes())
    sec = t.elastic
    assert t.scatt_type == LEG and len(GOLDEN_ENERGIES) >= 5
    for k, e in enumerate(GOLDEN_ENERGIES):
        i = int(np.searchsorted(sec.ein, e, side="right")) - 1
        assert sec.ein[i] < e < sec.ein[i + 1]
        for row in sec.mat[i:i + 2].reshape(-1, sec.mat.shape[2]):
            assert row[0] == 0.0 or (row[0] > 0.0 and minimum_reference(row)[0] > 0.0)
        g, mu, st = draw(sec, LEG, e, 500 + k)
        assert (st == SAMPLE_OK).all()
        check_drawn(sec, LEG, e, g, mu, st, "golden elastic")


@pytest.fixture(scope="module")
def tabular_run(tmp_path_factory):
    """a tabular library written by the driver, set up as in test_gpu_run: test_gpu_tabular_run_validates"""
    from test_gpu_run import drive, set_tag
    run = tmp_path_factory.mktemp("sample") / "run"
    ace_synth.write_inputs(run, CASE["name"], e2e_nuclide(), scatt_order=CASE["scatt_order"], mu_bins=CASE["mu_bins"],
                           extend_pts=CASE["extend_pts"], inel_extend_pts=CASE["inel_extend_pts"], threads=1)
    set_tag(run, "scatt_type", "tabular")
    set_tag(run, "scatt_order", "8")
    assert drive(run) == 0
    return run


def test_gpu_sample_tabular_library_of_the_driver(hip, tabular_run):
    t = reader.read_binary((tabular_run / f"{CASE['name']}.g2").read_bytes())
    assert t.scatt_type == TAB and t.elastic.mat.shape[2] == 8
    for k, e in enumerate(GOLDEN_ENERGIES):
        g, mu, st = draw(t.elastic, TAB, e, 600 + k)
        assert not (st == SAMPLE_BADROW).any() and (st == SAMPLE_OK).all()
        check_drawn(t.elastic, TAB, e, g, mu, st, "tabular elastic")


def test_gpu_sample_cli(tabular_run, tmp_path):
    out = tmp_path / "sample.json"
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.sample", str(tabular_run), "--table", CASE["name"], "--energy",
                        "7.9e-8", "0.96", "--events", "50000", "--seed", "3", "--json", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    rep = json.loads(out.read_text())
    assert {"table", "section", "scatt_type", "groups", "entries", "events", "seed", "energies", "flagged"} <= set(rep)
    assert rep["table"] == CASE["name"] and rep["section"] == "elastic" and rep["scatt_type"] == 1
    assert rep["flagged"] == 0 and [e["energy"] for e in rep["energies"]] == [7.9e-8, 0.96]
    for e in rep["energies"]:
        assert {"energy", "events", "drawn", "status", "groups"} <= set(e) and e["drawn"] == 50000
        assert e["status"]["ok"] == 50000 and len(e["groups"]) == rep["groups"] == 2
        for grp in e["groups"]:
            assert {"group", "expected", "sampled", "n", "z_group"} <= set(grp) and abs(grp["z_group"]) <= 5.0
            if grp["n"]:
                assert len(grp["z_shape"]) == len(grp["expected_shape"]) == len(grp["sampled_shape"]) == 8
                assert max(abs(z) for z in grp["z_shape"]) <= 5.0
