"""The host half of sampling (ndpp_amd/sample.py, include/ndpp_hip.h: ndpp_scatt_sample), no GPU
needed: the properties of the restatement sample_numpy the device is held to bit for bit
(tests/test_gpu_sample.py), every status once, and the entry point's argument checks, which are
decided before the device is touched.  The sections and events the GPU tests share are built here."""
import numpy as np
import pytest

from conftest import dp, ip
from ndpp_amd import sample
from ndpp_amd.sample import (SAMPLE_BADROW, SAMPLE_NEGDENSITY, SAMPLE_OK, SAMPLE_SKIPPED, SAMPLE_ZEROROW,
                             sample_numpy)
from ndpp_amd.validate import minimum_reference

LEG, TAB = 0, 1
BELOW_ONE = np.nextafter(1.0, 0.0)


def grid(n, rng):
    return np.geomspace(1e-3, 2.0, n) * np.concatenate(([1.0], rng.uniform(0.9, 1.1, n - 2), [1.0]))


def leg_section(n, G, L, seed, zero_group=True):
    """positive rows a_l = a_0 exp(-l (l + 1) tau), tau in [0.15, 1], a_0 >= 0 with one zero group"""
    rng = np.random.default_rng(seed)
    a0, tau = rng.uniform(0.0, 2.0, (n, G)), rng.uniform(0.15, 1.0, (n, G))
    if G >= 3 and zero_group:
        a0[:, 1] = 0.0
    l = np.arange(L)
    shape = lambda t: np.exp(-(l * (l + 1)) * t)
    # the heat kernel is positive, its truncation at L moments need not be: draw tau again until the
    # reference minimum of the row is (a blend of two positive rows is positive)
    for at in np.ndindex(n, G):
        while minimum_reference(shape(tau[at]))[0] <= 0.0:
            tau[at] = rng.uniform(0.15, 1.0)
    return grid(n, rng), a0[:, :, None] * np.exp(-(l * (l + 1))[None, None, :] * tau[:, :, None])


def tab_section(n, G, N, seed, zero_group=True):
    """bins in [0, 1) with leading, trailing and interior zero bins, and an interior zero group"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(0.0, 1.0, (n, G, N))
    if N >= 3:
        y[:, 0, 0] = y[:, 0, N - 1] = 0.0
    if N >= 7:
        y[:, G - 1, 2:4] = 0.0
    if G >= 3 and zero_group:
        y[:, 1, :] = 0.0
    return grid(n, rng), y


def events(x, seed, n_random=1000):
    """every grid point, the largest double below each, energies outside, a NaN, each with u in
    {0, 0.5, the largest double below 1} for both numbers, and n_random random events"""
    rng = np.random.default_rng(seed)
    special = np.concatenate((x, np.nextafter(x, 0.0), [x[0] / 2, x[-1] * 2, np.nan, 0.0, -1.0, np.inf]))
    us = np.array([0.0, 0.5, BELOW_ONE])
    e, ug, um = (v.ravel() for v in np.meshgrid(special, us, us, indexing="ij"))
    er = np.exp(rng.uniform(np.log(x[0]), np.log(x[-1]), n_random))
    return (np.concatenate((e, er)), np.concatenate((ug, rng.random(n_random))),
            np.concatenate((um, rng.random(n_random))))


def blended(x, y, ein):
    """the rows y[i] + (y[i1] - y[i]) f at the energies ein, (n_ev, G, L)"""
    i, f = sample._brackets(x, ein, np.ones(len(ein), dtype=bool))
    i1 = np.minimum(i + 1, len(x) - 1)
    return y[i] + (y[i1] - y[i]) * f[:, None, None]


def test_one_moment_is_the_uniform_cosine():
    x, y = leg_section(4, 3, 1, 2)
    ein, ug, um = events(x, 3)
    g, mu, st = sample_numpy(LEG, x, y, ein, ug, um)
    ok = st == SAMPLE_OK
    assert ok.sum() > 1000 and (np.abs(mu[ok] - (2.0 * um[ok] - 1.0)) <= 2.0 ** -51).all()


def test_one_bin_is_the_uniform_cosine():
    # bins that are powers of two make u T and its quotient by T exact: mu is -1 + 2 u to its last bit
    x = np.array([1.0, 2.0, 4.0])
    y = np.array([4.0, 4.0, 0.25]).reshape(3, 1, 1)
    um = np.concatenate(([0.0, 0.5, BELOW_ONE], np.random.default_rng(4).random(2000)))
    ein = np.where(np.arange(len(um)) % 2 == 0, 1.5, 1.0)
    g, mu, st = sample_numpy(TAB, x, y, ein, np.zeros_like(um), um)
    assert (st == SAMPLE_OK).all() and (g == 0).all()
    assert (np.abs(mu - (-1.0 + 2.0 * um)) <= np.spacing(1.0)).all()
    # any other mass: u T and the quotient round once each, 2 u 2^-52 < 2^-51 in mu
    x, y = tab_section(3, 1, 1, 5)
    ein = np.exp(np.random.default_rng(6).uniform(np.log(x[0]), np.log(x[-1]), len(um)))
    g, mu, st = sample_numpy(TAB, x, y, ein, np.zeros_like(um), um)
    assert (st == SAMPLE_OK).all() and (np.abs(mu - (-1.0 + 2.0 * um)) <= 2.0 ** -51).all()


@pytest.mark.parametrize("n,G,L", [(2, 1, 1), (5, 3, 11), (6, 7, 2), (4, 5, 6)])
def test_cdf_at_the_cosine_is_the_target(n, G, L):
    x, y = leg_section(n, G, L, 10 + L)
    ein, ug, um = events(x, 11)
    g, mu, st = sample_numpy(LEG, x, y, ein, ug, um)
    ok = st == SAMPLE_OK
    assert ok.sum() > 1000 and set(np.unique(st)) == {SAMPLE_OK, SAMPLE_SKIPPED}
    a = blended(x, y, ein[ok])[np.arange(ok.sum()), g[ok]]
    F = sample._legendre_cdf(a, mu[ok])
    err = np.abs(F - um[ok] * a[:, 0]) / a[:, 0]
    print(f"L = {L}: max |F(mu) - target| / a_0 = {err.max():.2e}")
    assert (err <= 1e-14).all()
    assert (np.abs(mu[ok]) <= 1.0).all()


@pytest.mark.parametrize("G,N", [(1, 3), (3, 7), (70, 128), (3, 1)])
def test_zero_bins_and_zero_groups_are_never_chosen(G, N):
    x, y = tab_section(4, G, N, 20 + N)
    ein, ug, um = events(x, 21)
    g, mu, st = sample_numpy(TAB, x, y, ein, ug, um)
    ok = st == SAMPLE_OK
    assert ok.sum() > 1000 and set(np.unique(st)) == {SAMPLE_OK, SAMPLE_SKIPPED}
    assert (np.abs(mu[ok]) <= 1.0).all() and (g[~ok] == -1).all() and (mu[~ok] == 0.0).all()
    rows = blended(x, y, ein[ok])
    assert (rows.sum(axis=2)[np.arange(ok.sum()), g[ok]] > 0.0).all()
    h = 2.0 / N
    k = np.minimum(np.floor((mu[ok] + 1.0) / h).astype(int), N - 1)
    inside = (mu[ok] > -1.0 + h * k) & (mu[ok] < -1.0 + h * (k + 1))          # (an edge belongs to two bins)
    assert inside.sum() > 0.9 * ok.sum()
    assert (rows[np.arange(ok.sum()), g[ok], k][inside] > 0.0).all()
    # the ends of u in particular
    for u in (0.0, BELOW_ONE):
        sel = ok & (ug == u) & (um == u)
        assert sel.sum() >= 2 * len(x) - 1


def test_zero_groups_are_never_chosen_legendre():
    x, y = leg_section(5, 5, 4, 30)
    ein, ug, um = events(x, 31)
    g, mu, st = sample_numpy(LEG, x, y, ein, ug, um)
    ok = st == SAMPLE_OK
    assert (g[ok] != 1).all() and set(np.unique(g[ok])) == {0, 2, 3, 4}
    assert (g[ok & (ug == 0.0)] == 0).all() and (g[ok & (ug == BELOW_ONE)] == 4).all()


@pytest.mark.parametrize("scatt_type,L", [(LEG, 1), (LEG, 6), (LEG, 11), (TAB, 1), (TAB, 7), (TAB, 128)])
def test_cosine_is_monotone_in_u(scatt_type, L):
    x, y = (leg_section if scatt_type == LEG else tab_section)(3, 1, L, 40 + L)
    um = np.sort(np.concatenate(([0.0, BELOW_ONE], np.random.default_rng(41).random(3000))))
    for e in (x[0], np.sqrt(x[0] * x[1]), x[-1]):
        g, mu, st = sample_numpy(scatt_type, x, y, np.full(len(um), e), np.zeros_like(um), um)
        assert (st == SAMPLE_OK).all() and (np.diff(mu) >= 0.0).all()
        end = 1.0 - 2.0 / L if scatt_type == TAB and L >= 3 else 1.0     # (tab_section: the end bins are zero)
        assert abs(mu[0] + end) < 1e-3 and abs(mu[-1] - end) < 1e-3


def interior_negative_row():
    """1/2 (1 + 2.6 P_2): negative for |mu| < 0.277"""
    return np.array([1.0, 2.0]), np.array([1.0, 0.0, 0.52] * 2).reshape(2, 1, 3)


def overflowing_negative_row():
    """3/2 a_1 and 5/2 a_2 overflow with opposite signs.  F = 5e307 (mu^2 - 1) (1.5 - 2.5 mu) + (mu + 1) / 2
    stays finite and crosses every target upwards at mu = 0.6 to rounding, where the density
    evaluates to inf - inf, a NaN"""
    return np.array([1.0, 2.0]), np.array([1.0, 1e308, -1e308] * 2).reshape(2, 1, 3)


def test_negative_rows():
    """The bisection keeps F(lo) < target <= F(hi), so it ends where F crosses the target upwards,
    and there the density is not negative: no event lands in a dip of a negative row, and none is
    flagged (NEGDENSITY is no positivity check, validate --certified is).  What
    is left for the status is a density that does not evaluate: here one that overflows."""
    x, y = interior_negative_row()
    um = np.random.default_rng(51).random(5000)
    g, mu, st = sample_numpy(LEG, x, y, np.full(len(um), 1.5), np.zeros_like(um), um)
    assert (st == SAMPLE_OK).all() and (np.abs(mu) > 0.27).all()
    x, y = overflowing_negative_row()
    g, mu, st = sample_numpy(LEG, x, y, np.full(len(um), 1.5), np.zeros_like(um), um)
    assert (g == 0).all() and (st == SAMPLE_NEGDENSITY).all() and (np.abs(mu - 0.6) < 1e-12).all()


def test_every_status_once():
    x = np.array([1.0, 2.0, 4.0, 8.0])
    y = np.ones((4, 2, 3))
    y[2:] = 0.0                                   # zero rows at 4 and 8
    y[0, 1, 1] = -3.0                             # a negative bin at 1
    ein = np.array([3.0, 0.5, 3.0, 3.0, 3.0, np.nan, 5.0, 1.0, 1.0])
    ug = np.array([0.2, 0.2, 1.0, 0.2, -0.1, 0.2, 0.2, 0.9, 0.2])
    um = np.array([0.2, 0.2, 0.2, np.nan, 0.2, 0.2, 0.2, 0.2, 0.2])
    g, mu, st = sample_numpy(TAB, x, y, ein, ug, um)
    S, B, Z = SAMPLE_SKIPPED, SAMPLE_BADROW, SAMPLE_ZEROROW
    assert st.tolist() == [SAMPLE_OK, S, S, S, S, S, Z, B, B]
    assert g.tolist() == [0] + [-1] * 8 and (mu[1:] == 0.0).all() and -1.0 < mu[0] < 1.0
    # Legendre: a non-finite moment, a negative mass
    yl = np.ones((4, 2, 3)) * np.array([1.0, 0.3, 0.1])
    yl[0, 0, 2] = np.inf
    yl[3, 1, 0] = -1.0
    g, mu, st = sample_numpy(LEG, x, yl, np.array([1.0, 1.0, 8.0, 3.0]), np.array([0.1, 0.9, 0.5, 0.5]), np.full(4, 0.3))
    assert st.tolist() == [B, SAMPLE_OK, B, SAMPLE_OK] and g.tolist() == [-1, 1, -1, 1]
    x2, y2 = overflowing_negative_row()
    g, mu, st = sample_numpy(LEG, x2, y2, [1.0], [0.0], [0.001])
    assert st.tolist() == [SAMPLE_NEGDENSITY] and g.tolist() == [0] and abs(mu[0] - 0.6) < 1e-12


def test_expectations_are_the_blended_row():
    x, y = tab_section(4, 3, 7, 60)
    e = float(np.sqrt(x[1] * x[2]))
    p, shape = sample.expectations((x, y), TAB, e)
    row = blended(x, y, np.array([e]))[0]
    assert np.allclose(p, row.sum(axis=1) / row.sum(), rtol=1e-14, atol=0) and p[1] == 0.0
    assert np.isnan(shape[1]).all() and np.allclose(shape[[0, 2]].sum(axis=1), 1.0, rtol=1e-14)
    x, y = leg_section(4, 3, 6, 61)
    p, shape = sample.expectations((x, y), LEG, e)
    assert (shape[[0, 2], 0] == 1.0).all() and abs(p.sum() - 1.0) < 1e-14
    with pytest.raises(ValueError):
        sample.expectations((x, y), LEG, x[-1] * 2)


def _call(hip):
    x, y = leg_section(3, 2, 4, 70)
    ein, ug, um = np.array([x[0], x[1]]), np.array([0.1, 0.2]), np.array([0.3, 0.4])
    g, mu, st = np.zeros(2, np.int32), np.zeros(2), np.zeros(2, np.int32)
    hold = (x, y, ein, ug, um, g, mu, st)
    return hold, [LEG, 2, 4, 3, dp(x), dp(y), 2, dp(ein), dp(ug), dp(um), ip(g), dp(mu), ip(st)]


def test_entry_refuses_before_the_device(hip):
    lib = hip.load()
    hold, args = _call(hip)

    def call(at, value):
        a = list(args)
        a[at] = value
        return lib.ndpp_scatt_sample(*a)

    for at in (4, 5, 7, 8, 9, 10, 11, 12):                  # every pointer
        assert call(at, None) == -22 and b"NULL" in lib.ndpp_last_error()
    for at, bad in ((0, 2), (0, -1), (1, 0), (2, 0), (2, 12), (3, 1), (6, -1), (1, 2 ** 31 - 1)):
        assert call(at, bad) == -22, (at, bad)
    a = list(args)
    a[0], a[2] = TAB, 129                                    # one bin too many; 128 passes the check
    assert lib.ndpp_scatt_sample(*a) == -22
    for k, v in ((1, hold[0][0]), (0, -1.0), (2, np.nan), (2, np.inf)):   # not increasing, not positive, not finite
        x = hold[0].copy()
        x[k] = v
        assert call(4, dp(x)) == -22 and b"strictly increasing" in lib.ndpp_last_error()
    if lib.ndpp_device_count() == 0:
        assert lib.ndpp_scatt_sample(*args) == -5 and b"no HIP device" in lib.ndpp_last_error()
        assert call(6, 0) == -5
        with pytest.raises(hip.NdppError):
            hip.scatt_sample(LEG, *hold[:5])
    del hold


def test_brackets_entry_is_the_restatements_bracket(hip):
    """ndpp_sample_brackets, the host half of the entry point, needs no device: rows and weights equal
    sample_numpy's in every bit, skipped events carry row -1, and bad arguments are refused"""
    x, _ = leg_section(6, 1, 1, 80)
    ein, ug, um = events(x, 81)
    row, wt = hip.sample_brackets(x, ein, ug, um)
    with np.errstate(invalid="ignore"):
        ok = (np.isfinite(ein) & (ein > 0.0) & (ein >= x[0]) & (ein <= x[-1]) & (ug >= 0.0) & (ug < 1.0)
              & (um >= 0.0) & (um < 1.0))
    i, f = sample._brackets(x, ein, ok)
    assert ok.sum() > 1000 and (~ok).sum() > 10
    assert np.array_equal(row, np.where(ok, i, -1)) and np.array_equal(wt, np.where(ok, f, 0.0))
    assert (wt >= 0.0).all() and (wt <= 1.0).all() and (wt[np.isin(ein, x)] == 0.0).all()
    lib = hip.load()
    r, w = np.zeros(2, np.int32), np.zeros(2)
    args = [6, dp(x), 2, dp(ein), dp(ug), dp(um), ip(r), dp(w)]
    for at, bad in ((0, 1), (2, -1), (1, None), (3, None), (4, None), (5, None), (6, None), (7, None),
                    (1, dp(x[::-1].copy()))):
        a = list(args)
        a[at] = bad
        assert lib.ndpp_sample_brackets(*a) == -22, at


def test_cli_input_errors(tmp_path, capsys):
    from pathlib import Path
    gold = Path(__file__).resolve().parent / "golden" / "e2e"
    assert sample.main([str(tmp_path / "none"), "--table", "x", "--energy", "1"]) == 2
    assert sample.main([str(gold), "--table", "nope", "--energy", "1"]) == 2
    assert "92238.71c" in capsys.readouterr().err
    for bad in (["--energy", "-1"], ["--energy", "abc"], ["--energy", "1", "--events", "0"]):
        assert sample.main([str(gold), "--table", "92238.71c", *bad]) == 2
