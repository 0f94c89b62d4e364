"""The host half of scoring (ndpp_amd/score.py, include/ndpp_hip.h: ndpp_scatt_score), no GPU needed:
the restatement score_numpy the device is held to bit for bit (tests/test_gpu_score.py) against a
long-double sum of the same contributions, the properties of its sum order, the normalised sums,
every status once, and the entry point's argument checks, which are decided before the device is
touched.  The events the GPU tests share are built here; the sections come from tests/test_sample.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import dp, ip
from ndpp_amd import score
from ndpp_amd.lib import NDPP_SCORE_CHUNK, SCORE_BADROW, SCORE_OK, SCORE_SKIPPED, SCORE_ZEROROW
from ndpp_amd.score import contributions, score_numpy
from test_sample import LEG, TAB, events, leg_section, tab_section

U = 2.0 ** -53


def score_events(x, seed, n_bins, n_random=1000):
    """the energies of test_sample.events (every grid point, the double below each, energies outside, a
    NaN), weights random in [-1, 2] with a zero and an infinite one, bins random in [-1, n_bins]"""
    ein = events(x, seed, n_random)[0]
    rng = np.random.default_rng(seed + 1000)
    weight = rng.uniform(-1.0, 2.0, len(ein))
    weight[-3], weight[-7] = 0.0, np.inf
    return ein, weight, rng.integers(-1, n_bins + 1, len(ein)).astype(np.int32)


def inside(x, seed, n_ev):
    return np.exp(np.random.default_rng(seed).uniform(np.log(x[0]), np.log(x[-1]), n_ev))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sum_bound(n_events_in_bin, abs_sum):
    """(NDPP_SCORE_CHUNK + n_chunks + 4) 2^-53 sum |c|: the first-order bound of a sequential
    sum of 256 terms, then of n_chunks partials, plus the three roundings of a term"""
    n_chunks = -(-n_events_in_bin // NDPP_SCORE_CHUNK)
    return (NDPP_SCORE_CHUNK + n_chunks + 4) * U * abs_sum


@pytest.mark.parametrize("n_bins", [1, 40])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n,G,L", [(5, 3, 11), (4, 70, 6)])
def test_restatement_against_a_long_double_sum(n, G, L, normalize, n_bins):
    x, y = leg_section(n, G, L, 700 + L)
    rng = np.random.default_rng(701)
    ein, weight, bins = inside(x, 702, 3000), rng.uniform(-1.0, 2.0, 3000), rng.integers(0, n_bins, 3000)
    tally, wsum, count, status = score_numpy(normalize, LEG, x, y, ein, weight, bins, n_bins)
    ev, c, v, st = contributions(normalize, LEG, x, y, ein, weight, bins, n_bins)
    assert (status == SCORE_OK).all() and len(ev) == 3000 and np.array_equal(st, status) and count.sum() == 3000
    worst = 0.0
    for b in range(n_bins):
        cb, vb = c[bins[ev] == b].astype(np.longdouble), v[bins[ev] == b].astype(np.longdouble)
        assert count[b] == len(cb)
        err = np.abs(tally[b].astype(np.longdouble) - cb.sum(axis=0))
        bound = sum_bound(len(cb), np.abs(cb).sum(axis=0))
        assert (err <= bound).all(), (b, float((err / bound)[bound > 0].max()))
        assert abs(np.longdouble(wsum[b]) - vb.sum()) <= sum_bound(len(vb), np.abs(vb).sum())
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    print(f"({n}, {G}, {L}) normalize {normalize}, {n_bins} bins: the worst error is {worst:.3f} of its bound")


def order_case():
    x, y = leg_section(5, 3, 11, 710)
    rng = np.random.default_rng(711)
    n_ev = 3000
    return x, y, inside(x, 712, n_ev), rng.uniform(-1.0, 2.0, n_ev), rng.integers(0, 4, n_ev).astype(np.int32)


def test_moving_events_across_bins_changes_no_bit():
    x, y, ein, weight, bins = order_case()
    want = score_numpy(1, LEG, x, y, ein, weight, bins, 4)
    # fresh random places for the events, handed out in ascending order inside every bin: the bins are
    # interleaved differently, each keeps its own order
    key = np.random.default_rng(713).random(len(ein))
    for b in range(4):
        key[bins == b] = np.sort(key[bins == b])
    for p in (np.argsort(key), np.argsort(bins, kind="stable")):
        assert not np.array_equal(p, np.arange(len(p)))
        got = score_numpy(1, LEG, x, y, ein[p], weight[p], bins[p], 4)
        assert all(same_bits(a, b) for a, b in zip(got[:3], want[:3]))


def test_reversing_one_bin_changes_a_bit():
    x, y, ein, weight, bins = order_case()
    want = score_numpy(1, LEG, x, y, ein, weight, bins, 4)
    at = np.flatnonzero(bins == 2)
    assert len(at) > 2 * NDPP_SCORE_CHUNK
    p = np.arange(len(ein))
    p[at] = at[::-1]
    got = score_numpy(1, LEG, x, y, ein[p], weight[p], bins[p], 4)
    assert np.array_equal(got[2], want[2])
    assert not same_bits(got[0][2], want[0][2]) and np.allclose(got[0], want[0], rtol=1e-12, atol=1e-15)
    for b in (0, 1, 3):
        assert same_bits(got[0][b], want[0][b]) and got[1][b] == want[1][b]


@pytest.mark.parametrize("scatt_type,G,L", [(LEG, 3, 11), (LEG, 70, 6), (TAB, 3, 7), (TAB, 70, 7)])
def test_normalised_rows_sum_to_the_count(scatt_type, G, L):
    """With weight 1 and normalize 1 every event adds a row whose masses sum to 1, so the sum over the
    groups (and bins) of a tally is its count, within the bound of the sums.  (The identity itself
    carries roundings that bound does not name -- W is a sum of G terms, a tabular mass one of L, a
    blend three and 1 / W one, to first order (G + L + 6) 2^-53 more -- but they are not needed: the
    errors measured are below one hundredth of the bound.)"""
    x, y = (leg_section if scatt_type == LEG else tab_section)(4, G, L, 720 + L)
    n_ev, n_bins = 3000, 5
    ein, bins = inside(x, 721, n_ev), np.random.default_rng(722).integers(0, n_bins, n_ev)
    tally, wsum, count, status = score_numpy(1, scatt_type, x, y, ein, np.ones(n_ev), bins, n_bins)
    ev, c, v, _ = contributions(1, scatt_type, x, y, ein, np.ones(n_ev), bins, n_bins)
    assert (status == SCORE_OK).all() and (y >= 0.0).all()
    for b in range(n_bins):
        mass = tally[b][:, 0] if scatt_type == LEG else tally[b]
        cb = c[bins[ev] == b][:, :, 0] if scatt_type == LEG else c[bins[ev] == b]
        total = mass.astype(np.longdouble).sum()
        bound = sum_bound(int(count[b]), np.abs(cb.astype(np.longdouble)).sum())
        print(f"bin {b}: {count[b]} events, sum {float(total)!r}, off by {float(abs(total - count[b])):.2e}, bound {float(bound):.2e}")
        assert abs(total - np.longdouble(count[b])) <= bound
        vb = v[bins[ev] == b].astype(np.longdouble)
        assert abs(np.longdouble(wsum[b]) - vb.sum()) <= sum_bound(len(vb), np.abs(vb).sum())


def status_case():
    x = np.array([1.0, 2.0, 4.0, 8.0])
    y = np.ones((4, 2, 3)) * np.array([1.0, 0.3, 0.1])
    y[2:] = 0.0                                   # zero rows at 4 and 8
    y[0, 1, 0] = -3.0                             # a negative mass at 1
    # 600 good events between 2 and 4 (two chunks per bin), the flagged ones in between
    flagged = [(0.5, 1.0, 0, SCORE_SKIPPED), (16.0, 1.0, 0, SCORE_SKIPPED), (np.nan, 1.0, 1, SCORE_SKIPPED),
               (3.0, np.inf, 1, SCORE_SKIPPED), (3.0, np.nan, 1, SCORE_SKIPPED), (3.0, 1.0, -1, SCORE_SKIPPED),
               (3.0, 1.0, 2, SCORE_SKIPPED), (0.0, 1.0, 0, SCORE_SKIPPED), (-3.0, 1.0, 0, SCORE_SKIPPED),
               (1.0, 1.0, 0, SCORE_BADROW), (1.5, 1.0, 1, SCORE_BADROW), (5.0, 1.0, 1, SCORE_ZEROROW),
               (8.0, 1.0, 0, SCORE_ZEROROW), (4.0, 1.0, 0, SCORE_ZEROROW)]
    rng = np.random.default_rng(730)
    good = [(float(e), float(w), int(b), SCORE_OK)
            for e, w, b in zip(rng.uniform(2.0, 3.9, 600), rng.uniform(-1.0, 2.0, 600), rng.integers(0, 2, 600))]
    good[5] = (3.0, 0.0, 0, SCORE_OK)             # weights of zero and below are scored
    good[6] = (3.0, -2.0, 1, SCORE_OK)
    rows = list(good)
    for k, f in enumerate(flagged):
        rows.insert(7 + 41 * k, f)
    cols = list(zip(*rows))
    return x, y, np.array(cols[0]), np.array(cols[1]), np.array(cols[2], dtype=np.int32), np.array(cols[3], dtype=np.int32)


def test_every_status_once():
    x, y, ein, weight, bins, want = status_case()
    tally, wsum, count, status = score_numpy(1, LEG, x, y, ein, weight, bins, 2)
    assert status.tolist() == want.tolist()
    assert {SCORE_OK, SCORE_SKIPPED, SCORE_BADROW, SCORE_ZEROROW} == set(status.tolist())
    # the flagged events leave everything untouched: the call without them gives the same bits
    ok = want == SCORE_OK
    clean = score_numpy(1, LEG, x, y, ein[ok], weight[ok], bins[ok], 2)
    assert (clean[3] == SCORE_OK).all() and count.sum() == ok.sum() == 600
    assert same_bits(tally, clean[0]) and same_bits(wsum, clean[1]) and same_bits(count, clean[2])
    # without normalisation no row is looked at: bad and zero rows are scored
    t0, w0, c0, s0 = score_numpy(0, LEG, x, y, ein, weight, bins, 2)
    assert ((s0 == SCORE_SKIPPED) == (want == SCORE_SKIPPED)).all() and set(s0.tolist()) == {SCORE_OK, SCORE_SKIPPED}
    assert c0.sum() == (want != SCORE_SKIPPED).sum()
    # a mass that is not finite, and a bin without events
    y2 = y.copy()
    y2[1, 0, 0] = np.inf
    t, w, c, s = score_numpy(1, LEG, x, y2, [3.0, 3.0], [1.0, 1.0], [0, 0], 3)
    assert s.tolist() == [SCORE_BADROW] * 2 and not t.any() and not w.any() and not c.any()
    # tabular: the mass is the sum of the bins
    t, w, c, s = score_numpy(1, TAB, x, np.abs(y), [1.0, 5.0], [1.0, 1.0], [0, 0], 1)
    assert s.tolist() == [SCORE_OK, SCORE_ZEROROW] and c.tolist() == [1]


def test_restatement_refuses_bad_arguments():
    x, y = leg_section(3, 2, 4, 740)
    ev = ([x[0]], [1.0], [0])
    for bad in (dict(normalize=2), dict(scatt_type=2), dict(n_bins=0), dict(x=x[::-1]), dict(y=np.ones((3, 2, 12)))):
        a = dict(normalize=1, scatt_type=LEG, x=x, y=y, n_bins=1)
        a.update(bad)
        with pytest.raises(ValueError):
            score_numpy(a["normalize"], a["scatt_type"], a["x"], a["y"], *ev, a["n_bins"])
    # without normalisation the scattering type is not read and a row may be as long as a tabular one
    t, w, c, s = score_numpy(0, 7, x, np.ones((3, 2, 128)), *ev, 1)
    assert s.tolist() == [SCORE_OK] and (t == 1.0).all()


def lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_long))


def _call():
    x, y = leg_section(3, 2, 4, 750)
    ein, weight, bins = np.array([x[0], x[1]]), np.array([0.5, 2.0]), np.array([0, 1], dtype=np.int32)
    tally, wsum, count, status = np.zeros((2, 2, 4)), np.zeros(2), np.zeros(2, dtype=np.int64), np.zeros(2, np.int32)
    hold = (x, y, ein, weight, bins, tally, wsum, count, status)
    return hold, [1, LEG, 2, 4, 3, dp(x), dp(y), 2, dp(ein), dp(weight), ip(bins), 2, dp(tally), dp(wsum), lp(count),
                  ip(status)]


def test_entry_refuses_before_the_device(hip):
    lib = hip.load()
    hold, args = _call()

    def call(at, value, **more):
        a = list(args)
        a[at] = value
        for k, v in more.items():
            a[int(k[1:])] = v
        return lib.ndpp_scatt_score(*a)

    for at in (5, 6, 8, 9, 10, 12, 13, 14, 15):              # every pointer
        assert call(at, None) == -22 and b"NULL" in lib.ndpp_last_error()
    for at, bad in ((0, 2), (0, -1), (1, 2), (1, -1), (2, 0), (3, 0), (3, 12), (4, 1), (7, -1), (11, 0), (11, -3),
                    (2, 2 ** 31 - 1)):
        assert call(at, bad) == -22, (at, bad)
    assert call(3, 129, _1=TAB) == -22 and call(3, 129, _0=0) == -22      # one bin too many, whatever the mode
    for k, v in ((1, hold[0][0]), (0, -1.0), (2, np.nan), (2, np.inf)):   # not increasing, not positive, not finite
        x = hold[0].copy()
        x[k] = v
        assert call(5, dp(x)) == -22 and b"strictly increasing" in lib.ndpp_last_error()
    if lib.ndpp_device_count() == 0:
        assert lib.ndpp_scatt_score(*args) == -5 and b"no HIP device" in lib.ndpp_last_error()
        assert call(7, 0) == -5
        assert call(0, 0, _1=7) == -5                        # normalize = 0 does not read the scattering type
        with pytest.raises(hip.NdppError):
            hip.scatt_score(1, LEG, *hold[:5], 2)
    del hold


def test_cli_input_errors(tmp_path, capsys):
    from pathlib import Path
    gold = Path(__file__).resolve().parent / "golden" / "e2e"
    assert score.main([str(tmp_path / "none"), "--table", "x", "--edges", "1", "2"]) == 2
    assert score.main([str(gold), "--table", "nope", "--edges", "1", "2"]) == 2
    assert "92238.71c" in capsys.readouterr().err
    for bad in (["--edges", "1"], ["--edges", "2", "1"], ["--edges", "-1", "1"], ["--edges", "1", "abc"],
                ["--edges", "1", "1"], ["--edges", "1", "2", "--events", "0"], ["--edges", "1", "2", "--seed", "-1"]):
        assert score.main([str(gold), "--table", "92238.71c", *bad]) == 2
