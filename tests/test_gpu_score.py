"""GPU: ndpp_scatt_score (include/ndpp_hip.h) against its restatement score_numpy
bit for bit -- chunk edges, the band skip, the passes over the partial buffer -- and the estimator's
identity: the scored tally over the count is the expectation of the analog tally of
ndpp_scatt_sample on the same events, on synthetic sections, on the golden Legendre table and, through
the command-line tool, on a tabular library the driver writes."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ndpp_amd import lib, reader, sample, score
from ndpp_amd.lib import NDPP_SCORE_CHUNK, SCORE_BADROW, SCORE_OK, SCORE_SKIPPED, SCORE_ZEROROW
from ndpp_amd.score import score_numpy
from test_e2e_reference import CASE
from test_gpu_sample import GOLDEN_ENERGIES, tabular_run  # noqa: F401  (tabular_run: the driver's tabular library)
from test_sample import LEG, TAB, grid, leg_section, tab_section
from test_score import inside, same_bits, score_events, status_case

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "e2e"
pytestmark = pytest.mark.gpu
EVENTS = 200000


def both(normalize, scatt_type, x, y, ein, weight, bins, n_bins):
    """the device and the restatement on the same events: equal in every bit where finite, NaN where
    the restatement is NaN"""
    got = score.score_section((x, y), scatt_type, ein, weight, bins, n_bins, normalize)
    want = score_numpy(normalize, scatt_type, x, y, ein, weight, bins, n_bins)
    for name, a, b in zip(("tally", "wsum", "count", "status"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if a.dtype == np.float64:
            nan = np.isnan(b)
            assert np.isnan(a[nan]).all(), f"{name}: {(~np.isnan(a[nan])).sum()} of {nan.sum()} NaNs are missing"
            diff = np.argwhere((a.view(np.int64) != b.view(np.int64)) & ~nan)
        else:
            diff = np.argwhere(a != b)
        assert not len(diff), (f"{name}: {len(diff)} of {a.size} differ, the first at {tuple(diff[0])}: "
                               f"{a[tuple(diff[0])]!r} against {b[tuple(diff[0])]!r}")
    return got


SECTIONS = [(LEG, 2, 1, 1), (LEG, 5, 3, 11), (LEG, 4, 70, 6), (LEG, 6, 7, 2), (TAB, 4, 3, 128), (TAB, 4, 70, 7)]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("scatt_type,n,G,L", SECTIONS)
def test_gpu_score_equals_the_restatement(hip, scatt_type, n, G, L, normalize):
    x, y = (leg_section if scatt_type == LEG else tab_section)(n, G, L, 800 + L + G)
    n_bins = 5
    ein, weight, bins = score_events(x, 801, n_bins, n_random=3000)             # more than one chunk per bin
    tally, wsum, count, status = both(normalize, scatt_type, x, y, ein, weight, bins, n_bins)
    assert set(np.unique(status)) == {SCORE_OK, SCORE_SKIPPED} and count.sum() == (status == SCORE_OK).sum() > 500
    assert (count > NDPP_SCORE_CHUNK).all() and np.isfinite(tally).all() and tally.any()
    # one event, and none
    k = int(np.flatnonzero(status == SCORE_OK)[-1])
    t, w, c, s = both(normalize, scatt_type, x, y, ein[k:k + 1], weight[k:k + 1], bins[k:k + 1], n_bins)
    assert c.sum() == 1 and s.tolist() == [SCORE_OK]
    t, w, c, s = score.score_section((x, y), scatt_type, ein[:0], weight[:0], bins[:0], n_bins, normalize)
    assert t.shape == (n_bins, G, L) and not t.any() and not w.any() and not c.any() and len(s) == 0
    # events, but none of them scored: the call ends before the sums, with zeroed outputs
    out = ein[status == SCORE_SKIPPED]
    t, w, c, s = both(normalize, scatt_type, x, y, out, np.ones(len(out)), np.full(len(out), -1, dtype=np.int32), n_bins)
    assert len(s) > 10 and (s == SCORE_SKIPPED).all() and not t.any() and not w.any() and not c.any()
    assert lib.scatt_score_info()["scored"] == 0


def test_gpu_score_every_status_equals_the_restatement(hip):
    x, y, ein, weight, bins, want = status_case()
    for normalize in (0, 1):
        tally, wsum, count, status = both(normalize, LEG, x, y, ein, weight, bins, 2)
    assert status.tolist() == want.tolist()
    assert set(status.tolist()) == {SCORE_OK, SCORE_SKIPPED, SCORE_BADROW, SCORE_ZEROROW}
    # rows that are not finite, and a factor that overflows: the whole row is read (inf * 0 is a NaN)
    y2 = y.copy()
    y2[1] *= 1e-320
    y2[1, 0, 2] = np.inf
    y2[1, 1, 1] = 0.0
    ok = want == SCORE_OK
    tally, wsum, count, status = both(1, LEG, x, y2, ein[ok], weight[ok], bins[ok], 2)
    assert np.isnan(tally).any() and not np.isfinite(wsum).any() and count.sum() == ok.sum()


def test_gpu_score_chunk_edges(hip):
    """bins that hold exactly 0, 1, 255, 256, 257 and 513 scored events and one of 3000, with events that
    are not scored in between"""
    x, y = leg_section(5, 3, 11, 810)
    sizes = [0, 1, 255, 256, 257, 513, 3000]
    rng = np.random.default_rng(811)
    bins = np.concatenate([np.full(s, b) for b, s in enumerate(sizes)] + [np.arange(7).repeat(30)]).astype(np.int32)
    weight = rng.uniform(-1.0, 2.0, len(bins))
    weight[sum(sizes):] = np.inf                               # 30 more per bin, none of them scored
    p = rng.permutation(len(bins))
    bins, weight = bins[p], weight[p]
    ein = inside(x, 812, len(bins))
    for normalize in (0, 1):
        tally, wsum, count, status = both(normalize, LEG, x, y, ein, weight, bins, 7)
        assert count.tolist() == sizes and (status == SCORE_SKIPPED).sum() == 210
        assert not tally[0].any() and wsum[0] == 0.0 and tally[1:, 0].all() and not tally[:, 1].any()


def band_section():
    """(6, 70, 4): the groups that scatter are 3 wide and move with the energy; row 2 is all zero, row 1
    has a -0.0 element, row 3 a group with P0 == 0.0 but P1 = 0.3, row 4 a NaN in a group with zero P0"""
    rng = np.random.default_rng(820)
    x, y = grid(6, rng), np.zeros((6, 70, 4))
    for r in range(6):
        y[r, 5 + 10 * r:8 + 10 * r] = rng.uniform(0.1, 1.0, (3, 4))
    y[2] = 0.0
    y[1, 40, 2] = -0.0
    y[3, 60, 1] = 0.3
    y[4, 2, 3] = np.nan
    return x, y


def test_gpu_score_band_skip_changes_no_bit(hip, monkeypatch):
    x, y = band_section()
    assert y[3, 60, 0] == 0.0 and y[4, 2, 0] == 0.0 and not y[2].any() and np.signbit(y[1, 40, 2])
    ein, weight, bins = score_events(x, 821, 3)
    for normalize in (0, 1):
        tally, wsum, count, status = both(normalize, LEG, x, y, ein, weight, bins, 3)
        assert count.min() > 100
        # a P0 > 0 band would drop the group whose P0 is zero, and the NaN
        assert tally[:, 60, 1].all() and not tally[:, 60, 0].any() and np.isnan(tally[:, 2, 3]).all()
        assert not np.signbit(tally[np.isfinite(tally) & (tally == 0.0)]).any()
    at = (ein == x[2]) & (status != SCORE_SKIPPED)              # (normalize = 1) on the zero row itself
    assert at.sum() >= 3 and (status[at] == SCORE_ZEROROW).all()
    # a factor that overflows: at x[0] the masses are subnormal, v = weight / W is infinite, and the groups
    # that are zero in both rows hold inf * 0, a NaN -- nothing may be skipped for such an event
    y[0] *= 1e-320
    y[4, 2, 3] = 0.0
    tally, wsum, count, status = both(1, LEG, x, y, ein, weight, bins, 3)
    assert np.isnan(tally[:, 69, 0]).all() and not np.isfinite(wsum).any()
    # the measurement hook that reads every group gives these bits too
    monkeypatch.setenv("NDPP_SCORE_BAND", "0")
    dense = both(1, LEG, x, y, ein, weight, bins, 3)
    assert all(same_bits(a, b) for a, b in zip(dense, (tally, wsum, count, status)))


def test_gpu_score_passes_change_no_bit(hip, monkeypatch):
    """(4, 70, 6) into 40 bins, about 100 000 events: some 400 chunks of 421 doubles, 1.3 MB of partials,
    so a budget of 1 MB takes two passes or more; the bits are those of one pass"""
    x, y = leg_section(4, 70, 6, 830)
    ein, weight, bins = score_events(x, 831, 40, n_random=100000)
    one = both(1, LEG, x, y, ein, weight, bins, 40)
    info = lib.scatt_score_info()
    assert info["passes"] == 1 and info["chunks"] * (70 * 6 + 1) * 8 > 2 ** 20
    monkeypatch.setenv("NDPP_SCORE_PARTIAL_MB", "1")
    two = score.score_section((x, y), LEG, ein, weight, bins, 40, 1)
    assert lib.scatt_score_info()["passes"] >= 2
    assert all(same_bits(a, b) for a, b in zip(one, two))


def identity(sec, scatt_type, spans, seed, score_fn=None, sample_fn=None, label=""):
    """EVENTS events log-uniform in each incoming bin of `spans`, weight 1, scored with normalize 1 and
    sampled: every element of the analog mean within 5 standard errors of the scored mean.  Legendre:
    5 sqrt(p_g / N), p_g the scored P0 share of the group -- the analog term 1(g) P_l(mu) is bounded by
    the group's indicator, so its variance given the energy is at most p_g.  Bins: 5 binomial standard
    errors of the scored share, sqrt(p (1 - p) / N)."""
    x, y = score._xy(sec)
    G, L = y.shape[1:]
    rng = np.random.default_rng(seed)
    ein = np.concatenate([np.clip(np.exp(rng.uniform(np.log(lo), np.log(hi), EVENTS)), lo, hi) for lo, hi in spans])
    ug, um = rng.random(len(ein)), rng.random(len(ein))
    bins = np.arange(len(spans)).repeat(EVENTS).astype(np.int32)
    tally, wsum, count, status = score.score_section(sec, scatt_type, ein, np.ones(len(ein)), bins, len(spans), 1,
                                                     score_fn)
    g, mu, st = sample.sample_section(sec, scatt_type, ein, ug, um, sample_fn)
    assert (status == SCORE_OK).all() and (st == sample.SAMPLE_OK).all() and count.tolist() == [EVENTS] * len(spans)
    analog, drawn = score.analog_tally(scatt_type, G, L, g, mu, st, bins, len(spans))
    worst = 0.0
    for b in range(len(spans)):
        mean, got = tally[b] / count[b], analog[b] / drawn[b]
        if scatt_type == LEG:
            se = np.sqrt(mean[:, :1] / EVENTS) * np.ones((1, L))
        else:
            se = np.sqrt(mean * (1.0 - mean) / EVENTS)
        assert (got[se == 0.0] == mean[se == 0.0]).all(), (label, b)
        z = np.abs(got - mean)[se > 0.0] / se[se > 0.0]
        worst = max(worst, float(z.max()))
        assert (z <= 5.0).all(), (label, b, float(z.max()))
        mass = mean[:, 0] if scatt_type == LEG else mean.sum(axis=1)
        assert abs(mass.sum() - 1.0) < 1e-12
    print(f"{label}: {len(spans)} incoming bins of {EVENTS} events, the analog tally within {worst:.2f} s.e. of the score")
    return worst


# (scatt_type, L, section seed, event seed).  Both restatements give the device's bits, so the seeds were
# decided on the CPU, with score_numpy and sample_numpy in place of the device, before they were
# committed: the first ones tried, within 5 standard errors there and therefore here.
IDENTITY = [(LEG, 6, 840, 841), (TAB, 7, 842, 843)]
GOLDEN_SEEDS = {6.44e-7: 850, 0.96: 851}


@pytest.mark.parametrize("scatt_type,L,sec_seed,seed", IDENTITY)
def test_gpu_score_is_the_expectation_of_the_analog_tally(hip, scatt_type, L, sec_seed, seed):
    x, y = (leg_section if scatt_type == LEG else tab_section)(5, 3, L, sec_seed)
    spans = [(float(x[0]), float(x[2])), (float(np.sqrt(x[2] * x[3])), float(x[4]))]
    identity((x, y), scatt_type, spans, seed, label="synthetic " + ("moments" if scatt_type == LEG else "bins"))


def golden_spans():
    sec = reader.read_binary((GOLD / f"{CASE['name']}.g2").read_bytes()).elastic
    spans = []
    for e in GOLDEN_SEEDS:
        assert e in GOLDEN_ENERGIES
        i = int(np.searchsorted(sec.ein, e, side="right")) - 1
        spans.append((float(sec.ein[i]), float(sec.ein[i + 1])))
    return sec, spans


def test_gpu_score_golden_legendre_table(hip):
    """two of GOLDEN_ENERGIES' brackets of the golden elastic table, one call each (seeds decided on the
    CPU, as above)"""
    sec, spans = golden_spans()
    for span, seed in zip(spans, GOLDEN_SEEDS.values()):
        identity(sec, LEG, [span], seed, label=f"golden elastic [{span[0]:.4e}, {span[1]:.4e}]")


def test_gpu_score_cli(tabular_run, tmp_path):  # noqa: F811
    out = tmp_path / "score.json"
    r = subprocess.run([sys.executable, "-m", "ndpp_amd.score", str(tabular_run), "--table", CASE["name"], "--edges",
                        "7.9e-8", "1e-6", "0.5", "0.96", "--events", "50000", "--seed", "3", "--json", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    rep = json.loads(out.read_text())
    assert {"table", "section", "scatt_type", "groups", "entries", "events", "seed", "edges", "bins", "flagged",
            "beyond"} <= set(rep)
    assert rep["table"] == CASE["name"] and rep["section"] == "elastic" and rep["scatt_type"] == 1
    assert rep["flagged"] == 0 and rep["beyond"] == 0 and len(rep["bins"]) == 3 and rep["entries"] == 8
    for k, b in enumerate(rep["bins"]):
        assert b["bin"] == k and b["events"] == b["scored"] == b["drawn"] == 50000 and b["status"]["ok"] == 50000
        assert len(b["group_sums"]) == rep["groups"] == 2 and abs(sum(b["group_sums"]) - 1.0) < 1e-12
        assert 0.0 <= b["worst_z"] <= 5.0 and b["beyond"] == 0
        assert np.array(b["score"]).shape == np.array(b["analog"]).shape == (2, 8)
