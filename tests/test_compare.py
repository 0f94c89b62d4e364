"""CPU: the library comparison without a device -- the argument checks of ndpp_lib_compare (decided
before the device is touched), the host restatement compare_numpy on hand-made sections, where the
supremum of the error lies (the union points and the limits from below them), and the input half of
compare_dirs on the golden end-to-end directories."""
import shutil
import struct
from pathlib import Path

import numpy as np
import pytest

from conftest import dp, ip

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "e2e"
INF = float("inf")
EPS = np.finfo(np.float64).eps


def cp():
    from ndpp_amd import compare
    return compare


# ---- argument checks of the entry point (before the device) ------------------------------------------
def test_lib_compare_refuses_bad_arguments_before_the_device(hip):
    lib = hip.load()
    xa, xb, xq = np.array([1.0, 4.0, 16.0]), np.array([2.0, 8.0]), np.array([2.0, 4.0])
    ya, yb = np.ones((3, 2, 3)), np.ones((2, 2, 2))
    err, arg, worst = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros((2, 2))
    # G, La, Lb, na, xa, ya, nb, xb, yb, nq, xq, err, arg, worst
    good = [2, 3, 2, 3, dp(xa), dp(ya), 2, dp(xb), dp(yb), 2, dp(xq), dp(err), ip(arg), dp(worst)]

    def refused(pos, value, word):
        a = list(good)
        a[pos] = value
        assert lib.ndpp_lib_compare(*a) == -22, (pos, value)
        msg = lib.ndpp_last_error()
        assert b"lib_compare" in msg and word in msg, (pos, value, msg)

    for pos in (4, 5, 7, 8, 10, 11, 12):
        refused(pos, None, b"NULL")
    for pos, word in ((0, b"G="), (1, b"La="), (2, b"Lb=")):
        for v in (0, -3):
            refused(pos, v, word)
    for pos, word in ((3, b"na="), (6, b"nb=")):
        for v in (1, 0, -1):
            refused(pos, v, word)
    for v in (0, -1):
        refused(9, v, b"nq=")
    for bad in ([1.0, 4.0, 4.0], [1.0, 4.0, 3.0], [0.0, 4.0, 16.0], [-1.0, 4.0, 16.0], [1.0, np.nan, 16.0], [1.0, 4.0, np.inf]):
        xbad = np.array(bad)
        refused(4, dp(xbad), b"xa must be strictly increasing")
    for bad in ([2.0, 2.0], [8.0, 2.0], [0.0, 2.0], [2.0, np.inf], [np.nan, 2.0]):
        xbad = np.array(bad)
        refused(7, dp(xbad), b"xb must be strictly increasing")
    a = list(good)
    a[0] = a[1] = 40000                               # G * La does not fit an index
    assert lib.ndpp_lib_compare(*a) == -22 and b"G * L" in lib.ndpp_last_error()
    a = list(good)
    a[0] = a[2] = 40000
    assert lib.ndpp_lib_compare(*a) == -22 and b"G * L" in lib.ndpp_last_error()
    # worst may be NULL: a valid call, which without a device is the device error
    if lib.ndpp_device_count() == 0:
        assert lib.ndpp_lib_compare(*good) == -5
        a = list(good)
        a[13] = None
        assert lib.ndpp_lib_compare(*a) == -5
        with pytest.raises(hip.NdppError) as e:
            hip.lib_compare(xa, ya, xb, yb, xq)
        assert e.value.code == -5
    with pytest.raises(ValueError):
        hip.lib_compare(xa[:2], ya, xb, yb, xq)
    with pytest.raises(ValueError):
        hip.lib_compare(xa, ya, xb, np.ones((2, 3, 2)), xq)


# ---- compare_numpy -----------------------------------------------------------------------------------
def rows(x, G=2, L=3, bend=0.0):
    """y[n][G][L]: P0 = g + 1, the other moments linear in u = log2 x (plus bend * u^2)"""
    u = np.log2(np.asarray(x, dtype=np.float64))
    y = np.zeros((len(u), G, L))
    for g in range(G):
        y[:, g, 0] = g + 1.0
        for l in range(1, L):
            y[:, g, l] = (u + bend * u * u) * (g + 1) / (4.0 * l)
    return y


def test_a_section_against_itself_is_zero_everywhere():
    x = 4.0 ** np.arange(-3, 4)
    y = rows(x, bend=0.3)
    xq = np.concatenate([x, np.sqrt(x[:-1] * x[1:]), [3.3, 0.017]])
    err, arg, worst = cp().compare_numpy(x, y, x, y, xq)
    assert np.array_equal(err, np.zeros(len(xq))) and np.array_equal(arg, np.zeros(len(xq), dtype=np.int32))
    assert np.array_equal(worst, np.zeros((2, 3)))


def test_one_perturbed_element_shows_at_its_energy_and_not_beyond_its_neighbours():
    x = 4.0 ** np.arange(-3, 4)                   # 7 points; f = 1/2 exactly at the midpoints (ratio 4, midpoints ratio 2)
    ya = rows(x)
    yb = ya.copy()
    delta = 2.0 ** -10
    yb[3, 1, 2] += delta                          # row 3, group 1, moment 2; scale: P0 of group 1 = 2
    mids = 2.0 * x[:-1]
    xq = np.concatenate([x, mids])
    err, arg, worst = cp().compare_numpy(x, ya, x, yb, xq)
    want = np.zeros(len(xq))
    want[3] = delta / 2.0
    want[7 + 2] = want[7 + 3] = 0.5 * delta / 2.0  # the midpoints of the two intervals row 3 bounds
    assert np.array_equal(err, want)
    assert arg[3] == 1 * 3 + 2 and arg[9] == 5 and arg[10] == 5
    assert np.array_equal(err[[0, 1, 2, 4, 5, 6, 7, 8, 11, 12]], np.zeros(10))     # 0 beyond the two neighbours
    w = np.zeros((2, 3))
    w[1, 2] = delta / 2.0
    assert np.array_equal(worst, w)


def test_exact_hits_return_the_stored_rows_difference_exactly():
    rng = np.random.default_rng(3)
    xa = np.array([0.5, 1.0, 3.0, 7.0, 20.0])
    xb = np.array([0.5, 2.0, 3.0, 20.0])          # common points 0.5, 3.0 and the last one, 20.0
    ya, yb = rng.normal(size=(5, 2, 2)), rng.normal(size=(4, 2, 2))
    err, arg, _ = cp().compare_numpy(xa, ya, xb, yb, [0.5, 3.0, 20.0])
    for k, (i, j) in enumerate(((0, 0), (2, 2), (4, 3))):
        d = np.abs(ya[i] - yb[j]).ravel()
        i1, j1 = min(i + 1, 4), min(j + 1, 3)
        scale = max(np.abs(ya[[i, i1], :, 0]).max(), np.abs(yb[[j, j1], :, 0]).max())
        assert err[k] == d.max() / scale and arg[k] == int(np.argmax(d)), k


def test_zero_scale_nan_infinity_and_queries_outside():
    xa, xb = np.array([1.0, 4.0, 16.0, 64.0]), np.array([2.0, 8.0, 32.0])
    ya, yb = np.ones((4, 2, 2)), np.ones((3, 2, 2))
    ya[:, :, 1], yb[:, :, 1] = 0.25, 0.5
    # P0 = 0 in all four rows involved at x = 2.5 .. 4: rows 0, 1 of A and 0, 1 of B
    ya[0:2, :, 0] = 0.0
    yb[0:2, :, 0] = 0.0
    err, arg, worst = cp().compare_numpy(xa, ya, xb, yb, [3.0])
    assert err[0] == 0.0 and arg[0] == 1 and np.array_equal(worst, np.zeros((2, 2)))      # the higher moment differs: still 0
    # a NaN and an infinity: +inf, arg the lowest such element, worst +inf for those elements alone
    ya[2, 1, 0] = np.nan
    ya[2, 1, 1] = np.inf
    xq = np.array([3.0, 9.0, 20.0, 1.5, 40.0, 0.0, -2.0, np.nan, np.inf, 2.0, 32.0])
    err, arg, worst = cp().compare_numpy(xa, ya, xb, yb, xq)
    assert err[0] == 0.0
    assert err[1] == INF and arg[1] == 2 and err[2] == INF and arg[2] == 2       # row 2 of A on either side
    assert np.array_equal(err[3:9], np.full(6, -1.0)) and np.array_equal(arg[3:9], np.full(6, -1))
    assert err[9] == 0.0 and err[10] == INF         # the first and the last common point are inside
    assert worst[1, 0] == INF and worst[1, 1] == INF and np.isfinite(worst[0]).all()
    # every query skipped: worst stays -1
    _, _, w = cp().compare_numpy(xa, ya, xb, yb, [1.0, 50.0])
    assert np.array_equal(w, np.full((2, 2), -1.0))
    with pytest.raises(ValueError):
        cp().compare_numpy([1.0, 1.0], ya[:2], xb, yb, [3.0])


def test_different_orders_compare_the_first_min_entries_only():
    rng = np.random.default_rng(5)
    xa, xb = np.array([1.0, 3.0, 9.0, 20.0]), np.array([0.5, 2.0, 8.0, 30.0, 40.0])
    ya, yb = rng.normal(size=(4, 3, 6)), rng.normal(size=(5, 3, 11))
    xq = cp().union_queries(xa, xb)
    err, arg, worst = cp().compare_numpy(xa, ya, xb, yb, xq)
    e2, a2, w2 = cp().compare_numpy(xa, ya, xb, np.ascontiguousarray(yb[:, :, :6]), xq)
    assert worst.shape == (3, 6) and np.array_equal(err, e2) and np.array_equal(arg, a2) and np.array_equal(worst, w2)
    yb[:, :, 6:] = np.nan                            # what is not compared is not read
    e3, _, _ = cp().compare_numpy(xa, ya, xb, yb, xq)
    assert np.array_equal(err, e3) and arg.max() < 18
    e4, a4, w4 = cp().compare_numpy(xb, yb, xa, ya, xq)     # and the other way round
    assert np.array_equal(e4, err) and np.array_equal(a4, arg) and np.array_equal(w4, worst)


# ---- where the supremum lies ----------------------------------------------------------------------------
def random_sections(seed, na, nb, G, La, Lb):
    rng = np.random.default_rng(seed)
    xa = np.sort(np.exp(rng.uniform(-6.0, 3.0, na)))
    xb = np.sort(np.exp(rng.uniform(-5.0, 4.0, nb)))
    return xa, rng.normal(size=(na, G, La)), xb, rng.normal(size=(nb, G, Lb))


@pytest.mark.parametrize("seed,na,nb,G,La,Lb", [(11, 9, 13, 3, 4, 4), (12, 17, 6, 1, 2, 5), (13, 12, 12, 4, 6, 3), (14, 30, 41, 2, 1, 1)])
def test_no_point_inside_a_union_interval_exceeds_the_union_queries(seed, na, nb, G, La, Lb):
    """err over 64 log-spaced points strictly inside every interval of the union of the grids never
    exceeds the maximum over union_queries by more than 4 eps of it.  The rows are random, so the scale
    differs from row to row: this holds only because union_queries reads the limit from below every
    union point as well (the next test)."""
    xa, ya, xb, yb = random_sections(seed, na, nb, G, La, Lb)
    u = cp().union_points(xa, xb)
    at_union = cp().compare_numpy(xa, ya, xb, yb, cp().union_queries(xa, xb))[0].max()
    t = np.arange(1, 65) / 65.0
    inside = np.exp(np.log(u[:-1])[:, None] + np.log(u[1:] / u[:-1])[:, None] * t[None, :]).ravel()
    assert ((inside > np.repeat(u[:-1], 64)) & (inside < np.repeat(u[1:], 64))).all()
    e = cp().compare_numpy(xa, ya, xb, yb, inside)[0]
    assert (e >= 0).all()
    print(f"seed {seed}: {len(u)} union points, max at the union queries {at_union:.17g}, inside {e.max():.17g}")
    assert e.max() <= at_union + 4 * EPS * at_union


def test_the_scale_jumps_at_a_grid_point_and_union_queries_reads_the_limit_from_below():
    # G = 1, L = 2.  A: P0 = 1, 1, 1000 at x = 1, 4, 16; B: the same P0; P1 differs by 1 at x = 4 only.
    # Below 4 the rows involved have P0 = 1: err -> 1.  At 4 itself the rows are 4 and 16: err = 1 / 1000.
    x = np.array([1.0, 4.0, 16.0])
    ya = np.zeros((3, 1, 2))
    ya[:, 0, 0] = [1.0, 1.0, 1000.0]
    yb = ya.copy()
    yb[1, 0, 1] = 1.0
    assert np.array_equal(cp().union_points(x, x), x)
    err, _, _ = cp().compare_numpy(x, ya, x, yb, x)
    assert np.array_equal(err, [0.0, 1e-3, 0.0])
    xq = cp().union_queries(x, x)
    assert np.array_equal(xq, [1.0, np.nextafter(4.0, 0.0), 4.0, np.nextafter(16.0, 0.0), 16.0])
    err, arg, worst = cp().compare_numpy(x, ya, x, yb, xq)
    assert abs(err[1] - 1.0) <= 4 * EPS and arg[1] == 1 and err[2] == 1e-3
    rep = cp().compare_sections((x, ya), (x, yb), cp().compare_numpy)
    assert rep["comparable"] and rep["err"] == err[1] and rep["energy"] == xq[1] and (rep["group"], rep["moment"]) == (0, 1)
    assert rep["queries"] == 5 and rep["worst"][0, 1] == err[1] and rep["worst"][0, 0] == 0.0


def test_compare_sections_reports_what_lies_outside_and_what_cannot_be_compared():
    c = cp()
    xa, ya, xb, yb = random_sections(21, 8, 11, 2, 3, 3)
    rep = c.compare_sections((xa, ya), (xb, yb), c.compare_numpy)
    lo, hi = max(xa[0], xb[0]), min(xa[-1], xb[-1])
    assert rep["comparable"] and rep["moments"] == 3 and rep["worst"].shape == (2, 3)
    assert rep["outside_a"]["points"] == int(((xa < lo) | (xa > hi)).sum()) > 0
    assert rep["outside_b"]["points"] == int(((xb < lo) | (xb > hi)).sum()) > 0
    assert rep["outside_a"]["below"] == [xa[0], lo] and rep["outside_a"]["above"] is None
    assert rep["outside_b"]["below"] is None and rep["outside_b"]["above"] == [hi, xb[-1]]
    assert rep["err"] == rep["worst"].max() and lo <= rep["energy"] <= hi
    dup = xa.copy()
    dup[3] = dup[2]
    assert c.compare_sections((dup, ya), (xb, yb), c.compare_numpy) == dict(comparable=False, reason="not comparable: grid not increasing")
    assert c.compare_sections((xa, ya), (xb, yb[:, :1]), c.compare_numpy)["reason"] == "not comparable: different group structure"
    assert c.compare_sections((xa, ya), (xb + 1e3, yb), c.compare_numpy)["reason"] == "not comparable: no common energy range"


# ---- tables and directories (the input half) ----------------------------------------------------------------
def golden_dir(tmp_path, name, sub=""):
    """a copy of the golden run directory with RUNDIR substituted, as the driver would have left it"""
    d = tmp_path / name
    shutil.copytree(GOLD / sub if sub else GOLD, d, ignore=shutil.ignore_patterns("chi_sab") if not sub else None)
    xml = d / "ndpp_lib.xml"
    xml.write_text(xml.read_text().replace("RUNDIR", str(d.resolve())))
    return d


def test_compare_tables_names_every_section_and_every_reason():
    from ndpp_amd import reader
    c = cp()
    t = reader.read_binary((GOLD / "chi_sab" / "94239.71c.g7").read_bytes())
    u = reader.read_binary((GOLD / "92238.71c.g2").read_bytes())
    secs = c.compare_tables(t, t, c.compare_numpy)
    assert list(secs) == ["elastic", "chi-total", "chi-prompt", "chi-delayed-1", "chi-delayed-2", "chi-delayed-3"]
    assert all(s["comparable"] and s["err"] == 0.0 for s in secs.values())
    assert secs["chi-total"]["moments"] == 1 and secs["chi-total"]["worst"].shape == (t.groups, 1)
    secs = c.compare_tables(u, u, c.compare_numpy)
    assert list(secs) == ["elastic", "inelastic", "nu-inelastic"] and all(s["err"] == 0.0 for s in secs.values())
    # another group structure: nothing is comparable; sections one side lacks are named
    secs = c.compare_tables(u, t, c.compare_numpy)
    assert secs["elastic"]["reason"] == "not comparable: different group structure"
    assert secs["inelastic"]["reason"] == "not comparable: section only in A"
    assert secs["chi-total"]["reason"] == "not comparable: section only in B"
    assert not any(s["comparable"] for s in secs.values())
    # scatt_type: tabular on both sides, and on one
    import copy
    tab = copy.deepcopy(u)
    tab.scatt_type = reader.SCATT_TYPE_TABULAR
    assert {s["reason"] for s in c.compare_tables(tab, tab, c.compare_numpy).values()} == {"not comparable: tabular output"}
    assert {s["reason"] for s in c.compare_tables(tab, u, c.compare_numpy).values()} == {"not comparable: different scatt_type"}
    # a P3 copy against the P5 table: the first four moments, equal
    low = copy.deepcopy(u)
    low.scatt_order = 3
    for s in (low.elastic, low.inelastic, low.nuinelastic):
        s.mat = np.ascontiguousarray(s.mat[:, :, :4])
    secs = c.compare_tables(low, u, c.compare_numpy)
    assert all(s["comparable"] and s["err"] == 0.0 and s["moments"] == 4 for s in secs.values())
    # a grid with a repeated energy
    bad = copy.deepcopy(u)
    bad.elastic.ein = bad.elastic.ein.copy()
    bad.elastic.ein[5] = bad.elastic.ein[4]
    secs = c.compare_tables(bad, u, c.compare_numpy)
    assert secs["elastic"]["reason"] == "not comparable: grid not increasing" and secs["inelastic"]["comparable"]


def test_compare_dirs_matches_tables_by_name_and_reports_one_sided_ones(tmp_path):
    c = cp()
    a = golden_dir(tmp_path, "a", "chi_sab")
    b = golden_dir(tmp_path, "b", "chi_sab")
    rep = c.compare_dirs(a, b, 1e-12, compare=c.compare_numpy)
    assert [t["name"] for t in rep["tables"]] == ["94239.71c", "hh2o.10t", "grph.10t", "be.10t"]
    assert rep["only_in_a"] == rep["only_in_b"] == rep["above"] == rep["not_comparable"] == [] and rep["err"] == 0.0
    # B loses a table and lists the others in another order; one path attribute points nowhere: the file next to the xml is read
    xml = b / "ndpp_lib.xml"
    lines = xml.read_text().splitlines(keepends=True)
    tabs = [ln for ln in lines if "<ndpp_table" in ln]
    rest = [ln for ln in lines if "<ndpp_table" not in ln]
    keep = [tabs[3], tabs[0].replace('path="94239.71c.g7"', 'path="/nowhere/at/all/94239.71c.g7"'), tabs[1]]
    xml.write_text("".join(rest[:-1] + keep + rest[-1:]))
    rep = c.compare_dirs(a, b, compare=c.compare_numpy)
    assert [t["name"] for t in rep["tables"]] == ["94239.71c", "hh2o.10t", "be.10t"]
    assert rep["only_in_a"] == ["grph.10t"] and rep["only_in_b"] == []
    rep = c.compare_dirs(b, a, compare=c.compare_numpy)
    assert rep["only_in_a"] == [] and rep["only_in_b"] == ["grph.10t"]
    lines = c.format_lines(rep)
    assert len(lines) == 6 + 1 + 1 + 1 and lines[-1].split() == ["grph.10t", "only", "in", "B"]
    # one table of A with another group edge (byte 22 on: name[10], kT, G, then the edges)
    f = a / "hh2o.10t.g7"
    raw = bytearray(f.read_bytes())
    edge = struct.unpack_from("<d", raw, 22 + 8)[0]
    struct.pack_into("<d", raw, 22 + 8, edge * 1.5)
    f.write_bytes(bytes(raw))
    rep = c.compare_dirs(a, b, 1e-12, compare=c.compare_numpy)
    assert rep["not_comparable"] == [("hh2o.10t", "elastic")] and rep["above"] == []
    hh = [t for t in rep["tables"] if t["name"] == "hh2o.10t"][0]["sections"]["elastic"]
    assert hh == dict(comparable=False, reason="not comparable: different group structure")
    assert any("hh2o.10t" in ln and "not comparable: different group structure" in ln for ln in c.format_lines(rep))
    # a perturbed moment: above a tolerance, named with its place
    f = a / "be.10t.g7"
    from ndpp_amd import reader
    t = reader.read_binary(f.read_bytes())
    raw = bytearray(f.read_bytes())
    iE = 40
    g0 = int(t.elastic.gmin[iE]) - 1
    v = t.elastic.mat[iE, g0, 1]
    at = bytes(raw).find(struct.pack("<d", v))
    struct.pack_into("<d", raw, at, v + 1e-3)
    f.write_bytes(bytes(raw))
    rep = c.compare_dirs(a, b, 1e-6, compare=c.compare_numpy)
    assert rep["above"] == [("be.10t", "elastic")] and rep["at"] == ("be.10t", "elastic") and rep["err"] > 1e-6
    import json
    js = json.dumps(c.as_json(rep))
    assert "be.10t" in js and "Infinity" not in js


def test_cli_exit_statuses(hip, tmp_path, capsys):
    c = cp()
    a = golden_dir(tmp_path, "a")
    assert c.main([str(a), str(tmp_path / "missing")]) == 2
    assert "input error" in capsys.readouterr().err
    assert c.main([str(tmp_path / "missing"), str(a)]) == 2
    (tmp_path / "empty").mkdir()
    assert c.main([str(a), str(tmp_path / "empty")]) == 2
    for tol in ("x", "nan", "-1", "inf"):
        assert c.main([str(a), str(a), "--tol", tol]) == 2
    trunc = golden_dir(tmp_path, "trunc")
    f = trunc / "92238.71c.g2"
    f.write_bytes(f.read_bytes()[:1000])
    assert c.main([str(a), str(trunc)]) == 2
    capsys.readouterr()
    js = tmp_path / "rep.json"
    rc = c.main([str(a), str(a), "--tol", "1e-12", "--json", str(js)])
    out = capsys.readouterr()
    if hip.load().ndpp_device_count() == 0:
        assert rc == 3 and "library error" in out.err and "error -5" in out.err and not js.exists()
    else:
        assert rc == 0 and js.exists() and "92238.71c" in out.out
