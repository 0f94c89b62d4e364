"""ndpp_amd.derive on the CPU: the whole tool with the numpy restatements injected, the host tables,
and the command line (no GPU).  The device is pinned to the same restatements in test_gpu_derive.py."""
import json
import shutil
from pathlib import Path

import numpy as np
import pytest
from numpy.polynomial import legendre as npleg

import tabular_ref
from ndpp_amd import compare, derive, reader, sample, validate

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "e2e"
BIN_COUNTS = (1, 3, 7, 32, 128)
EPS = np.finfo(float).eps
NK = derive.NUMPY_KERNELS


def positive_rows(n=40, seed=5, lmax=10):
    """squares of random degree-5 Legendre series plus 1e-3, as (rows [n][lmax + 1] of moments, the
    coefficient rows): the moments by a 64-point Gauss rule, exact for these degree-10 densities"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, 6))
    x, w = npleg.leggauss(64)
    f = npleg.legval(x, c.T) ** 2 + 1e-3
    P = np.array([npleg.Legendre.basis(l)(x) for l in range(lmax + 1)])
    return (f * w) @ P.T, c


@pytest.fixture(scope="module")
def rows(hip):
    return positive_rows()


def edges(N):
    e = -1.0 + 2.0 * np.arange(N + 1) / N
    e[-1] = 1.0
    return e


def run_cli(args, kernels=NK):
    return derive.main([str(a) for a in args], kernels)


def exact(e):
    return repr(float(e))


# ---- identity: the reader and the writers meet ---------------------------------------------------

@pytest.mark.parametrize("sub", ["chi_sab", "."])
def test_identity_reproduces_the_reference_library(hip, tmp_path, sub):
    src = (GOLD / sub).resolve()
    tabs = compare.read_library(src)
    e_bins = next(iter(tabs.values()))[1].e_bins
    out = tmp_path / "out"
    assert run_cli([src, out, "--groups", *map(exact, e_bins)]) == 0
    assert len(tabs) == (4 if sub == "chi_sab" else 1)
    for attrs, _ in tabs.values():
        assert (out / attrs["path"]).read_bytes() == (src / attrs["path"]).read_bytes(), attrs["path"]
    a = reader.read_lib_xml((out / "ndpp_lib.xml").read_bytes())
    b = reader.read_lib_xml((src / "ndpp_lib.xml").read_bytes())
    assert set(a) == set(b)
    for k in a:
        if k == "energy_bins":
            assert np.array_equal(a[k], b[k])
        elif k != "directory":
            assert a[k] == b[k], k
    assert a["directory"] != b["directory"]


# ---- condensation ------------------------------------------------------------------------------

def test_one_group_equals_condense_in_every_bit(hip):
    tabs = compare.read_library(GOLD / "chi_sab")
    seen = 0
    for _, t in tabs.values():
        one, rep = derive.table(t, groups=[t.e_bins[0], t.e_bins[-1]], kernels=NK)
        assert one.groups == 1 and rep["flagged"] == 0
        for name in derive.SECTIONS:
            s = getattr(t, name)
            if s is None:
                continue
            got = getattr(one, name)
            assert np.array_equal(got.mat[:, 0], validate.condense(s)) and got.mat.shape[1] == 1
            assert np.array_equal(got.ein, s.ein)
            seen += 1
        if t.chi:
            for name in ("total", "prompt"):
                assert np.array_equal(one.chi[name][:, 0], validate.condense(t.chi[name][:, :, None])[:, 0])
            d = t.chi["delayed"]
            assert one.chi["delayed"].shape == d.shape[:2] + (1,)
            for j in range(d.shape[0]):
                assert np.array_equal(one.chi["delayed"][j, :, 0], validate.condense(d[j][:, :, None])[:, 0])
            seen += 10
    assert seen > 10          # the chi rows of the fissile table were among them


def test_regrouping_in_two_steps_is_equal_to_rounding(hip):
    """7 -> 3 -> 1 adds the same numbers in another order than 7 -> 1: equal to 1e-15 of the row's scale
    (the largest |P0| of the incoming energy), not in bits.  Measured on these tables: 3.9e-16."""
    worst = 0.0
    for _, t in compare.read_library(GOLD / "chi_sab").values():
        e = t.e_bins
        three, _ = derive.table(t, groups=[e[0], e[2], e[5], e[7]], kernels=NK)
        a, _ = derive.table(three, groups=[e[0], e[7]], kernels=NK)
        b, _ = derive.table(t, groups=[e[0], e[7]], kernels=NK)
        assert np.array_equal(three.e_bins, e[[0, 2, 5, 7]])
        for name in derive.SECTIONS:
            if getattr(t, name) is None:
                continue
            scale = np.abs(getattr(t, name).mat[:, :, 0]).max(axis=1)
            scale[scale == 0.0] = 1.0
            d = np.abs(getattr(a, name).mat - getattr(b, name).mat)[:, 0] / scale[:, None]
            worst = max(worst, float(d.max()))
    print("7 -> 3 -> 1 against 7 -> 1:", worst)
    assert worst <= 1e-15


def test_group_edges_must_be_the_tables_own(hip):
    t = next(iter(compare.read_library(GOLD / "chi_sab").values()))[1]
    e = t.e_bins
    assert derive.group_segments(e, e[[0, 3, 7]]).tolist() == [0, 3, 7]
    for bad in ([e[0], np.nextafter(e[3], 1.0), e[7]], [e[0], e[3]], [e[1], e[7]], [e[0], e[3], e[3], e[7]], [e[0]]):
        with pytest.raises(derive.InputError):
            derive.group_segments(e, bad)


# ---- bins from moments -------------------------------------------------------------------------

@pytest.mark.parametrize("N", BIN_COUNTS)
def test_bins_of_positive_rows(hip, rows, N):
    a, c = rows
    t, status = derive.bins_numpy(a[:, None, :], N)
    t, a0 = t[:, 0], a[:, 0]
    assert t.dtype == np.float64 and status.dtype == np.int32 and (status == 0).all()
    total = np.abs(t.sum(axis=1) - a0) / a0
    # a 16-point Gauss rule on each bin integrates the degree-10 density exactly
    x, w = npleg.leggauss(16)
    e = edges(N)
    mid, half = 0.5 * (e[1:] + e[:-1]), 0.5 * (e[1:] - e[:-1])
    pts = mid[:, None] + half[:, None] * x                                    # [N][16]
    f = npleg.legval(pts, c.T) ** 2 + 1e-3                                    # [rows][N][16]
    want = (f * w).sum(axis=2) * half
    err = np.abs(t - want).max(axis=1) / a0
    print(f"N = {N}: sum against a_0 {total.max():.2e}, bins against Gauss {err.max():.2e}")
    assert total.max() <= 1e-14 and err.max() <= 1e-13
    assert (t >= 0.0).all()
    if N == 1:
        W = hip.derive_tables(11, 1)[0]
        assert np.array_equal(t[:, 0], a0 * W[0, 0]) and W[0, 0] == 1.0


def test_negative_row_is_flagged_where_the_bins_resolve_it(hip):
    """f = 1/2 (1 + 2.6 P_2) of DESIGN.md section 18 is negative around mu = 0: a_0 = 1, a_2 = 1.3 / 2.5"""
    a = np.zeros((1, 1, 3))
    a[0, 0] = [1.0, 0.0, 0.52]
    t, st = derive.bins_numpy(a, 128)
    assert st[0, 0] == hip.DERIVE_NEGBIN and t.min() < 0.0
    t, st = derive.bins_numpy(a, 1)
    assert st[0, 0] == 0 and t[0, 0, 0] == 1.0


def test_bins_status_bits(hip):
    a = np.zeros((5, 1, 4))
    a[0, 0] = [0.0, 0.3, 0.0, 0.0]                  # a_0 == 0: zeros, whatever follows
    a[1, 0] = [1.0, np.nan, 0.0, 0.0]
    a[2, 0] = [np.inf, 0.0, 0.0, 0.0]
    a[3, 0] = [0.0, np.nan, 0.0, 0.0]
    a[4, 0] = [1.0, 0.2, 0.1, 0.0]
    t, st = derive.bins_numpy(a, 7)
    assert st[:, 0].tolist() == [hip.DERIVE_ZERO, hip.DERIVE_NONFINITE, hip.DERIVE_NONFINITE,
                                 hip.DERIVE_ZERO | hip.DERIVE_NONFINITE, 0]
    assert (t[0] == 0.0).all() and (t[3] == 0.0).all() and np.isnan(t[1]).all()


# ---- moments from bins -------------------------------------------------------------------------

@pytest.mark.parametrize("N", BIN_COUNTS)
def test_moments_of_bins_and_the_round_trip(hip, rows, N):
    a, _ = rows
    t, _ = derive.bins_numpy(a.reshape(8, 5, 11), N)
    out, lo, hi, st = derive.moments_numpy(t, 11)
    assert (st == 0).all() and out.shape == lo.shape == hi.shape == (8, 5, 11)
    assert np.array_equal(out[:, :, 0], sample._masses(reader.SCATT_TYPE_TABULAR, t))
    assert (lo <= out).all() and (out <= hi).all()
    S = out[:, :, :1]
    orig = a.reshape(8, 5, 11)
    excess = np.maximum(lo - orig, orig - hi) / S
    print(f"N = {N}: largest excess {excess.max():.2e} S, widest enclosure {((hi - lo) / S).max():.2e} S, "
          f"histogram's moments off by {(np.abs(out - orig) / S).max():.2e} S")
    assert (orig >= lo - 1e-13 * S).all() and (orig <= hi + 1e-13 * S).all()
    # without bounds: the same moments and statuses
    out2, lo2, hi2, st2 = derive.moments_numpy(t, 11, bounds=False)
    assert lo2 is None and hi2 is None and np.array_equal(out2, out) and np.array_equal(st2, st)


def test_moments_status_bits(hip):
    t = np.full((4, 1, 7), 0.1)
    t[1, 0, 3] = -0.05
    t[2, 0, 0] = np.nan
    t[3, 0, 6] = np.inf
    _, _, _, st = derive.moments_numpy(t, 3)
    assert st[:, 0].tolist() == [0, hip.DERIVE_NEGBIN, hip.DERIVE_NONFINITE, hip.DERIVE_NONFINITE]


@pytest.mark.parametrize("N", BIN_COUNTS)
def test_extremes_are_the_reference_ones_moved_by_eight_ulp(hip, N):
    """pmin and pmax against tests/tabular_ref.legendre_bin_extremes less and plus 8 ulp of 1.  Both sides
    evaluate P_l in double: against 40-digit arithmetic the reference's extremes are up to 7 ulp off at
    l <= 10 (its roots come from a companion matrix) and these within 1, so "nothing else" is 8 ulp --
    which also says that the true extreme lies inside every bound."""
    W, V, pmin, pmax = hip.derive_tables(11, N)
    rmin, rmax = tabular_ref.legendre_bin_extremes(N, 10)
    assert np.abs(pmin - (rmin - 8 * EPS)).max() <= 8 * EPS
    assert np.abs(pmax - (rmax + 8 * EPS)).max() <= 8 * EPS
    assert (pmin <= rmin).all() and (pmax >= rmax).all()
    assert (pmin <= V).all() and (V <= pmax).all() and (V[0] == 1.0).all()
    assert np.abs(W.sum(axis=1) - np.eye(11)[0]).max() <= 4 * EPS


def test_tables_refuse_bad_sizes(hip):
    for L, N in ((0, 4), (12, 4), (3, 0), (3, 129)):
        with pytest.raises(hip.NdppError) as e:
            hip.derive_tables(L, N)
        assert e.value.code == hip.NDPP_EINVAL


def test_bad_argument_is_reported_before_the_device(hip):
    """the missing device (NDPP_EDEVICE on a machine without one) must not be what a bad call reports"""
    for call in (lambda: hip.derive_bins(np.zeros((1, 1, 12)), 4), lambda: hip.derive_bins(np.zeros((1, 1, 3)), 129),
                 lambda: hip.derive_moments(np.zeros((1, 1, 4)), 12),
                 lambda: hip.derive_groups(np.zeros((1, 3, 2)), [0, 2, 2, 3]),
                 lambda: hip.derive_groups(np.zeros((1, 3, 2)), [0, 2])):
        with pytest.raises(hip.NdppError) as e:
            call()
        assert e.value.code == hip.NDPP_EINVAL, str(e.value)


# ---- rebinning ---------------------------------------------------------------------------------

def test_rebinning(hip, rows):
    """128 -> 32 sums four bins where the direct table takes one difference: equal to 1e-15 of the row's
    mass (measured here: 8.8e-17); 128 -> 128 is the identity in bits"""
    a, _ = rows
    leg = reader.NdppTable("x", 2.53e-8, np.array([0.0, 1.0, 2.0, 3.0, 4.0, 20.0]), reader.SCATT_TYPE_LEGENDRE, 10,
                           False, False, 65, 0.0)
    ein = np.geomspace(1e-5, 20.0, 8)
    mat = a.reshape(8, 5, 11)
    leg.elastic = reader.ScattSection(ein, np.ones(6, np.int32), np.ones(8, np.int32), np.full(8, 5, np.int32), mat)
    t128, _ = derive.table(leg, bins=128, kernels=NK)
    t32, _ = derive.table(leg, bins=32, kernels=NK)
    assert (t128.scatt_type, t128.scatt_order, t128.moments) == (reader.SCATT_TYPE_TABULAR, 128, 128)
    m32, rep = derive.table(t128, bins=32, kernels=NK)
    assert (m32.scatt_order, m32.elastic.mat.shape) == (32, (8, 5, 32)) and rep["flagged"] == 0
    d = np.abs(m32.elastic.mat - t32.elastic.mat) / mat[:, :, :1]
    print("128 -> 32 against 32:", d.max())
    assert d.max() <= 1e-15
    same, _ = derive.table(t128, bins=128, kernels=NK)
    assert np.array_equal(same.elastic.mat, t128.elastic.mat)
    with pytest.raises(derive.InputError, match="divide"):
        derive.table(t128, bins=48, kernels=NK)
    # and back: the first moments of a Legendre table are a cut
    cut, _ = derive.table(leg, moments=4, kernels=NK)
    assert cut.scatt_order == 3 and np.array_equal(cut.elastic.mat, mat[:, :, :4])
    with pytest.raises(derive.InputError, match="stored"):
        derive.table(cut, moments=5, kernels=NK)
    with pytest.raises(derive.InputError):
        derive.table(leg, bins=4, moments=2, kernels=NK)


def test_slices_change_no_bit(hip):
    t = next(iter(compare.read_library(GOLD).values()))[1]
    whole, _ = derive.table(t, groups=[t.e_bins[0], t.e_bins[-1]], bins=7, kernels=NK)
    per_energy = 1 * 7 * 8
    cut, _ = derive.table(t, groups=[t.e_bins[0], t.e_bins[-1]], bins=7, kernels=NK,
                          max_bytes=per_energy * (len(t.elastic.ein) // 3 + 1))
    for name in derive.SECTIONS:
        assert np.array_equal(getattr(whole, name).mat, getattr(cut, name).mat)


# ---- the command line --------------------------------------------------------------------------

@pytest.fixture()
def planted(hip, tmp_path):
    """the golden two-group library with f = 1/2 (1 + 2.6 P_2) planted in one elastic row"""
    src = tmp_path / "planted"
    shutil.copytree(GOLD, src, ignore=shutil.ignore_patterns("chi_sab"))
    path = src / "92238.71c.g2"
    data = path.read_bytes()
    t = reader.read_binary(data)
    g = int(t.elastic.gmin[3]) - 1
    t.elastic.mat[3, g] = [1.0, 0.0, 0.52, 0.0, 0.0, 0.0]
    path.write_bytes(derive.table_file(t, 2, derive.stored_name(data, 2)))
    return src


def test_cli_ok_and_report(hip, tmp_path):
    src = GOLD / "chi_sab"
    e = next(iter(compare.read_library(src).values()))[1].e_bins
    out = tmp_path / "o"
    assert run_cli([src, out, "--groups", exact(e[0]), exact(e[3]), exact(e[7]), "--bins", "2", "--json",
                    tmp_path / "r.json"]) == 0
    rep = json.loads((tmp_path / "r.json").read_text())
    assert len(rep["tables"]) == 4 and rep["flagged"] == 0 and rep["request"]["bins"] == 2
    lib_out = compare.read_library(out)
    for _, t in lib_out.values():
        assert (t.groups, t.scatt_type, t.moments) == (2, reader.SCATT_TYPE_TABULAR, 2)
    assert lib_out["94239.71c"][1].chi["total"].shape[1] == 2
    assert validate.main([str(out)]) == 0
    # and the moments of that tabular library, with the enclosure's width per l in the report
    back = tmp_path / "back"
    assert run_cli([out, back, "--moments", "3", "--json", tmp_path / "b.json"]) == 0
    rep = json.loads((tmp_path / "b.json").read_text())
    w = rep["tables"][0]["sections"]["elastic"]["width"]
    assert len(w) == 3 and 0.0 <= w[0] <= 64 * EPS and all(0.0 < v < 2.0 for v in w[1:])
    for _, t in compare.read_library(back).values():
        assert (t.scatt_type, t.scatt_order) == (reader.SCATT_TYPE_LEGENDRE, 2)


def test_cli_flags_the_negative_rows_the_validator_finds(hip, tmp_path):
    """the golden library's P5 rows are negative in places: at 32 bins the derived library has negative
    bins, the run exits 1, and validate counts the same rows in every table and section"""
    src = GOLD / "chi_sab"
    e = next(iter(compare.read_library(src).values()))[1].e_bins
    out = tmp_path / "o"
    assert run_cli([src, out, "--groups", exact(e[0]), exact(e[3]), exact(e[7]), "--bins", "32", "--json",
                    tmp_path / "r.json"]) == derive.EXIT_FLAGGED
    rep = json.loads((tmp_path / "r.json").read_text())
    assert validate.main([str(out), "--json", str(tmp_path / "v.json")]) == 1
    val = json.loads((tmp_path / "v.json").read_text())["tables"]
    for t in rep["tables"]:
        for sec, s in t["sections"].items():
            assert len(val[t["name"]]["sections"][sec]["offending"]) == s["negbin"] and s["nonfinite"] == 0
    assert rep["flagged"] == sum(s["negbin"] for t in rep["tables"] for s in t["sections"].values()) > 0


def test_cli_negative_rows_exit_1_and_still_write(hip, planted, tmp_path, capsys):
    out = tmp_path / "o"
    assert run_cli([planted, out, "--bins", "128", "--json", tmp_path / "r.json"]) == derive.EXIT_FLAGGED
    assert "--repair-positivity" in capsys.readouterr().err
    rep = json.loads((tmp_path / "r.json").read_text())
    assert rep["tables"][0]["sections"]["elastic"]["negbin"] >= 1 and rep["flagged"] >= 1
    t = compare.read_library(out)["92238.71c"][1]
    assert t.moments == 128 and t.elastic.mat[3].min() < 0.0


def test_cli_refusals_write_nothing(hip, tmp_path, capsys):
    src = GOLD / "chi_sab"
    e = next(iter(compare.read_library(src).values()))[1].e_bins
    out = tmp_path / "o"
    tab = tmp_path / "tab"
    assert run_cli([src, tab, "--bins", "32"]) == derive.EXIT_FLAGGED      # (negative rows: written all the same)
    cases = [[src, out, "--groups", exact(e[0]), "1.0e-3", exact(e[7])],          # not an edge of the library
             [src, out, "--groups", exact(e[1]), exact(e[7])],                      # another first edge
             [tab, out, "--bins", "5"],                                             # 5 does not divide 32
             [src, out, "--moments", "7"],                                          # 6 are stored
             [src, out, "--bins", "129"], [src, out, "--bins", "x"],
             [src, out, "--bins", "4", "--moments", "2"],
             [src, out],                                                            # no request
             [tmp_path / "nowhere", out, "--bins", "4"],
             [src, src, "--bins", "4"]]                                             # DIR_OUT is DIR_IN
    before = sorted(p.name for p in src.iterdir())
    for args in cases:
        assert run_cli(args) == derive.EXIT_INPUT, args
        assert "input error" in capsys.readouterr().err
        assert not out.exists()
    assert sorted(p.name for p in src.iterdir()) == before


def test_cli_library_error_is_exit_3(hip, tmp_path):
    def broken(*args):
        raise hip.NdppError(hip.NDPP_EDEVICE, "derive_bins: no device")
    out = tmp_path / "o"
    assert run_cli([GOLD, out, "--bins", "4"], dict(NK, bins=broken)) == derive.EXIT_LIBRARY
    assert not out.exists()
