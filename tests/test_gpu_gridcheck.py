"""GPU: ndpp_grid_error against its host restatement bit for bit, ndpp_scatt_library_at against
the rows ndpp_scatt_library integrated on its own grids bit for bit (whole grids and a strict
subset), and the driver's --check-grid / --refine-grid end to end on the U-238-like run directory."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from synth import library_nuclide, u238_case
from test_e2e_reference import write_case2
from test_run_inputs import case1, drive as drive_out, listing

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

# The worst interpolation error --check-grid reports on the unrefined case1 library, measured on an
# MI355X (profiles/gridcheck/README.md); the refinement test runs at an eighth of it, so that
# refinement has to act (about two passes where the error falls as h^2) and ends in test time.
W0 = 0.3657825907084588
TOL = W0 / 8.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("L,G,n", [(6, 2, 1000), (11, 70, 5000), (1, 1, 2)])
def test_gpu_grid_error_equals_the_host_restatement_bit_for_bit(hip, L, G, n):
    from ndpp_amd import gridcheck
    rng = np.random.default_rng(1000 * L + G)
    x = 1e-11 * np.exp(np.cumsum(rng.uniform(1e-5, 56.0 / n, n)))      # 1e-11 MeV up to about 20 MeV
    y = rng.uniform(0.0, 1.0, (n, G, L)) * 10.0 ** rng.integers(-14, 1, (n, G, L))
    y[:, :, 1:] *= rng.choice([-1.0, 1.0], (n, G, max(L - 1, 0)))
    xm = gridcheck.midpoints(x)
    ym = 0.5 * (y[:-1] + y[1:]) + 1e-3 * rng.standard_normal((n - 1, G, L)) * np.abs(y[:-1])
    if n > 100:
        y[10:13] = 0.0                          # zero rows: intervals with scale 0 on both, on one side
        ym[10:12] = 0.0
        ym[11, G - 1, L - 1] = 1.0              # zero scale with a non-zero higher element (L > 1)
        ym[40, G // 2, 0] = np.nan              # a NaN
        y[60, 0, L - 1] = np.inf                # an infinity: two intervals
        x[80] = x[79]                           # a duplicate abscissa
        xm[79] = x[79]
        xm[90] = x[91]                          # a midpoint on the edge
        y[100] = y[101] = ym[100] = 0.25        # exact ties: the lowest index wins
        ym[100, G - 1, L - 1] = 0.5
        ym[100, 0, 0] = 0.0
    want_e, want_a = gridcheck.grid_error_numpy(x, y, xm, ym)
    got_e, got_a = hip.grid_error(x, y, xm, ym)
    print(f"grid_error L={L} G={G} n={n}: max finite err {np.nanmax(np.where(np.isfinite(got_e), got_e, 0)):.3e}, "
          f"skipped {(got_e < 0).sum()}, infinite {np.isinf(got_e).sum()}, "
          f"bit differences {(bits(got_e) != bits(want_e)).sum()}, arg differences {(got_a != want_a).sum()}")
    assert np.array_equal(bits(got_e), bits(want_e)) and np.array_equal(got_a, want_a)
    if n > 100:
        assert got_e[79] == -1.0 and got_e[90] == -1.0 and got_e[10] == 0.0 and got_e[11] == 0.0
        assert np.isinf(got_e[40]) and np.isinf(got_e[59]) and np.isinf(got_e[60])
        assert got_a[100] == 0 and (got_e >= 0).sum() > n - 10


def params_for(hip, c, mu_its=None):
    p = hip.Params.default(c["order"] + 1, c["mu_bins"])
    p.extend_pts, p.inel_extend_pts = c["extend_pts"], c["inel_extend_pts"]
    if mu_its is not None:
        p.adaptive_mu_its = mu_its
    return p


def at_cases():
    h1 = library_nuclide(0.999167, seed=11, n_grid=60, order=5, mu_bins=513, extend_pts=10, inel_extend_pts=5,
                         freegas_cutoff_kT=400.0)
    u = u238_case(n_grid=60, n_levels=5, n_el_rows=25, groups=2, order=5, mu_bins=513, freegas_cutoff_kT=4.0,
                  extend_pts=10, inel_extend_pts=5)
    return h1, u


@pytest.mark.parametrize("nuscatt,mu_its", [(True, None), (False, None), (True, 10)])
def test_gpu_scatt_library_at_on_the_built_grids_gives_the_same_bits(hip, nuscatt, mu_its):
    """mu_its 10: a tunable set outside the box where the Gauss stage runs (test_gpu_tunables)"""
    h1, u = at_cases()
    p = params_for(hip, u, mu_its)
    built = hip.scatt_library(p, [h1, u], u["bins"], nuscatt)
    assert built[0]["ein_inel"] is None and built[1]["ein_inel"] is not None
    assert (built[1]["nuinel_mat"] is not None) == nuscatt
    at = hip.scatt_library_at(p, [h1, u], u["bins"], [b["ein_el"] for b in built], [b["ein_inel"] for b in built], nuscatt)
    for k, (a, b) in enumerate(zip(at, built)):
        for key in ("ein_el", "el_mat", "ein_inel", "inel_mat", "nuinel_mat"):
            same = (a[key] is None and b[key] is None) or np.array_equal(bits(a[key]), bits(b[key]))
            print(f"nuclide {k} {key}: identical {same}")
            assert same, (k, key)
    # a strict subset of the energies (every third elastic, every second inelastic, the top copy point left out;
    # the U-238-like nuclide first): the corresponding rows, whatever else is in the batch
    sub_el = [b["ein_el"][:-1][1::3] for b in built]
    sub_in = [None, built[1]["ein_inel"][:-1][::2]]
    at = hip.scatt_library_at(p, [u, h1], u["bins"], sub_el[::-1], sub_in[::-1], nuscatt)[::-1]
    for k, (a, b) in enumerate(zip(at, built)):
        assert np.array_equal(a["ein_el"], sub_el[k])
        assert np.array_equal(bits(a["el_mat"]), bits(b["el_mat"][:-1][1::3])), k
    assert at[0]["ein_inel"] is None and at[0]["inel_mat"] is None
    assert np.array_equal(bits(at[1]["inel_mat"]), bits(built[1]["inel_mat"][:-1][::2]))
    if nuscatt:
        assert np.array_equal(bits(at[1]["nuinel_mat"]), bits(built[1]["nuinel_mat"][:-1][::2]))
    # an energy above the top group edge is the copy of the row before it; an empty elastic list is an empty section
    top = hip.scatt_library_at(p, [u], u["bins"], [built[1]["ein_el"][-3:]], [None], nuscatt)[0]
    assert np.array_equal(bits(top["el_mat"]), bits(built[1]["el_mat"][-3:])) and np.array_equal(top["el_mat"][-1], top["el_mat"][-2])
    none = hip.scatt_library_at(p, [u], u["bins"], [None], [built[1]["ein_inel"][:4]], nuscatt)[0]
    assert none["el_mat"].shape[0] == 0 and np.array_equal(bits(none["inel_mat"]), bits(built[1]["inel_mat"][:4]))


def drive(run, *extra):
    """test_run_inputs.drive (a child process under its time limit), its output shown"""
    rc, out = drive_out(run, *extra)
    print(out[-6000:])
    return rc


def files_of(run, rename_to=None):
    """what the driver wrote: the tables' library files and ndpp_lib.xml (which names the run
    directory: rename_to puts another run's name there, for a comparison)"""
    out = {n: (Path(run) / n).read_bytes() for n in listing(run)
           if n.endswith((".g2", ".g7")) or n == "ndpp_lib.xml"}
    if rename_to is not None:
        out["ndpp_lib.xml"] = out["ndpp_lib.xml"].replace(str(Path(run).resolve()).encode(),
                                                          str(Path(rename_to).resolve()).encode())
    return out


def test_gpu_thermal_tables_are_checked_not_refined(hip, tmp_path):
    """The four-table run directory (a fissionable neutron table and three thermal tables): --check-grid
    writes a plain run's bytes and reports every thermal table through sab_batch on its midpoints;
    --refine-grid leaves the thermal files as they are; and the rows the check integrates -- the midpoints
    with the grid's top point appended as a sentinel and dropped, because sab_batch's last row is the copy
    of its neighbour -- are the rows sab_batch gives where those midpoints are interior points of a grid."""
    from ndpp_amd import gridcheck, run as drv
    plain, chk, ref = tmp_path / "plain", tmp_path / "check", tmp_path / "refine"
    for d in (plain, chk, ref):
        write_case2(d)
    assert drive(plain) == 0
    assert drive(chk, "--check-grid", "--json", str(tmp_path / "check.json")) == 0
    a = files_of(plain)
    assert len(a) == 5 and a == files_of(chk, rename_to=plain)
    s = drv.read_ndpp_xml(plain)
    tables = drv.load_tables(s, drv.read_cross_sections(s["cross_sections"]))
    p, bins = drv.params_of(s), s["energy_bins"]
    rep = json.loads((tmp_path / "check.json").read_text())["grid"]["check"]["tables"]
    assert [r["kind"] for r in rep] == ["neutron", "thermal", "thermal", "thermal"]
    assert set(rep[0]["sections"]) == {"elastic"} and "note" not in rep[0]
    for k in (1, 2, 3):
        d = tables[k]["data"]
        ein = hip.add_one_more_point(hip.sab_egrid_lib(p, d, bins))
        sec = rep[k]["sections"]
        assert set(sec) == {"elastic"} and rep[k]["note"] == "thermal table: checked, not refined" and rep[k]["breakpoints"] == []
        e = sec["elastic"]
        print(f"{rep[k]['name']}: {e['intervals']} intervals, worst {e['worst']:.3e} in {e['interval']}, above {e['above']}")
        assert e["intervals"] == len(ein) - 2 and e["skipped"] == 0            # all but the copied top point
        assert e["worst"] is not None and 0.0 <= e["worst"] < np.inf
        # the sentinel: the evaluator's rows at the midpoints == sab_batch's rows where they are interior points
        mids = gridcheck.midpoints(ein)[:-1]
        got = gridcheck.library_evaluator(p, bins, tables, s["nuscatter"], {(k, "sab"): ein[-1]})({(k, "sab"): mids})
        both = np.sort(np.concatenate([ein, mids]))
        want = hip.sab_batch(p, d, both, bins)[np.searchsorted(both, mids)]
        assert np.array_equal(bits(got[(k, "sab")]["elastic"]), bits(want)), rep[k]["name"]
        # ... and the last row of a plain call on the midpoints alone IS a copy, which is why the sentinel is there
        alone = hip.sab_batch(p, d, mids, bins)
        assert np.array_equal(alone[-1], alone[-2]) and np.array_equal(bits(alone[:-1]), bits(want[:-1]))
    assert drive(ref, "--refine-grid", "1e-2", "--check-grid", "--json", str(tmp_path / "refine.json")) == 0
    b = files_of(ref, rename_to=plain)
    for name in a:
        if name.endswith("t.g7"):
            assert a[name] == b[name], name                                       # thermal files: untouched
    g = json.loads((tmp_path / "refine.json").read_text())["grid"]
    assert [t["kind"] for t in g["refine"]["tables"]] == ["neutron", "thermal", "thermal", "thermal"]
    assert all(t["grids"] == {} and t["note"] == "thermal table: checked, not refined" for t in g["refine"]["tables"][1:])
    # (the counts above tol differ: this run counts against 1e-2; the errors themselves are the same)
    key = lambda t: [(t["sections"]["elastic"][k]) for k in ("worst", "interval", "group", "order", "intervals", "skipped")]
    assert [key(t) for t in g["check"]["tables"][1:]] == [key(r) for r in rep[1:]]


def test_gpu_check_then_refine_end_to_end(hip, tmp_path):
    """case1 (the U-238-like table of the end-to-end golden): a plain run and a --check-grid run write the
    same bytes; --refine-grid TOL acts, and the check of the refined grids that follows it in the same run
    finds every interval at or below TOL but the ones the refine report lists as unresolved, and those sit
    on breakpoints.  That check integrates the midpoints the last refinement pass integrated, all in one
    batch instead of pass by pass: it is a consistency check of the bookkeeping (insertion, interval
    tracking, report), not new evidence about the error metric -- that is pinned by the bit-for-bit
    comparison with the host restatement above and by its analytic cases in test_gridcheck.py."""
    from ndpp_amd import reader, run as drv
    assert TOL > 0.0
    plain, chk, ref = (case1(tmp_path / n) for n in ("plain", "check", "refine"))
    assert drive(plain) == 0
    assert drive(chk, "--check-grid", "--json", str(tmp_path / "check.json")) == 0
    a = files_of(plain)
    assert len(a) == 2 and a == files_of(chk, rename_to=plain)
    rep0 = json.loads((tmp_path / "check.json").read_text())["grid"]["check"]["tables"]
    assert len(rep0) == 1 and set(rep0[0]["sections"]) == {"elastic", "inelastic", "nu-inelastic"}
    w0 = max(s["worst"] for s in rep0[0]["sections"].values())
    print(f"unrefined case1: worst error {w0:.6e} (W0 of this file {W0:.6e}); per section "
          + ", ".join(f"{k} {s['worst']:.3e}" for k, s in rep0[0]["sections"].items()))
    assert all(s["skipped"] == 0 for s in rep0[0]["sections"].values())
    assert W0 / 1.5 < w0 < W0 * 1.5          # TOL below is still "about an eighth of the worst error"

    assert drive(ref, "--refine-grid", repr(TOL), "--check-grid", "--json", str(tmp_path / "refine.json")) == 0
    g = json.loads((tmp_path / "refine.json").read_text())["grid"]
    rr, cc = g["refine"]["tables"][0], g["check"]["tables"][0]
    n_bp = len(rr["breakpoints"])
    assert n_bp >= 1 and sum(gr["added"] for gr in rr["grids"].values()) > 0      # refinement acted
    unresolved = {"elastic": [], "inelastic": [], "nu-inelastic": []}
    for name, gr in rr["grids"].items():
        print(f"refine {name}: {gr['points_before']} -> {gr['points_after']} in {gr['passes']} passes, stopped "
              f"{gr['stopped']}, unresolved {[(u['section'], u['interval'], u['err']) for u in gr['unresolved']]}")
        assert gr["stopped"] in ("converged", "max_passes") and gr["skipped"] == 0
        assert len(gr["unresolved"]) <= n_bp
        for u in gr["unresolved"]:
            assert u["at_breakpoint"] and u["reason"] == "max_passes", u
            # an interval of the inelastic grid counts for both of its sections
            for sec in ((u["section"],) if name == "elastic" else ("inelastic", "nu-inelastic")):
                unresolved[sec].append(u["interval"])
    for name, s in cc["sections"].items():
        print(f"check of the refined grid, {name}: worst {s['worst']:.3e}, above {s['above']} of {s['intervals']}")
        assert s["skipped"] == 0
        for iv in s["above_intervals"]:
            assert iv in unresolved[name], (name, iv)

    # the refined library reads back, validates, keeps every original energy, and -- through the library, before
    # print_tol and thinning -- every original row bit for bit
    t0 = reader.read_binary(next(v for k, v in a.items() if k.endswith(".g2")))
    t1 = reader.read_binary(next(v for k, v in files_of(ref).items() if k.endswith(".g2")))
    for s0, s1 in ((t0.elastic, t1.elastic), (t0.inelastic, t1.inelastic), (t0.nuinelastic, t1.nuinelastic)):
        assert np.all(np.diff(s1.ein) > 0) and np.isin(s0.ein, s1.ein).all() and len(s1.ein) >= len(s0.ein)
        assert np.array_equal(hip.group_index(drv.read_ndpp_xml(ref)["energy_bins"], s1.ein), s1.group_index)
    # validate reads both libraries; its verdict on positivity (a property of the truncated P5 expansion of this
    # table, free-gas rows near the thermal edge) is the same for the refined library as for the plain one
    codes = []
    for d in (plain, ref):
        r = subprocess.run([sys.executable, "-m", "ndpp_amd.validate", str(d)], cwd=ROOT, capture_output=True, text=True,
                           timeout=200)
        print(r.stdout[-1500:], r.stderr[-1500:])
        assert r.returncode in (0, 1) and "1 tables" in r.stdout
        codes.append(r.returncode)
    assert codes[0] == codes[1]
    s = drv.read_ndpp_xml(ref)
    tables = drv.load_tables(s, drv.read_cross_sections(s["cross_sections"]))
    p, bins = drv.params_of(s), s["energy_bins"]
    from ndpp_amd import gridcheck
    res = hip.scatt_library(p, [tables[0]["data"]], bins, s["nuscatter"])
    new, _ = gridcheck.refine(p, bins, tables, res, s["nuscatter"], TOL)
    for x, m in (("ein_el", "el_mat"), ("ein_inel", "inel_mat"), ("ein_inel", "nuinel_mat")):
        at = np.searchsorted(new[0][x], res[0][x])
        assert np.array_equal(new[0][x][at], res[0][x])
        assert np.array_equal(bits(new[0][m][at]), bits(res[0][m]))
    assert len(new[0]["ein_el"]) == len(t1.elastic.ein) and len(new[0]["ein_inel"]) == len(t1.inelastic.ein)
