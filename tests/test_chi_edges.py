"""The chi kernel against the Fortran across laws, TAB1 schemes and table edges: the cases of
synth.chi_edge_cases(), their goldens from calc_chi (tests/golden/chi_edges.npz, written by
`make_golden.py chi_edges`), the C oracle and the gfx950 kernel.

Each case exists for one condition, stated in its `why`; test_case_condition computes that
condition from the case's inputs alone, so that an edit of the generator cannot empty a case
unnoticed.

What the goldens showed about the reference (not a difference between the three codes):
an interior duplicated pair of nuclide energies never reaches `energy(j) == energy(j+1)`
(chidata_header.F90:197).  binary_search (search.F90:21-71) ends with energy(L) <= Ein <
energy(R), R = L + 1; with Ein on a pair (p, p+1) that leaves L = p + 1, the interval above the
pair, and an Ein off the pair cannot land in an empty interval.  So `dup_energy` has no NaN row
(f is never 0/0), in the Fortran, the oracle and the kernel alike.  The step is reached with
j = 1 from `Ein < energy(1)` when the FIRST two energies are equal -- the case `dup_leading` --
and with j = n_grid - 1 when the LAST two are, which reads out of bounds in the reference and
is refused by ndpp_chi_batch (test_chi_batch_refuses_before_the_device)."""
import ctypes as C

import numpy as np
import pytest

from conftest import dp, load_golden
from synth import chi_case, chi_edge_cases, chi_spectrum_grid, chi_union_grid, law4_table_rows, tab1_parse
from test_chi import run_oracle

CASES = chi_edge_cases()
NAMES = list(CASES)
NAN_CASES = ("overflow",)            # the only case whose golden holds NaN (see the module docstring)
KEYS = ("chi_t", "chi_p", "chi_d")


@pytest.fixture(scope="module")
def golden():
    return load_golden("chi_edges")


def _gold(golden, name):
    return [golden[f"{name}_{k}"] for k in KEYS]


# ---- the inputs -------------------------------------------------------------------------------------
def _entries(c):
    return list(c["spectra"]) + list(c["delayed"])


def _law4_x(data, e):
    """(row interval, x) of chidata_header.F90:282-292 for incoming energy e"""
    g = chi_spectrum_grid(data)
    if e < g[0]:
        return 1, 0.0
    if e >= g[-1]:
        return len(g) - 1, 1.0
    i = int(np.searchsorted(g, e, side="right"))
    return i, (e - g[i - 1]) / (g[i] - g[i - 1])


def _is_hist(law, data):
    return law == 4 and int(data[0]) == 1 and data[2] == 1


def _tab1_blocks(c):
    """name -> (TAB1 block, U or None) of everything chi_tab1 interpolates in a case"""
    out = {}
    for k, e in enumerate(_entries(c)):
        law, d = e[0], np.asarray(e[1])
        if law in (7, 9):
            out[f"T{law}_{k}"] = (d, d[-1])
        elif law == 11:
            n = 2 + 2 * int(d[0]) + 2 * int(d[1 + 2 * int(d[0])])
            out[f"a_{k}"], out[f"b_{k}"] = (d, d[-1]), (d[n:], d[-1])
    if c["nu_t_type"] == 2:
        out["nu_t"] = (c["nu_t_data"], None)
    if c["nu_d_type"] == 2:
        out["nu_d"] = (c["nu_d_data"], None)
    lc = 1
    for j in range(c["n_prec"]):
        blk = c["prec_data"][lc:]
        out[f"yield_{j}"] = (blk, None)
        lc += 2 + 2 * int(blk[0]) + 2 * int(blk[1 + 2 * int(blk[0])]) + 1
    return out


def _regions_hit(nbt, x, pts):
    """the regions (0-based) that have one of pts strictly inside one of their bins"""
    hit = set()
    for e in pts:
        i = int(np.searchsorted(x, e, side="right"))            # 1-based bin: x(i) <= e < x(i+1)
        if 1 <= i < len(x) and x[i - 1] < e < x[i]:
            hit.add(next(j for j, b in enumerate(nbt) if i < b) if len(nbt) else 0)
    return hit


def _tab1_lin(block, e):
    """a TAB1 block with NR = 0 or one region of scheme 1 or 2, at e (enough for the checks here)"""
    nbt, ints, x, y = tab1_parse(block)
    scheme = int(ints[0]) if len(ints) else 2
    assert len(ints) <= 1 and scheme in (1, 2)
    if e < x[0]:
        return y[0]
    if e > x[-1]:
        return y[-1]
    i = min(int(np.searchsorted(x, e, side="right")), len(x) - 1)
    return y[i - 1] if scheme == 1 else np.interp(e, x, y)


def _cond_arith_only(c, u):
    assert {e[0] for e in _entries(c)} == {4, 61}
    assert any(_is_hist(e[0], e[1]) for e in _entries(c))
    l61 = [e[1] for e in _entries(c) if e[0] == 61 and int(e[1][0]) == 1 and e[1][2] == 1]
    assert l61 and any(0.5 < _law4_x(l61[0], e)[1] < 1.0 for e in u)       # where a histogram would pick another row
    assert c["nu_t_type"] == 1 and all(int(b[0]) == 0 for b, _ in _tab1_blocks(c).values())


def _cond_tab1_schemes(c, u):
    blocks = _tab1_blocks(c)
    kinds = {k.split("_")[0] for k in blocks}
    assert {"T7", "T9", "a", "b", "nu", "yield"} <= kinds and {"nu_t", "nu_d"} <= set(blocks)
    one, three = [], []
    for name, (blk, U) in blocks.items():
        nbt, ints, x, y = tab1_parse(blk)
        assert len(nbt) == 0 or nbt[-1] == len(x), name
        if any(s in (3, 5) for s in ints):
            assert (x > 0).all(), name
        if any(s in (4, 5) for s in ints):
            assert (y > 0).all(), name
        pts = u if not name.startswith(("a_", "b_")) else u[u - U > 0]      # law 11 returns before a, b matter
        assert _regions_hit(nbt, x, pts) == set(range(max(len(nbt), 1))), name
        if len(nbt) == 1:
            one.append(int(ints[0]))
        if len(nbt) == 3:
            three.append((len(x), len(set(ints))))
    assert any(int(b[0]) == 0 for b, _ in blocks.values())
    assert sorted(one) == [1, 2, 3, 4, 5]
    assert len(three) >= 2 and all(n >= 7 and k >= 2 for n, k in three)


def _cond_thresholds(c, u):
    bins = c["bins"]
    laws = set()
    for e in _entries(c):
        law, d = e[0], np.asarray(e[1])
        if law not in (7, 9, 11):
            continue
        laws.add(law)
        U = d[-1]
        assert U > 0 and u[0] < U < u[-1]
        above = u[u - U > 0]
        assert (u - U <= 0).sum() >= 2 and len(above) >= 3
        Tmax = tab1_parse(d)[3].max()
        assert (above - U >= 1e-3 * Tmax).all()                  # away from the cancelling I (see the issue's note)
        assert bins[1:].min() < U < bins.max()
        assert any(bins[1:].min() < E - U < bins.max() for E in above)
    assert laws == {7, 9, 11}
    assert all(t > 1 for t in c["thr"]) and 18 in c["mts"]
    split = [t for t in c["thr"] if u[0] < c["energy"][t - 1] < u[-1]]
    assert len(split) >= 3                                       # union energies on both sides of three thresholds


def _cond_nearest_row(c, u):
    (l1, d1), (l2, d2) = [e[:2] for e in c["spectra"]]
    assert l1 == 4 and l2 == 4 and not _is_hist(l1, d1) and _is_hist(l2, d2)
    xs = np.array([_law4_x(d1, e)[1] for e in u])
    assert (xs == 0.5).any() and ((xs > 0.5 - 1e-9) & (xs < 0.5)).any() and ((xs > 0.5) & (xs < 0.5 + 1e-9)).any()
    i = _law4_x(d1, u[xs == 0.5][0])[0]
    rows = law4_table_rows(d1)
    lo, hi = (np.interp(c["bins"][1:], r[1], r[2]) for r in (rows[i - 1], rows[i]))
    assert np.abs(np.diff(np.concatenate([[0.0], lo])) - np.diff(np.concatenate([[0.0], hi]))).max() > 1e-3
    assert any(0.5 < _law4_x(d2, e)[1] < 1.0 for e in u)


def _cond_eout_edges(c, u):
    bins = c["bins"]
    rows = law4_table_rows(c["spectra"][0][1])
    assert any(r[1][0] > bins[2] for r in rows) and any(r[1][-1] < bins[-1] for r in rows)
    assert any(len(r[1]) == 2 for r in rows)
    assert any(np.isin(bins[1:-1], r[1]).any() for r in rows)
    assert u[0] < c["energy"][0]


def _cond_groups(c, u, G):
    assert len(c["bins"]) - 1 == G and c["nnest"] == [2] and c["n_prec"] == 1
    other = CASES["groups_70" if G == 1 else "groups_1"]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(_entries(c), _entries(other)))
    assert np.array_equal(c["fission"], other["fission"])
    if G == 70:
        r = c["bins"][2:] / c["bins"][1:-1]
        assert np.allclose(r[:-1], r[0], rtol=1e-12)             # log-spaced


def _cond_many_energies(c, u):
    assert 130 <= len(u) <= 140 and len(c["bins"]) - 1 == 2
    assert any(e[0] == 4 and len(chi_spectrum_grid(e[1])) >= 40 for e in c["spectra"])
    assert sum(e[0] in (7, 9) for e in _entries(c)) >= 3


def _cond_dup_energy(c, u):
    e = c["energy"]
    k = np.flatnonzero(e[1:] == e[:-1])
    assert len(k) == 1 and 0 < k[0] < len(e) - 2
    a = e[k[0]]
    assert {np.nextafter(a, -np.inf), a, np.nextafter(a, np.inf)} <= set(u)


def _cond_dup_leading(c, u):
    e = c["energy"]
    assert e[0] == e[1] and (np.diff(e[1:]) > 0).all()
    assert (u < e[0]).sum() >= 2 and 2 in c["thr"]


def _cond_overflow(c, u):
    law, d = c["delayed"][0]
    assert law == 7
    T = np.array([_tab1_lin(d, e) for e in u])
    ratio = c["bins"][None, 1:] / T[:, None]
    assert (np.abs(ratio / 709.78 - 1.0) > 0.05).all()           # no libm decides which exp overflows
    over = ratio > 709.78
    assert over[:, -1].any() and not over[:, :-1].any()          # the top edge only
    assert 0 < over.any(axis=1).sum() <= len(u) // 2


def _cond_no_delayed(c, u):
    assert c["nu_d_type"] == 0 and c["n_prec"] == 0 and c["delayed"] == []


def _cond_p_valid(c, u):
    n = c["nnest"][0]
    assert n >= 3
    first, mid, last = c["spectra"][0], c["spectra"][1], c["spectra"][n - 1]
    pv = first[2]
    assert len(pv["pv_nbt"]) == 3 and pv["pv_nbt"][-1] == len(pv["pv_x"]) and len(set(pv["pv_int"])) == 3
    assert _regions_hit(pv["pv_nbt"], np.array(pv["pv_x"]), u) == {0, 1, 2}
    assert len(mid[2]["pv_x"]) > 0 and not mid[2].get("pv_nbt") and any(v != 1.0 for v in mid[2]["pv_y"])
    assert len(last[2]["pv_nbt"]) >= 1 and any(v != 1.0 for v in last[2]["pv_y"])


CONDITIONS = {"arith_only": _cond_arith_only, "tab1_schemes": _cond_tab1_schemes, "thresholds": _cond_thresholds,
              "nearest_row": _cond_nearest_row, "eout_edges": _cond_eout_edges,
              "groups_1": lambda c, u: _cond_groups(c, u, 1), "groups_70": lambda c, u: _cond_groups(c, u, 70),
              "many_energies": _cond_many_energies, "dup_energy": _cond_dup_energy, "dup_leading": _cond_dup_leading,
              "overflow": _cond_overflow, "no_delayed": _cond_no_delayed, "p_valid": _cond_p_valid}


@pytest.mark.parametrize("name", NAMES)
def test_case_condition(name):
    """The condition each case exists for, from its inputs; and the limits every case keeps."""
    c = CASES[name]
    u = chi_union_grid(c)
    assert c["why"] and set(CONDITIONS) == set(NAMES)
    assert len(u) <= 140 and len(c["bins"]) - 1 <= 70
    for e in _entries(c):                 # staggered grids: every table is met at interior points, not only at nodes
        if len(_entries(c)) > 1 and len(chi_spectrum_grid(e[1])) > 2:
            g = chi_spectrum_grid(e[1])
            assert len(np.setdiff1d(u[(u > g[0]) & (u < g[-1])], g)) > 0
    CONDITIONS[name](c, u)


@pytest.mark.parametrize("name", NAMES)
def test_arith_marker(name):
    """`arith` marks exactly the cases in which nothing reaches exp / log / erf / sinh: laws 4 and 61
    only, and every TAB1 block (nu_t, nu_d, yields, an applied p_valid) lin-lin or histogram."""
    c = CASES[name]
    free = {e[0] for e in _entries(c)} <= {4, 61}
    free = free and all(set(tab1_parse(b)[1]) <= {1, 2} for b, _ in _tab1_blocks(c).values())
    free = free and all(set((e[2] or {}).get("pv_int") or []) <= {1, 2} for e in c["spectra"] if len(e) > 2)
    assert c["arith"] == free
    assert CASES["arith_only"]["arith"]


# ---- the oracle and the host grid against the Fortran (CPU) ---------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_chi_edges_oracle_vs_golden(oracle, hip, golden, name):
    """Bit for bit, NaN pattern included, as test_chi_egrid_and_oracle_vs_golden demands of chi_case.
    Measured: every case equal in every bit, the transcendental ones too (gcc and flang call the
    same libm here), so no 1e-13 allowance is made."""
    c = CASES[name]
    grid = golden[f"{name}_e_grid"]
    assert np.array_equal(hip.chi_egrid_lib(c), grid)          # the union-grid host code
    assert np.array_equal(chi_union_grid(c), grid)
    ref = _gold(golden, name)
    got = run_oracle(oracle, hip, c, grid)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(a, b, equal_nan=True)
    ct, cp, cd = ref
    finite = ~np.isnan(ct).any(axis=1)
    if name in NAN_CASES:
        assert (~finite).any() and 2 * finite.sum() >= len(grid)
    else:
        assert not any(np.isnan(a).any() for a in ref)
    assert not np.isnan(cp).any()
    assert np.abs(ct[finite].sum(axis=1) - 1.0).max() < 1e-13 and np.abs(cp.sum(axis=1) - 1.0).max() < 1e-13


@pytest.fixture(scope="module")
def ref_chi(ref, tmp_path_factory):
    """The reference build with the shim's ref_calc_chi_pv.  conftest's `ref` builds only when no
    library is there, so one built from an older shim loads and lacks the entry.  Then `make ref`
    is run as conftest runs it -- a build that fails raises, and fails the test -- and the new
    library is loaded from a copy (the linker replaces the file; the old one stays mapped under its
    name for the rest of the session)."""
    if hasattr(ref, "ref_calc_chi_pv"):
        return ref
    import shutil
    from conftest import REF_SO, ROOT, _make
    _make(ROOT / "oracle", "ref")
    fresh = tmp_path_factory.mktemp("ref") / "libndpp_ref_fresh.so"
    shutil.copy(REF_SO, fresh)
    return C.CDLL(str(fresh))


def test_chi_edges_golden_is_what_the_reference_gives(ref_chi, golden):
    """Where the reference build exists: calc_chi itself on every case (through ref_calc_chi_pv, and
    chi_case through the first entry ref_calc_chi as well) gives the stored goldens bit for bit."""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, str(GOLDEN))
    from make_golden import ref_chi_case
    ref = ref_chi
    for name, c in CASES.items():
        got = ref_chi_case(ref, c, ncap=160)
        for a, k in zip(got, ("e_grid",) + KEYS):
            assert np.array_equal(a, golden[f"{name}_{k}"], equal_nan=True), (name, k)
    old = load_golden("chi")
    for entry in ("ref_calc_chi", "ref_calc_chi_pv"):
        for a, k in zip(ref_chi_case(ref, chi_case(), entry=entry), ("e_grid",) + KEYS):
            assert np.array_equal(a, old[k]), (entry, k)


def test_dup_leading_reaches_the_duplicate_step(oracle, hip, golden):
    """Below the first (duplicated) nuclide energy chi_prob leaves j = 2: the reaction with threshold 2
    contributes there.  With the step dropped its prob would be 0 and chi_p the first reaction's
    spectrum alone."""
    c = CASES["dup_leading"]
    grid = golden["dup_leading_e_grid"]
    alone = dict(c, mts=c["mts"][:1], thr=c["thr"][:1], sig=c["sig"][:1], nnest=c["nnest"][:1],
                 spectra=c["spectra"][:c["nnest"][0]])
    cp = run_oracle(oracle, hip, alone, grid)[1]
    below = grid < c["energy"][0]
    assert below.sum() >= 2
    assert np.abs(cp[below] - golden["dup_leading_chi_p"][below]).max() > 1e-3


# ---- ndpp_chi_batch refuses before it asks for the device (CPU) -----------------------------------
def _batch(hip, c, G=None, patch=None):
    nuc, PA, npr, DA, nd, keep = hip.chi_structs(c)
    if patch:
        patch(nuc, PA, DA)
    bins, grid = np.ascontiguousarray(c["bins"], dtype=np.float64), np.array([1e-6, 1.0])
    G = len(bins) - 1 if G is None else G
    ct, cp, cd = np.zeros((2, 8)), np.zeros((2, 8)), np.zeros((max(nd, 1), 2, 8))
    lib = hip.load()
    rc = lib.ndpp_chi_batch(C.byref(nuc), npr, PA, nd, DA, G, dp(bins), 2, dp(grid), dp(ct), dp(cp), dp(cd))
    del keep
    return rc, lib.ndpp_last_error()


def _with(c, **kw):
    c = dict(c)
    c.update(kw)
    return c


def _spec(c, k, data, where="spectra"):
    s = list(c[where])
    s[k] = (s[k][0], np.asarray(data, dtype=np.float64))
    return _with(c, **{where: s})


def test_chi_batch_refuses_before_the_device(hip):
    """Every malformed input below is -22 with a message naming what is wrong, on a machine with no
    device too; the unchanged case is the device error there.  chi_case(): spectra[0] is law 4
    (NR = 0, NE = 3: locators at words 5..7), spectra[2] law 11."""
    c = chi_case()
    l4, watt = c["spectra"][0][1], c["spectra"][2][1]
    n = c["n_grid"]

    def word(data, k, v):
        d = np.array(data, dtype=np.float64)
        d[k] = v
        return d

    def regions_without_pairs(nuc, PA, DA):
        assert PA[0].has_next == 1
        PA[0].pv_n_regions = 1

    dup_end = c["energy"].copy()
    dup_end[-1] = dup_end[-2]
    bad = [
        ("last two nuclide energies equal", _with(c, energy=dup_end), {}, b"energy grid"),
        ("law 4 with NR = 2", _spec(c, 0, word(l4, 0, 2.0)), {}, b"multiple interpolation regions"),
        ("law-4 locator beyond n_data", _spec(c, 0, word(l4, 5 + 1, len(l4) + 5.0)), {}, b"locator"),
        ("law-4 row with NP = 1", _spec(c, 0, word(l4, int(l4[5]) + 1, 1.0)), {}, b"table of incoming energy 1 truncated"),
        ("Watt data cut before U", _spec(c, 2, watt[:-1]), {}, b"Watt data truncated"),
        ("n_sigma one short", _with(c, sig=[c["sig"][0], c["sig"][1][:-1], c["sig"][2]]), {}, b"sigma has"),
        ("threshold > n_grid", _with(c, thr=[c["thr"][0], n + 1, c["thr"][2]]), {}, b"sigma has"),
        ("nu_t polynomial longer than its words", _with(c, nu_t_data=np.array([5.0, 2.4, 0.12])), {}, b"nu_t polynomial"),
        ("precursor block cut short", _with(c, prec_data=c["prec_data"][:-1]), {}, b"precursor group 3"),
        ("has_next, regions, no pv_x", c, dict(patch=regions_without_pairs), b"p_valid incomplete"),
        ("G = 0", c, dict(G=0), b"G=0"),
    ]
    for what, case, kw, msg in bad:
        rc, err = _batch(hip, case, **kw)
        assert rc == -22 and msg in err, (what, rc, err)
    rc, err = _batch(hip, c)
    if hip.load().ndpp_device_count() == 0:
        assert rc == -5 and b"no HIP device" in err
    else:
        assert rc == 0


# ---- the kernel (GPU) ------------------------------------------------------------------------------
def _dense_grid(c):
    """union-grid midpoints (arithmetic and geometric), a point below the first nuclide energy, one
    below the lowest spectrum energy and one above 20 MeV"""
    u = chi_union_grid(c)
    return np.unique(np.concatenate([u, 0.5 * (u[1:] + u[:-1]), np.sqrt(u[1:] * u[:-1]),
                                     [0.5 * c["energy"][0], 0.5 * u[0], 25.0]]))


def _compare(name, what, got, ref, arith):
    """NaN pattern equal, finite values within the project's 1e-10 absolute (rows are pdfs); the cases
    marked arith bit for bit.  Returns the maximum."""
    worst = 0.0
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        assert np.array_equal(np.isnan(a), np.isnan(b)), (name, what)
        if a.size and not np.isnan(b).all():
            worst = max(worst, float(np.nanmax(np.abs(a - b))))
    print(f"chi_edges {name} ({what}): max abs err {worst:.2e}")
    assert worst < 1e-10
    if arith:
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, ref)), (name, what)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_chi_edges_vs_golden(hip, golden, name):
    """On the Fortran's own union grid.  The kernel is built with the reference's operation order
    and claims to differ only through erf / exp / sinh / log last bits: where none is reached
    (`arith`) every bit must be the Fortran's."""
    c = CASES[name]
    got = hip.chi_batch(c, c["bins"], golden[f"{name}_e_grid"])
    _compare(name, "golden grid", got, _gold(golden, name), c["arith"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_chi_edges_dense_grid_vs_oracle(hip, oracle, name):
    c = CASES[name]
    grid = _dense_grid(c)
    assert (grid < c["energy"][0]).any() and (grid < chi_union_grid(c)[0]).any() and grid[-1] > 20.0
    _compare(name, f"dense grid, {len(grid)} energies", hip.chi_batch(c, c["bins"], grid),
             run_oracle(oracle, hip, c, grid), c["arith"])


@pytest.mark.gpu
def test_gpu_chi_launch_shape(hip):
    """One thread per incoming energy in blocks of 64: 1, 63, 64, 65 and 129 energies (a full block,
    a partial one, two blocks and a tail) as prefixes of one grid, and the grid reversed.  A row
    depends on its energy alone, so each must equal the 129-point run's row bit for bit."""
    c = CASES["many_energies"]
    grid = _dense_grid(c)[::3][:129]
    assert len(grid) == 129
    full = hip.chi_batch(c, c["bins"], grid)
    assert not any(np.isnan(a).any() for a in full) and len({a.tobytes() for a in full[0]}) > 100
    for n in (1, 63, 64, 65, 129):
        part = hip.chi_batch(c, c["bins"], grid[:n])
        assert all(np.array_equal(p, f[..., :n, :]) for p, f in zip(part, full)), n
    rev = hip.chi_batch(c, c["bins"], grid[::-1].copy())
    assert all(np.array_equal(r[..., ::-1, :], f) for r, f in zip(rev, full))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 70])
def test_gpu_chi_groups(hip, oracle, golden, G):
    """One group and seventy, against the Fortran on its grid and against the oracle on the dense one."""
    name = f"groups_{G}"
    c = CASES[name]
    assert len(c["bins"]) - 1 == G
    got = hip.chi_batch(c, c["bins"], golden[f"{name}_e_grid"])
    assert got[0].shape[1] == G
    _compare(name, "golden grid", got, _gold(golden, name), False)
    grid = _dense_grid(c)
    _compare(name, "dense grid", hip.chi_batch(c, c["bins"], grid), run_oracle(oracle, hip, c, grid), False)
    if G == 1:
        assert all(np.array_equal(a, np.ones_like(a)) for a in got)
