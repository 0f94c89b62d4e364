"""Deterministic synthetic tables shaped like the flattened ACE structures
(SURVEY.md 8d): no ACE files exist in the image.  Shared by the golden
generator and the tests (TEST INFRASTRUCTURE)."""
import numpy as np


def mu_grid(M):
    dmu = 2.0 / float(M - 1)
    mu = -1.0 + np.arange(M, dtype=np.float64) * dmu
    mu[-1] = 1.0
    return mu


def kalbach_rows(M, n_rows, np_lo, np_hi, e_lo, e_hi, seed, dup_last=False, intt=2):
    """A law-44-like ScattData: n_rows incoming energies, each with NP outgoing
    energies (Eout starts at 0), a normalised pdf and Kalbach-Mann f(mu) columns
    f = A/(2 sinh A) (cosh(A mu) + R sinh(A mu)), R in [0,0.5], A in [0.5,3]
    (scattdata_header.F90:822-831).  Returns the CSR tables of the C ABI."""
    rng = np.random.default_rng(seed)
    mu = mu_grid(M)
    e_grid = np.logspace(np.log10(e_lo), np.log10(e_hi), n_rows)
    row_ptr = [0]
    eout, pdf, f, intts = [], [], [], []
    for k in range(n_rows):
        NP = int(rng.integers(np_lo, np_hi + 1))
        emax = 0.9 * e_grid[k]
        eo = np.concatenate([[0.0], np.sort(rng.uniform(0.0, emax, NP - 2)), [emax]])
        if dup_last and k % 2 == 1:
            eo[-2] = eo[-1]          # Zr-90-like duplicate end points (:1127-1130)
        p = np.exp(-eo / (0.3 * emax + 1e-30)) * (eo + 0.05 * emax)
        de = np.diff(eo)
        norm = np.sum(0.5 * (p[1:] + p[:-1]) * de)
        p = p / norm
        R = rng.uniform(0.0, 0.5, NP)
        A = rng.uniform(0.5, 3.0, NP)
        cols = 0.5 * A[:, None] / np.sinh(A[:, None]) * (
            np.cosh(A[:, None] * mu[None, :]) + R[:, None] * np.sinh(A[:, None] * mu[None, :]))
        eout.append(eo)
        pdf.append(p)
        f.append(cols)
        intts.append(intt)
        row_ptr.append(row_ptr[-1] + NP)
    return dict(e_grid=e_grid, row_ptr=np.array(row_ptr, dtype=np.int32),
                eout=np.concatenate(eout), pdf=np.concatenate(pdf),
                intt=np.array(intts, dtype=np.int32),
                f=np.ascontiguousarray(np.concatenate(f, axis=0)))


def law9_edata(e_lo, e_hi, n=8, U=0.5):
    """edist%data of an evaporation spectrum (ACE law 9): TAB1 of T(E) with NR=0
    followed by the restriction energy U (scattdata_header.F90:1289-1302)."""
    E = np.logspace(np.log10(e_lo), np.log10(e_hi), n)
    T = 0.2 + 0.1 * np.sqrt(E)
    return np.concatenate([[0.0, float(n)], E, T, [U]])


def sab_table(mode, seed, NEi=24, NEo=16, NMU=8, elastic=None, NEo_range=(10, 30)):
    """A synthetic thermal-scattering table shaped like the ACE data NDPP consumes
    (ace_header.F90:201-235).  mode 0/1: equal/skewed discrete E_out x mu;
    mode 2: continuous E_out pdf with discrete mu, NEo_range[0] .. NEo_range[1] outgoing energies per
    incoming energy ((50, 300)).  elastic: None, "coherent"
    (Bragg edges, exact mode) or "incoherent" (discrete cosines)."""
    rng = np.random.default_rng(seed)
    kT = 2.53e-8
    ei = np.logspace(-11, np.log10(4e-6), NEi)
    sig = 20.0 + 60.0 / (1.0 + ei / 1e-8)
    t = dict(threshold_inelastic=float(ei[-1]), threshold_elastic=0.0, NEi=NEi, NEo=NEo, NMU=NMU,
             mode=mode, ei=ei, sig=sig,
             e_out=np.zeros(1), mu=np.zeros(1), cptr=np.zeros(NEi + 1, dtype=np.int32),
             ce_out=np.zeros(1), cpdf=np.zeros(1), cmu=np.zeros(1),
             el_mode=3, NEe=0, NMUe=0, ee=np.zeros(1), eP=np.zeros(1), emu=np.zeros(1))
    if mode in (0, 1):
        q = (np.arange(NEo) + 0.5) / NEo
        e_out = np.empty((NEi, NEo))
        mu = np.empty((NEi, NEo, NMU))
        for k in range(NEi):
            e_out[k] = np.sort(ei[k] * (0.2 + 1.6 * q) + kT * (-np.log(1 - q)) * 1.5)
            base = np.clip(1.0 - 2.0 * kT / (ei[k] + kT), -0.9, 0.9)
            mu[k] = np.sort(np.clip(base * 0.3 + rng.uniform(-0.95, 0.95, (NEo, NMU)), -1, 1), axis=1)
        t["e_out"], t["mu"] = e_out.ravel(), mu.ravel()
    else:
        ptr, ce, cp, cm = [0], [], [], []
        for k in range(NEi):
            n = int(rng.integers(NEo_range[0], NEo_range[1] + 1))
            emax = 3.0 * ei[k] + 12 * kT
            eo = np.concatenate([[0.0], np.sort(rng.uniform(0, emax, n - 2)), [emax]])
            pdf = (eo + 0.02 * emax) * np.exp(-eo / (ei[k] + 2 * kT))
            pdf /= np.sum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(eo))
            cm.append(np.sort(rng.uniform(-1, 1, (n, NMU)), axis=1))
            ce.append(eo)
            cp.append(pdf)
            ptr.append(ptr[-1] + n)
        t.update(cptr=np.array(ptr, dtype=np.int32), ce_out=np.concatenate(ce),
                 cpdf=np.concatenate(cp), cmu=np.concatenate(cm).ravel())
    if elastic == "coherent":
        ee = np.array([1.8e-9, 4.5e-9, 6.3e-9, 1.1e-8, 2.2e-8, 5.0e-8, 1.2e-7, 4.0e-6])
        t.update(el_mode=4, NEe=len(ee), NMUe=0, ee=ee, eP=np.cumsum(1e-9 * rng.uniform(0.5, 2, len(ee))),
                 threshold_elastic=float(ee[-1]))
    elif elastic == "incoherent":
        ee = np.logspace(-11, np.log10(4e-6), 12)
        NMUe = 6
        t.update(el_mode=3, NEe=len(ee), NMUe=NMUe, ee=ee, eP=5.0 / (1 + ee / 1e-7),
                 emu=np.sort(rng.uniform(-1, 1, (len(ee), NMUe)), axis=1).ravel(),
                 threshold_elastic=float(ee[-1]))
    return t


def sab_ein_grid(t, n=40, seed=3):
    """Test E_in points: inside, at and beyond the table, incl. exact table points."""
    rng = np.random.default_rng(seed)
    e = np.concatenate([10 ** rng.uniform(-11.3, np.log10(t["threshold_inelastic"]), n),
                        t["ei"][[0, 3, -1]], [t["threshold_inelastic"] * 1.5, 5e-12]])
    return np.sort(e)


# ---- fission spectra (chi) ---------------------------------------------------
def law4_block(e_in, np_pts, e_max, seed, hist=False):
    """edist%data of a continuous tabular distribution (ACE law 4): NR, [NBT,INT], NE,
    E_in(NE), L(NE), then per E_in: INTT', NP, E_out(NP), pdf(NP), cdf(NP)
    (layout read at chidata_header.F90:258-350)."""
    rng = np.random.default_rng(seed)
    NE = len(e_in)
    head = ([1.0, float(NE), 1.0] if hist else [0.0]) + [float(NE)] + list(e_in)
    blocks, locs = [], []
    pos = len(head) + NE  # 0-based offset of the first block == its 1-based index - 1
    for k in range(NE):
        eo = np.concatenate([[0.0], np.sort(rng.uniform(0, e_max, np_pts - 2)), [e_max]])
        T = 1.2 + 0.05 * k
        pdf = np.sqrt(eo + 1e-3) * np.exp(-eo / T)
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(eo))])
        pdf, cdf = pdf / cdf[-1], cdf / cdf[-1]
        blk = [2.0, float(np_pts)] + list(eo) + list(pdf) + list(cdf)
        locs.append(float(pos))
        pos += len(blk)
        blocks += blk
    return np.array(head + locs + blocks)


def tab1_block(x, y):
    return [0.0, float(len(x))] + list(x) + list(y)


def chi_case(seed=18):
    """A synthetic fissionable nuclide (SURVEY 8d config 5 shape): three fission
    reactions -- MT 19 with two nested spectra (law 4 then law 7), MT 20 law 11 (Watt),
    MT 21 law 9 -- and 3 delayed precursor groups (law 4, law 4 histogram, law 7)."""
    rng = np.random.default_rng(seed)
    n_grid = 50
    energy = np.logspace(-11, np.log10(20.0), n_grid)
    part = [2.0 / (1 + energy) ** 0.3, 0.6 * np.ones(n_grid), 0.3 * np.ones(n_grid)]
    thr = [1, 36, 42]
    sig = [part[0][thr[0] - 1:], part[1][thr[1] - 1:] * np.linspace(0, 1, n_grid - thr[1] + 1),
           part[2][thr[2] - 1:] * np.linspace(0, 1, n_grid - thr[2] + 1)]
    fission = part[0].copy()
    fission[thr[1] - 1:] += sig[1]
    fission[thr[2] - 1:] += sig[2]
    e3 = [1e-11, 1.0, 20.0]
    spectra = [  # (law, data) in chain order
        (4, law4_block(e3, 12, 15.0, seed)),
        (7, np.array(tab1_block([1e-11, 20.0], [1.30, 1.45]) + [-20.0])),        # T(E), U
        (11, np.array(tab1_block([1e-11, 20.0], [0.95, 1.05]) +                  # Watt a(E)
                      tab1_block([1e-11, 20.0], [2.2, 2.6]) + [3.0])),           # b(E), U
        (9, np.array(tab1_block([5.0, 20.0], [0.5, 0.9]) + [5.5])),
    ]
    nnest = [2, 1, 1]
    delayed = [(4, law4_block([1e-11, 20.0], 8, 3.0, seed + 1)),
               (4, law4_block([1e-11, 20.0], 8, 2.0, seed + 2, hist=True)),
               (7, np.array(tab1_block([1e-11, 20.0], [0.4, 0.45]) + [-20.0]))]
    prec = []
    for j in range(3):
        prec += [0.01 * (j + 1)] + tab1_block([1e-11, 20.0], [0.2 + 0.1 * j, 0.25 + 0.1 * j])
    return dict(n_grid=n_grid, energy=energy, fission=fission,
                nu_t_type=1, nu_t_data=np.array([2.0, 2.4, 0.12]),
                nu_d_type=2, nu_d_data=np.array(tab1_block([1e-11, 4.0, 20.0], [0.016, 0.016, 0.009])),
                n_prec=3, prec_data=np.array(prec), mts=[19, 20, 21], thr=thr, sig=sig,
                nnest=nnest, spectra=spectra, delayed=delayed,
                bins=np.concatenate([[0.0], np.logspace(-3, np.log10(20.0), 7)]))


# ---- chi edge cases (tests/golden/chi_edges.npz) ------------------------------------------------
# Every number below comes from literals, + - * /, sqrt, seeded uniform draws and np.linspace:
# no np.exp / np.log / np.logspace, whose last bits depend on the numpy build, because the
# goldens are compared bit for bit with inputs regenerated on another machine.
def tab1_regions(x, y, nbt=(), ints=()):
    """A TAB1 block with interpolation regions: NR, NBT(NR), INT(NR), NE, x(NE), y(NE).  The last
    NBT is the point count, so that interpolation.F90:84-91 never leaves `interp` unset."""
    assert len(nbt) == len(ints) and len(x) == len(y) and (len(nbt) == 0 or nbt[-1] == len(x))
    return ([float(len(nbt))] + [float(b) for b in nbt] + [float(s) for s in ints] + [float(len(x))] +
            [float(v) for v in x] + [float(v) for v in y])


def tab1_parse(block):
    """(nbt, ints, x, y) of the TAB1 block that starts at block[0]."""
    block = np.asarray(block, dtype=np.float64)
    NR = int(block[0])
    NE = int(block[1 + 2 * NR])
    o = 2 + 2 * NR
    return (block[1:1 + NR].astype(int), block[1 + NR:1 + 2 * NR].astype(int), block[o:o + NE],
            block[o + NE:o + 2 * NE])


def law4_rows(e_in, eouts, widths, scheme=None):
    """law4_block with every row's outgoing grid given: eouts[k] are the E_out points of incoming
    energy k, its pdf is (E + 1e-3) / (1 + E / widths[k])^3, the cdf its trapezoid sums, both
    normalised.  scheme None: NR = 0; else NR = 1, NBT = NE, INT = scheme."""
    NE = len(e_in)
    assert len(eouts) == NE and len(widths) == NE
    head = ([1.0, float(NE), float(scheme)] if scheme is not None else [0.0]) + [float(NE)] + [float(e) for e in e_in]
    blocks, locs = [], []
    pos = len(head) + NE
    for eo, w in zip(eouts, widths):
        eo = np.asarray(eo, dtype=np.float64)
        q = 1.0 + eo / w
        pdf = (eo + 1e-3) / (q * q * q)
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(eo))])
        pdf, cdf = pdf / cdf[-1], cdf / cdf[-1]
        blk = [2.0, float(len(eo))] + list(eo) + list(pdf) + list(cdf)
        locs.append(float(pos))
        pos += len(blk)
        blocks += blk
    return np.array(head + locs + blocks)


def law4_table_rows(data):
    """[(E_in, E_out(NP), cdf(NP))] of a law-4 / law-61 block (for checks on the inputs)."""
    data = np.asarray(data)
    NR = int(data[0])
    NE = int(data[1 + 2 * NR])
    o = 2 + 2 * NR
    rows = []
    for k in range(NE):
        lc = int(data[o + NE + k])
        NP = int(data[lc + 1])
        rows.append((data[o + k], data[lc + 2:lc + 2 + NP], data[lc + 2 + 2 * NP:lc + 2 + 3 * NP]))
    return rows


def _rand_rows(seed, n_rows, n_pts, e_max, w0=0.4, dw=0.9):
    rng = np.random.default_rng(seed)
    eouts = [np.concatenate([[0.0], np.sort(rng.uniform(0, e_max, n_pts - 2)), [e_max]]) for _ in range(n_rows)]
    return eouts, [w0 + dw * k for k in range(n_rows)]


def _law4(e_in, seed, n_pts=9, e_max=15.0, scheme=None, **kw):
    return law4_rows(e_in, *_rand_rows(seed, len(e_in), n_pts, e_max, **kw), scheme=scheme)


def chi_spectrum_grid(data):
    """incoming energies of one spectrum: chi_init, chidata_header.F90:98-108"""
    NR = int(data[0])
    NE = int(data[1 + 2 * NR])
    return np.asarray(data[2 + 2 * NR:2 + 2 * NR + NE], dtype=np.float64)


def chi_union_grid(c):
    """The union of the spectra's incoming grids, the energies calc_chi evaluates at (chi.F90:97-113;
    none of the edge cases has a zero energy or a tail the reference's merge would drop)."""
    return np.unique(np.concatenate([chi_spectrum_grid(e[1]) for e in c["spectra"] + c["delayed"]]))


def _geom(e0, ratio, n, last=None):
    """e0 * ratio^k by repeated multiplication (np.logspace goes through pow), optionally ending at `last`"""
    e = e0 * np.cumprod(np.concatenate([[1.0], np.full(n - 1, float(ratio))]))
    if last is not None:
        assert e[-2] < last
        e[-1] = last
    return e


NUC_E = _geom(1e-11, 1.78, 50, last=20.0)
CHI_BINS7 = np.array([0.0, 1e-3, 5e-3, 0.03, 0.15, 0.75, 4.0, 20.0])
NU_T_POLY = np.array([4.0, 2.4, 0.12, 1e-3, -2e-5])          # NC = 4: E**0 .. E**3


def _chi_assemble(energy, rxns, delayed, yields, bins, why, arith=False, nu_t=(1, NU_T_POLY), nu_d=None):
    """A chi_case()-shaped dict.  rxns: (MT, threshold, amplitude, [spectrum entries]) per fission
    reaction, its sigma amplitude * (1 + 0.2 sqrt(E)) from the threshold on, ramped from 0.1 to 1
    when the threshold is above 1; fission = 0.05 + the sum, so that it is positive everywhere.
    delayed: one spectrum entry per precursor group; yields: its TAB1 yield block.  `why` states the
    condition the case exists for, `arith` that no spectrum or TAB1 block of it reaches
    exp / log / erf / sinh (the kernel must then equal the Fortran bit for bit)."""
    energy = np.asarray(energy, dtype=np.float64)
    n = len(energy)
    shape = 1.0 + 0.2 * np.sqrt(energy)
    fission = np.full(n, 0.05)
    sig, spectra = [], []
    for _, thr, amp, specs in rxns:
        ramp = np.ones(n - thr + 1) if thr == 1 else np.linspace(0.1, 1.0, n - thr + 1)
        s = amp * shape[thr - 1:] * ramp
        fission[thr - 1:] += s
        sig.append(s)
        spectra += list(specs)
    prec = []
    for j, yb in enumerate(yields):
        prec += [0.01 * (j + 1)] + list(yb)
    if nu_d is None:
        nu_d = (2, tab1_block([1e-11, 4.0, 20.0], [0.016, 0.016, 0.009])) if delayed else (0, [0.0])
    assert len(yields) == len(delayed)
    return dict(n_grid=n, energy=energy, fission=fission, nu_t_type=nu_t[0], nu_t_data=np.array(nu_t[1], dtype=np.float64),
                nu_d_type=nu_d[0], nu_d_data=np.array(nu_d[1], dtype=np.float64), n_prec=len(delayed),
                prec_data=np.array(prec if prec else [0.0]), mts=[r[0] for r in rxns], thr=[r[1] for r in rxns],
                sig=sig, nnest=[len(r[3]) for r in rxns], spectra=spectra, delayed=list(delayed),
                bins=np.asarray(bins, dtype=np.float64), why=why, arith=arith)


def _lin_yields(n):
    return [tab1_block([1e-11, 20.0], [0.2 + 0.1 * j, 0.25 + 0.1 * j]) for j in range(n)]


def _arr(*parts):
    return np.array([float(v) for p in parts for v in p])


def _case_arith_only():
    eA, eB, eC = [1e-11, 1e-3, 1.0, 9.0, 20.0], [1e-11, 3e-2, 14.0, 20.0], [1e-11, 2e-6, 0.4, 20.0]
    rxns = [(19, 1, 2.0, [(4, _law4(eA, 401)), (61, _law4(eB, 402, scheme=1))]),   # law 61, NR=1 INT=1: NOT a histogram
            (20, 30, 0.6, [(4, _law4(eC, 403, scheme=1))])]                        # law 4, NR=1 INT=1: histogram
    delayed = [(61, _law4([1e-11, 5e-5, 20.0], 404, n_pts=7, e_max=3.0)),
               (4, _law4([1e-11, 2.0, 20.0], 405, n_pts=7, e_max=2.0, scheme=1))]
    return _chi_assemble(NUC_E, rxns, delayed, _lin_yields(2), CHI_BINS7, arith=True,
                         why="laws 4 and 61 only, a law-4 histogram table, a law-61 table with NR=1 INT=1 that has "
                             "incoming energies at x > 0.5; polynomial nu_t, lin-lin nu_d and yields")


def _case_tab1_schemes():
    T7 = tab1_regions([1e-11, 1e-8, 1e-5, 1e-3, 0.1, 1.0, 5.0, 20.0], [1.3, 1.25, 1.32, 1.4, 1.36, 1.45, 1.5, 1.6],
                      [3, 5, 8], [5, 2, 4])
    T9 = tab1_regions([1e-11, 3e-7, 2e-4, 0.03, 2.0, 20.0], [1.0, 1.1, 1.25, 1.4, 1.7, 2.0], [6], [1])
    Wa = tab1_regions([1e-11, 3.5, 5.0, 8.0, 12.0, 20.0], [0.95, 0.97, 1.0, 1.02, 1.04, 1.05], [6], [3])
    Wb = tab1_regions([1e-11, 4.2, 6.0, 10.0, 20.0], [2.2, 2.3, 2.45, 2.5, 2.6], [5], [4])
    rxns = [(19, 1, 2.0, [(7, _arr(T7, [-20.0]))]), (20, 1, 0.6, [(9, _arr(T9, [-5.0]))]),
            (21, 1, 0.3, [(11, _arr(Wa, Wb, [3.0]))])]
    delayed = [(7, _arr(tab1_block([1e-11, 5e-10, 7e-4, 20.0], [0.4, 0.41, 0.43, 0.45]), [-20.0])),
               (7, _arr(tab1_block([1e-11, 6e-6, 0.5, 20.0], [0.5, 0.52, 0.55, 0.6]), [-20.0])),
               (7, _arr(tab1_block([1e-11, 4e-2, 7.0, 20.0], [0.3, 0.32, 0.33, 0.36]), [-20.0]))]
    yields = [tab1_block([1e-11, 1e-3, 20.0], [0.2, 0.22, 0.25]),
              tab1_regions([1e-11, 1e-5, 1.0, 20.0], [0.3, 0.28, 0.35, 0.31], [4], [2]),
              tab1_regions([1e-11, 1e-9, 1e-6, 1e-4, 0.02, 3.0, 20.0], [0.4, 0.45, 0.42, 0.5, 0.47, 0.44, 0.4],
                           [3, 5, 7], [2, 4, 1])]
    nu_t = (2, tab1_regions([1e-11, 1e-7, 1e-2, 4.0, 20.0], [2.4, 2.41, 2.5, 2.9, 4.8], [5], [5]))
    nu_d = (2, tab1_regions([1e-11, 1e-9, 1e-6, 1e-4, 0.05, 2.5, 9.0, 20.0],
                            [0.016, 0.0162, 0.0158, 0.016, 0.0155, 0.014, 0.011, 0.009], [2, 5, 8], [1, 3, 5]))
    return _chi_assemble(NUC_E, rxns, delayed, yields, CHI_BINS7, nu_t=nu_t, nu_d=nu_d,
                         why="TAB1 blocks with NR=0, NR=1 with INT 1..5 and NR=3 with mixed schemes: T(E) of laws 7 "
                             "and 9, a(E), b(E) of law 11, tabular nu_t, nu_d and the yields; union energies "
                             "strictly inside a bin of every region")


def _case_thresholds():
    T7 = tab1_block([1e-5, 1e-3, 0.2, 0.5, 0.9, 3.0, 20.0], [1.2, 1.22, 1.25, 1.3, 1.33, 1.4, 1.5])
    T9 = tab1_block([1e-5, 0.05, 1.0, 2.0, 2.6, 7.0, 20.0], [0.8, 0.82, 0.9, 1.0, 1.05, 1.2, 1.4])
    Wa = tab1_block([1e-5, 1.7, 3.0, 4.5, 11.0, 20.0], [0.95, 0.96, 0.98, 1.0, 1.03, 1.05])
    Wb = tab1_block([1e-5, 20.0], [2.2, 2.6])
    # law 7 at Ein = 3: Ein - U = 2.5 exactly, a group edge (the clamp's `>` is strict)
    rxns = [(18, 3, 1.0, [(4, _law4([1e-5, 1e-4, 0.01, 6.5, 20.0], 411))]),          # MT 18: sigma is `fission`
            (19, 30, 1.5, [(7, _arr(T7, [0.5]))]), (20, 38, 0.6, [(9, _arr(T9, [2.0]))]),
            (21, 44, 0.3, [(11, _arr(Wa, Wb, [3.0]))])]
    delayed = [(9, _arr(tab1_block([1e-5, 0.6, 1.0, 1.3, 20.0], [0.4, 0.42, 0.44, 0.45, 0.5]), [1.0])),
               (4, _law4([1e-5, 0.3, 20.0], 412, n_pts=7, e_max=3.0))]
    return _chi_assemble(NUC_E, rxns, delayed, _lin_yields(2), [0.0, 1e-3, 0.1, 0.3, 1.0, 2.5, 6.0, 20.0],
                         why="U > 0 inside the grid for laws 7, 9, 11: at least two union energies with Ein - U <= 0 "
                             "and several above per law, group edges on both sides of Ein - U and of U; thresholds "
                             "> 1 with union energies on both sides; one reaction on MT 18")


def _ulps(v, n):
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return float(v)


def _case_nearest_row():
    e1 = [1e-11, 1.0, 3.0, 15.0, 20.0]                                   # x = 0.5 of its row [1, 3] is E = 2
    e2 = [1e-11, _ulps(2.0, -3), _ulps(2.0, -1), 2.0, _ulps(2.0, 1), _ulps(2.0, 3), 20.0]
    eo1, _ = _rand_rows(421, len(e1), 10, 15.0)
    rxns = [(19, 1, 2.0, [(4, law4_rows(e1, eo1, [0.3, 0.6, 2.5, 5.0, 8.0]))]),
            (20, 1, 0.7, [(4, _law4(e2, 422, scheme=1, dw=0.5))])]
    delayed = [(4, _law4([1e-11, 20.0], 423, n_pts=7, e_max=3.0))]
    return _chi_assemble(NUC_E, rxns, delayed, _lin_yields(1), CHI_BINS7, arith=True,
                         why="the nearest-row rule `x > 0.5` of a non-histogram law-4 table at x = 0.5 exactly and "
                             "within a few ulp on either side, rows that differ by more than 1e-3 in a group; the "
                             "second table is a histogram one with an incoming energy at x > 0.5")


def _case_eout_edges():
    bins = [0.0, 1e-3, 0.01, 0.1, 1.0, 5.0, 20.0]
    e1 = [1e-11, 1e-4, 0.5, 6.0, 20.0]
    eouts = [[0.05, 0.3, 1.0, 2.5, 7.0, 12.0],        # starts above two edges, an E_out on an edge, ends below the top
             [0.0, 15.0],                             # NP = 2, ends below the top edge
             [0.0, 0.01, 0.4, 1.0, 3.0, 20.0],        # two E_out on edges, ends on the top edge
             [0.02, 0.5, 2.0, 8.0, 25.0],             # starts above two edges, ends above the top edge
             [0.0, 1.0, 30.0]]
    rxns = [(19, 1, 2.0, [(4, law4_rows(e1, eouts, [0.5, 1.0, 1.5, 2.5, 4.0]))]),
            (20, 20, 0.6, [(4, _law4([1e-11, 3e-3, 2.0, 20.0], 431, e_max=10.0, scheme=1))])]
    delayed = [(4, law4_rows([1e-11, 20.0], [[0.0, 4.0], [0.0, 5.0]], [0.4, 0.5]))]
    return _chi_assemble(_geom(1e-10, 1.94, 40, last=20.0), rxns, delayed, _lin_yields(1), bins, arith=True,
                         why="law-4 rows whose first E_out lies above the lowest two group edges, rows that end "
                             "below the top edge, a row with NP = 2, group edges equal to E_out points; a union "
                             "energy below the first nuclide energy")


def _groups_nuclide(bins, G):
    rxns = [(19, 1, 2.0, [(4, _law4([1e-11, 1e-3, 1.0, 20.0], 441)),
                          (7, _arr(tab1_block([1e-11, 2e-5, 0.3, 20.0], [1.3, 1.32, 1.4, 1.45]), [-20.0]))])]
    delayed = [(4, _law4([1e-11, 0.7, 20.0], 442, n_pts=7, e_max=3.0))]
    return _chi_assemble(NUC_E, rxns, delayed, _lin_yields(1), bins,
                         why=f"G = {G}: one prompt chain (law 4, then law 7) and one precursor group")


def _case_many_energies():
    e4 = _geom(1e-11, 2.06, 40, last=20.0)
    T7 = tab1_block(_geom(1.6e-11, 2.3, 34), np.linspace(1.2, 1.5, 34))          # staggered against e4
    T9 = tab1_block(_geom(2.5e-11, 2.4, 32), np.linspace(1.0, 2.0, 32))
    Td = tab1_block(_geom(4e-11, 2.5, 30), np.linspace(0.4, 0.5, 30))
    rxns = [(19, 1, 2.0, [(4, _law4(e4, 451, n_pts=6, e_max=12.0, dw=0.1))]), (20, 10, 0.6, [(7, _arr(T7, [-20.0]))]),
            (21, 25, 0.3, [(9, _arr(T9, [-5.0]))])]
    return _chi_assemble(NUC_E, rxns, [(7, _arr(Td, [-20.0]))], _lin_yields(1), [0.0, 1.0, 20.0],
                         why="a union grid of at least 130 incoming energies (more than two blocks of 64 threads, the "
                             "last one partial), G = 2")


def _dup_grid(n, k):
    e = _geom(1e-11, 2.65, n, last=20.0)
    e[k + 1] = e[k]
    return e


def _case_dup_energy():
    e = _dup_grid(30, 14)
    a = float(e[14])
    rxns = [(19, 1, 2.0, [(4, _law4([1e-11, _ulps(a, -1), a, _ulps(a, 1), 20.0], 461))]),
            (20, 12, 0.6, [(4, _law4([1e-11, 0.5 * a, 2.0 * a, 20.0], 462, scheme=1))])]
    delayed = [(4, _law4([1e-11, 20.0], 463, n_pts=7, e_max=3.0))]
    return _chi_assemble(e, rxns, delayed, _lin_yields(1), CHI_BINS7, arith=True,
                         why="a nuclide grid with one interior duplicated pair; spectrum energies one ulp below the "
                             "pair, at it and one ulp above it")


def _case_dup_leading():
    e = _geom(1e-9, 2.25, 30, last=20.0)
    e[1] = e[0]
    rxns = [(19, 1, 2.0, [(4, _law4([1e-11, float(e[0]), 1e-3, 20.0], 466))]),
            (20, 2, 0.6, [(4, _law4([1e-10, 0.2, 20.0], 467, scheme=1))])]
    delayed = [(4, _law4([1e-11, 20.0], 468, n_pts=7, e_max=3.0))]
    return _chi_assemble(e, rxns, delayed, _lin_yields(1), CHI_BINS7, arith=True,
                         why="the first two nuclide energies are equal and union energies lie below them: the only "
                             "way an in-range input reaches `energy(j) == energy(j+1)`; a reaction with threshold 2 "
                             "is then above its threshold")


def _case_overflow():
    Td = tab1_regions([1e-11, 1.0, 20.0], [0.02, 0.5, 0.5], [3], [1])      # histogram: T = 0.02 below 1 MeV
    rxns = [(19, 1, 2.0, [(4, _law4([1e-11, 1e-4, 2.0, 5.0, 12.0, 20.0], 471))])]
    delayed = [(7, _arr(Td, [-20.0])), (7, _arr(tab1_block([1e-11, 20.0], [0.4, 0.45]), [-20.0]))]
    return _chi_assemble(NUC_E, rxns, delayed, _lin_yields(2), [0.0, 1e-3, 0.03, 0.15, 0.75, 4.0, 20.0],
                         why="a delayed Maxwell spectrum with T = 0.02 below 1 MeV: exp(Egp1 / T) overflows for the top "
                             "edge only (20 / 0.02 = 1000, next edge 200; 709.78 decides), inf * 0 = NaN in that row")


def _case_no_delayed():
    rxns = [(19, 1, 2.0, [(4, _law4([1e-11, 1e-3, 1.0, 20.0], 481)),
                          (7, _arr(tab1_block([1e-11, 2e-5, 0.3, 20.0], [1.3, 1.32, 1.4, 1.45]), [-20.0]))]),
            (20, 20, 0.6, [(9, _arr(tab1_block([1e-11, 2.0, 4.0, 9.0, 20.0], [0.8, 0.9, 1.0, 1.1, 1.3]), [2.0]))])]
    return _chi_assemble(NUC_E, rxns, [], [], CHI_BINS7, why="nu_d_type = 0 and no precursor group")


def _case_p_valid():
    pv3 = dict(pv_x=[1e-11, 1e-7, 1e-4, 1e-2, 0.5, 4.0, 20.0], pv_y=[0.9, 0.8, 0.85, 0.6, 0.5, 0.3, 0.25],
               pv_nbt=[3, 5, 7], pv_int=[2, 4, 3])
    pv_no_regions = dict(pv_x=[1e-11, 1.0, 20.0], pv_y=[0.3, 0.6, 0.2])                 # ignored (sic), :210
    pv_last = dict(pv_x=[1e-11, 5.0, 20.0], pv_y=[0.7, 0.4, 0.1], pv_nbt=[3], pv_int=[2])   # ignored: no next
    rxns = [(19, 1, 2.0, [(4, _law4([1e-11, 1e-3, 1.0, 9.0, 20.0], 491), pv3),
                          (7, _arr(tab1_block([1e-11, 3e-9, 2e-5, 0.1, 20.0], [1.3, 1.31, 1.32, 1.4, 1.45]), [-20.0]),
                           pv_no_regions),
                          (9, _arr(tab1_block([1e-11, 2.0, 20.0], [1.0, 1.2, 1.5]), [-5.0]), pv_last)]),
            (20, 25, 0.6, [(4, _law4([1e-11, 5e-6, 0.03, 20.0], 492, scheme=1))])]
    delayed = [(4, _law4([1e-11, 20.0], 493, n_pts=7, e_max=3.0))]
    return _chi_assemble(NUC_E, rxns, delayed, _lin_yields(1), CHI_BINS7,
                         why="a nested chain whose first spectrum has a three-region p_valid with union energies "
                             "strictly inside every region, a second with pairs but n_regions = 0 and a p_valid on "
                             "the last spectrum (both ignored)")


def chi_edge_cases():
    """Ordered name -> case, each in the layout of chi_case() (entries of spectra may be
    (law, data, p_valid dict)) with its own `bins`, the condition it exists for (`why`; computed
    from the inputs by tests/test_chi_edges.py) and `arith`.  groups_1_and_70 is one nuclide under
    two group structures, hence two entries."""
    bins70 = np.concatenate([[0.0], _geom(1e-11, 1.5076, 70, last=20.0)])       # log-spaced, as test_sab's 70 groups
    return {"arith_only": _case_arith_only(), "tab1_schemes": _case_tab1_schemes(), "thresholds": _case_thresholds(),
            "nearest_row": _case_nearest_row(), "eout_edges": _case_eout_edges(),
            "groups_1": _groups_nuclide([0.0, 20.0], 1), "groups_70": _groups_nuclide(bins70, 70),
            "many_energies": _case_many_energies(), "dup_energy": _case_dup_energy(),
            "dup_leading": _case_dup_leading(), "overflow": _case_overflow(), "no_delayed": _case_no_delayed(),
            "p_valid": _case_p_valid()}


# ---- thermal tables at their edges (sab_edge_cases) --------------------------
SAB_G8 = np.concatenate([[0.0], np.logspace(-9, np.log10(20.0), 8)])          # the 8 groups of make_golden.SAB_CASES
SAB_TOP_INSIDE = np.array([0.0, 1e-9, 1e-8, 1e-7, 3e-7])
SAB_BOTTOM_ABOVE = np.array([1e-8, 3e-8, 1e-7, 3e-7, 1e-6, 20.0])
SAB_EDGE_EXTEND_PTS = 2            # EXTEND_PTS of the stored sab_egrid (the default 50 only repeats each interval's fill)
SAB_EDGE_TOL = 1e-8
SAB_MODE_SEEDS = {0: 2000, 1: 2001, 2: 2002}        # the three tables of orders_* and groups_*


def _nbrs(v):
    v = float(v)
    return [float(np.nextafter(v, -np.inf)), v, float(np.nextafter(v, np.inf))]


def _sab_small(mode, seed, elastic=None, NEo=9, NMU=4, NEo_range=(5, 9)):
    """sab_table with 8 incoming energies; incoherent elastic data on 8 of its 12 energies (both ends kept)"""
    t = sab_table(mode, seed, NEi=8, NEo=NEo, NMU=NMU, elastic=elastic, NEo_range=NEo_range)
    if elastic == "incoherent":
        keep = np.array([0, 2, 3, 5, 6, 8, 10, 11])
        t.update(NEe=8, ee=t["ee"][keep], eP=t["eP"][keep], emu=t["emu"].reshape(12, -1)[keep].ravel())
    return t


def sab_groups_bins(G):
    if G == 1:
        return np.array([0.0, 20.0])
    if G == 70:
        return np.concatenate([[0.0], _geom(1e-11, 1.5076, 70, last=20.0)])    # as chi_edge_cases' 70 groups
    e = np.logspace(-11, np.log10(20.0), G)
    e[-1] = 20.0
    return np.concatenate([[0.0], e])


def sab_edge_cases():
    """Ordered name -> case of the thermal Legendre path: `table` (the layout of sab_table), `bins`,
    `ein` (its own, never sab_egrid's), `L` (orders, scatt_order + 1), `cond` (the condition it exists
    for; a condition that asks for a table per mode or per kind of elastic data has one case per
    table, named <cond>_m<mode> or <cond>_<kind>), `why`, and `egrid` (the structure spans 0 .. 20 MeV,
    so the reference's sab_egrid runs on it).  No case makes the reference stop: every threshold is
    the last energy of its table, so binary_search never sees a value outside its array."""
    out = {}

    def add(name, cond, t, bins, ein, L, why):
        bins = np.asarray(bins, dtype=np.float64)
        out[name] = dict(cond=cond, table=t, bins=bins, ein=np.unique(np.asarray(ein, dtype=np.float64)), L=L,
                         why=why, egrid=bool(bins[0] == 0.0 and bins[-1] >= 19.99))

    three = lambda: {m: _sab_small(m, SAB_MODE_SEEDS[m], "incoherent") for m in (0, 1, 2)}
    for L in (1, 11):
        for m, t in three().items():
            add(f"orders_{L}_m{m}", f"orders_{L}", t, SAB_G8, sab_ein_grid(t, n=14), L,
                f"order {L} of pn_rt (scatt_order {L - 1}) on 8 groups, incoherent elastic data")
    for G in (1, 70, 300):
        for m, t in three().items():
            add(f"groups_{G}_m{m}", f"groups_{G}", t, sab_groups_bins(G), sab_ein_grid(t, n=12), 2,
                f"G = {G}" + (": every live row has P0 = 1" if G == 1 else
                              ", log-spaced: rows whose plain sum of P0 over groups is not the compensated one"))

    t = _sab_small(2, 2101)
    ce, ptr = t["ce_out"].copy(), t["cptr"]
    for k in (1, 3, 4, 6):
        ce[ptr[k]] = 0.5 * ce[ptr[k] + 1]
    t["ce_out"] = ce
    first = min(ce[ptr[k]] for k in (1, 3, 4, 6))
    add("cont_first_eout_positive", "cont_first_eout_positive", t,
        np.unique([0.0, 0.25 * first, 0.75 * first, 1e-8, 1e-7, 1e-6, 20.0]), sab_ein_grid(t, n=12), 4,
        "continuous rows whose first E_out is positive with three group edges below it: e_bins(g) < Eout(1) with "
        "e_bins(g+1) < Eout(1) (the group is empty) and with e_bins(g+1) inside the row")

    t = _sab_small(2, 2102)
    ce, ptr = t["ce_out"].copy(), t["cptr"]
    ce[ptr[2]] = 0.5 * ce[ptr[2] + 1]
    t["ce_out"] = ce
    add("cont_edges_on_points", "cont_edges_on_points", t,
        np.unique([0.0, ce[ptr[2]], ce[ptr[3] + 2], ce[ptr[6] + 3], ce[ptr[6] - 1], 20.0]), sab_ein_grid(t, n=12), 4,
        "interior group edges equal to the first point of row 2, to interior points of rows 3 and 6 (f = 0) and to "
        "the last point of row 5 (the >= branches)")

    t = _sab_small(2, 2104, NMU=1, NEo_range=(2, 4))
    add("cont_two_point_rows", "cont_two_point_rows", t, SAB_G8, sab_ein_grid(t, n=12), 4,
        "continuous rows of exactly two outgoing energies, one cosine each")

    t = _sab_small(1, 2105, NEo=5, NMU=1)
    add("skewed_min", "skewed_min", t, SAB_G8, sab_ein_grid(t, n=12), 4,
        "the smallest legal skewed table: 5 outgoing energies (weights 0.1 0.4 1 0.4 0.1), one cosine")

    for m in (0, 1, 2):
        t = _sab_small(m, 2110 + m, "coherent")
        top = SAB_TOP_INSIDE[-1]
        add(f"top_inside_m{m}", "top_inside", t, SAB_TOP_INSIDE, np.concatenate([sab_ein_grid(t, n=12), _nbrs(top)]), 4,
            "the top edge 3e-7 lies below both thresholds: discrete E_out at or past it, E_in on it and one ulp to "
            "each side, rows left with no mass")
        lo = SAB_BOTTOM_ABOVE[0]
        add(f"bottom_above_zero_m{m}", "bottom_above_zero", t, SAB_BOTTOM_ABOVE,
            np.concatenate([sab_ein_grid(t, n=12), _nbrs(lo)]), 4,
            "the bottom edge 1e-8 lies above some discrete E_out and above some incoming energies")

    for kind, m, seed in (("coherent", 0, 2120), ("incoherent", 2, 2121)):
        t = _sab_small(m, seed, kind)
        ee = t["ee"]
        add(f"elastic_edges_{kind}", "elastic_edges", t, SAB_G8,
            np.concatenate([np.concatenate([_nbrs(e) for e in ee]), [0.5 * ee[0]]]), 4,
            "E_in on every elastic table energy (Bragg edge) and one ulp to each side, the elastic threshold and "
            "one ulp below it, a point below the first elastic energy")

    for m in (0, 1, 2):
        t = _sab_small(m, 2130 + m)
        ei = t["ei"]
        add(f"inel_edges_m{m}", "inel_edges", t, SAB_G8,
            np.concatenate([np.concatenate([_nbrs(e) for e in ei]), [0.5 * ei[0], 0.25 * ei[0]]]), 4,
            "E_in on every inelastic table energy and one ulp to each side, the inelastic threshold with both "
            "neighbours, two points below the first table energy")

    for name, m, seed, scale, between in (("thresholds_el_below", 0, 2140, 0.1, [6e-7, 1e-6, 2.5e-6]),
                                          ("thresholds_el_above", 2, 2141, 5.0, [6e-6, 1e-5, 1.5e-5])):
        t = _sab_small(m, seed, "coherent")
        t["ee"] = t["ee"] * scale
        t["threshold_elastic"] = float(t["ee"][-1])
        add(name, name, t, SAB_G8, np.concatenate([sab_ein_grid(t, n=10), between, _nbrs(t["threshold_elastic"])]), 4,
            "the elastic threshold lies " + ("below" if scale < 1 else "above") + " the inelastic one, incoming "
            "energies between the two: rows with " + ("inelastic" if scale < 1 else "elastic") + " scattering only")

    t = _sab_small(1, 2150, "incoherent")
    t["el_mode"] = 4
    add("exact_with_cosines", "exact_with_cosines", t, SAB_G8, sab_ein_grid(t, n=12), 4,
        "elastic mode EXACT with n_elastic_mu > 0: the reference's `pass` branch, el = sig * 0")

    t = _sab_small(0, 2160, "incoherent")
    add("two_energies", "two_energies", t, SAB_G8, [1e-9, 3e-8], 4,
        "two incoming energies: the last row of scatt_mat is the copy of the first")

    for m in (0, 1):
        t = sab_revisit_table(m)
        ei = t["ei"]
        grid = sab_ein_grid(t, n=20)
        add(f"eout_revisits_group_m{m}", "eout_revisits_group", t, SAB_G8,
            np.concatenate([grid[grid <= ei[4]], ei[:5], [ei[6]]]), 4,
            "discrete E_out out of order, the same way in every row: the outgoing energies leave a group and come "
            "back to it, so a bin kept in a register must go back to the row in between")
    return out


SAB_REVISIT_PERM = (0, 8, 1, 7, 2, 6, 3, 5, 4)      # of the sorted outgoing energies: low, high, low, high, ...


def sab_revisit_table(mode, perm=SAB_REVISIT_PERM):
    """_sab_small's discrete table with the outgoing energies of every row, and their cosines, taken in
    the order `perm`: a blend of two rows keeps that order"""
    t = _sab_small(mode, 2170 + mode)
    NEi, NEo, NMU = t["NEi"], t["NEo"], t["NMU"]
    p = np.asarray(perm)
    t["e_out"] = np.ascontiguousarray(t["e_out"].reshape(NEi, NEo)[:, p]).ravel()
    t["mu"] = np.ascontiguousarray(t["mu"].reshape(NEi, NEo, NMU)[:, p]).ravel()
    return t


def apply_tol_edge_inputs():
    """name -> data[n][G][L] for apply_tol_scatt at tol = SAB_EDGE_TOL: (L, G, n) = (1, 1, 1), (11, 8, 129),
    (2, 70, 40), (2, 300, 40).  A few live groups per row, P0 over twelve decades; from n > 1 on, row 1 is all
    zero, every positive P0 of row 2 is below tol (the reference gives 0 * (orig / 0) = NaN), row 3 has a P0
    equal to tol, row 4 a negative P0, row 5 a single value above tol and nothing else, row 6 a negative total."""
    out = {}
    for L, G, n in ((1, 1, 1), (11, 8, 129), (2, 70, 40), (2, 300, 40)):
        rng = np.random.default_rng(9000 + G)
        p0 = rng.uniform(0, 1, (n, G)) * 10.0 ** rng.integers(-12, 1, (n, G))
        d = rng.uniform(-1, 1, (n, G, L)) * p0[:, :, None]
        d[:, :, 0] = p0
        d = d * (rng.uniform(size=(n, G)) < min(1.0, 4.0 / G))[:, :, None]
        if n == 1:
            d[0, 0, :] = 3e-9
        else:
            d[1] = 0.0
            d[2] = 0.0
            d[2, :3, :] = np.array([3e-9, 9.9e-9, 1e-12])[:, None]
            d[3, 0, 0] = SAB_EDGE_TOL
            d[4, 0, 0], d[4, 1, 0] = -0.25, 0.9
            d[5] = 0.0
            d[5, G - 1, :] = 0.7
            d[6] = 0.0
            d[6, 0, 0], d[6, 1, 0] = -0.5, 0.25
        out[f"L{L}_G{G}_n{n}"] = np.ascontiguousarray(d)
    return out


# ---- raw ACE blocks for the ACE -> tabular conversion (convert_file4 / convert_file6) ----
def _ang_table(rng, interp, npts, positive=False):
    """[JJ, NP, cosines(NP), pdf(NP), cdf(NP)] of one ACE tabular angular distribution."""
    cs = np.concatenate([[-1.0], np.sort(rng.uniform(-1, 1, npts - 2)), [1.0]])
    if positive:                       # log interpolation in mu needs mu > 0 to be finite
        cs = np.linspace(1e-3, 1.0, npts)
    pdf = 0.5 * (1 + rng.uniform(-0.8, 0.8) * cs + rng.uniform(0, 0.4) * cs ** 2) + 0.05
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(cs))])
    return [float(interp), float(npts)] + list(cs) + list(pdf / cdf[-1]) + list(cdf / cdf[-1])


def ace_adist(energies, kinds, seed):
    """DistAngle (ace_header.F90:14-24): kinds[k] in {"iso", "equi", "hist", "lin"}.
    Returns energy, type, location, data (locations are 0-based offsets lc with
    data(lc+1) the first word, as ace.F90 stores them)."""
    rng = np.random.default_rng(seed)
    data, typ, loc = [0.0], [], []     # one pad word so that no table sits at lc = 0
    for k in kinds:
        if k == "iso":
            typ.append(1)
            loc.append(0)
        elif k == "equi":
            typ.append(2)
            loc.append(len(data))       # data(lc+1) is the first edge; data(lc) must exist
            edges = np.concatenate([[-1.0], np.sort(rng.uniform(-1, 1, 31)), [1.0]])
            data += list(edges)
        else:
            typ.append(3)
            loc.append(len(data))
            data += _ang_table(rng, 1 if k == "hist" else 2, int(rng.integers(3, 40)))
    return (np.asarray(energies, dtype=np.float64), np.array(typ, dtype=np.int32),
            np.array(loc, dtype=np.int32), np.array(data))


def ace_edist(law, e_in, np_lo, np_hi, seed, interps=(1, 2), inttp=2):
    """edist%data of ACE law 4 / 44 / 61 (layout read at scattdata_header.F90:799-865):
    NR=0, NE, E_in(NE), L(NE), then per E_in INTT', NP, E_out, pdf, cdf and law 44: R, A;
    law 61: LC(NP) locators (0 = isotropic) followed by the angular tables."""
    rng = np.random.default_rng(seed)
    NE = len(e_in)
    head = [0.0, float(NE)] + list(e_in)
    body, locs = [], []
    pos = len(head) + NE
    for k in range(NE):
        NP = int(rng.integers(np_lo, np_hi + 1))
        emax = 0.9 * e_in[k]
        eo = np.concatenate([[0.0], np.sort(rng.uniform(0, emax, NP - 2)), [emax]])
        pdf = np.exp(-eo / (0.3 * emax)) * (eo + 0.05 * emax)
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(eo))])
        blk = [float(inttp), float(NP)] + list(eo) + list(pdf / cdf[-1]) + list(cdf / cdf[-1])
        locs.append(float(pos))
        if law == 44:
            blk += list(rng.uniform(0, 0.5, NP)) + list(rng.uniform(0.5, 3.0, NP))
        elif law == 61:
            lc_at = len(blk)
            blk += [0.0] * NP
            for j in range(NP):
                if rng.uniform() < 0.2:
                    continue                                  # LC = 0: isotropic
                interp = int(interps[int(rng.integers(len(interps)))])
                blk[lc_at + j] = float(pos + len(blk))
                blk += _ang_table(rng, interp, int(rng.integers(3, 30)), positive=interp in (3, 5))
        pos += len(blk)
        body += blk
    return np.array(head + locs + body)


# ---- nuclide-level inputs of the E_in grid builders (create_Ein_grid) --------------------
def grid_cases():
    """(name, dict) pairs: what create_Ein_grid reads -- nuclide grid, group structure,
    awr, kT, free-gas cutoff, inelastic threshold and per ScattData (is_init, MT, Q, E_grid)."""
    kT = 2.5301e-8
    bins2 = np.array([0.0, 6.25e-7, 20.0])
    bins8 = np.concatenate([[1e-11], np.logspace(-7, np.log10(20.0), 8)])
    bins5 = np.array([0.0, 1e-3, 0.05, 0.5, 3.0, 20.0])
    h1 = dict(awr=0.999167, kT=kT, cutoff=400.0 * kT, thresh=20.0, bins=bins2,
              nuc=np.logspace(-11, np.log10(20.0), 300),
              sds=[(1, 2, 0.0, np.array([1e-11, 1e-6, 1.0, 20.0]))])
    nuc_u = np.unique(np.concatenate([np.logspace(-11, np.log10(30.0), 400), [0.0449, 0.148, 1.0]]))
    u_sds = [(1, 2, 0.0, np.logspace(-5, np.log10(20.0), 40)),
             (1, 51, -0.0449, np.array([0.0451, 1.0, 20.0])),
             (1, 52, -0.148, np.array([0.1486, 2.0, 30.0])),
             (0, 18, 190.0, np.array([1e-11, 20.0])),
             (1, 91, -1.2, np.array([1.3, 2.5, 6.0, 12.0, 20.0])),
             (1, 16, -6.15, np.array([6.2, 9.0, 14.0, 20.0]))]
    u2 = dict(awr=236.0058, kT=kT, cutoff=400.0 * kT, thresh=0.0449, bins=bins2, nuc=nuc_u, sds=u_sds)
    u5 = dict(u2, bins=bins5)
    u8 = dict(u2, bins=bins8, cutoff=0.0)        # free-gas treatment off, first edge > 0
    o16 = dict(awr=15.8575, kT=kT, cutoff=400.0 * kT, thresh=6.4, bins=bins5,
               nuc=np.logspace(-11, np.log10(20.0), 150),
               sds=[(1, 2, 0.0, np.logspace(-6, np.log10(20.0), 25)),
                    (1, 51, -6.05, np.array([6.4, 10.0, 20.0]))])
    return [("h1_g2", h1), ("u238_g2", u2), ("u238_g5", u5), ("u238_g8_nofg", u8), ("o16_g5", o16)]


# ---- a whole nuclide as raw ACE blocks (calc_scatt / ndpp_scatt_nuclide) -------------------
def nuclide_case():
    """An O-16-like nuclide: elastic with isotropic / tabular / 32-equiprobable angular tables
    and free gas below 4 kT; MT 51 level (law 3 + tabular angles); MT 91 continuum (law 44, CM,
    p_valid 1 -> 0.8); MT 22 (law 61, lab, energy-dependent multiplicity); MT 102 capture and an
    MT 18 fission entry that ScattData%init must skip.  Three groups."""
    kT = 2.5301e-8
    n_grid = 30
    energy = 1e-11 * (20.0 / 1e-11) ** (np.arange(n_grid) / (n_grid - 1.0))
    elastic = 3.8 + 0.2 / (1.0 + energy)
    el_ad = ace_adist([1e-11, 1e-3, 20.0], ["iso", "lin", "equi"], seed=16)
    thr = {51: 29, 91: 29, 22: 28}
    def sigma(MT, scale):
        n = n_grid - thr[MT] + 1
        return scale * np.arange(n) / max(n - 1, 1) + 0.01 * np.arange(n)
    lvl_ad = ace_adist([energy[thr[51] - 1], 20.0], ["lin", "hist"], seed=51)
    pv = ([1e-5, 20.0], [1.0, 0.8])
    reactions = [
        dict(MT=2, Q=0.0, mult=1, thr=1, in_cm=1, sigma=None, adist=el_ad, edists=[]),
        dict(MT=102, Q=4.1, mult=0, thr=1, in_cm=0, sigma=0.1 / np.sqrt(energy / 1e-11), adist=None, edists=[]),
        dict(MT=51, Q=-6.05, mult=1, thr=thr[51], in_cm=1, sigma=sigma(51, 0.2), adist=lvl_ad,
             edists=[dict(law=3, data=np.array([6.43, 0.885]), pv_x=None, pv_y=None)]),
        dict(MT=91, Q=-7.2, mult=1, thr=thr[91], in_cm=1, sigma=sigma(91, 0.3), adist=None,
             edists=[dict(law=44, data=ace_edist(44, np.array([1.0, 5.0, 20.0]), 5, 9, seed=91, inttp=2),
                          pv_x=pv[0], pv_y=pv[1])]),
        dict(MT=22, Q=-2.5, mult=1, thr=thr[22], in_cm=0, sigma=sigma(22, 0.4), adist=None,
             edists=[dict(law=61, data=ace_edist(61, np.array([1.0, 5.0, 20.0]), 5, 9, seed=22),
                          pv_x=[1e-5, 20.0], pv_y=[0.9, 1.0])],
             mult_E=([1e-5, 10.0, 20.0], [1.0, 1.5, 2.0])),
        dict(MT=18, Q=190.0, mult=1, thr=1, in_cm=0, sigma=np.ones(n_grid), adist=None, edists=[]),
    ]
    return dict(awr=15.8575, kT=kT, freegas_cutoff=4.0 * kT, energy=energy, elastic=elastic,
                reactions=reactions, bins=np.array([0.0, 6.25e-7, 0.1, 20.0]),
                order=2, mu_bins=129, extend_pts=3, inel_extend_pts=4)


def pack_nuclide(d):
    """Flat (ints, doubles) encoding of nuclide_case() for oracle/ref_shim.f90:ref_calc_scatt."""
    I, D = [len(d["energy"]), len(d["reactions"])], [d["awr"], d["kT"], d["freegas_cutoff"]]
    D += list(d["energy"]) + list(d["elastic"])
    for r in d["reactions"]:
        sig = [] if r["sigma"] is None else list(r["sigma"])
        ad = r["adist"]
        mE = r.get("mult_E")
        I += [r["MT"], r["mult"], r["thr"], r["in_cm"], len(sig), 0 if ad is None else 1,
              0 if ad is None else len(ad[0]), 0 if ad is None else len(ad[3]), len(r["edists"]),
              0 if mE is None else len(mE[0])]
        D += [r["Q"]] + sig
        if ad is not None:
            I += list(ad[1]) + list(ad[2])
            D += list(ad[0]) + list(ad[3])
        if mE is not None:
            D += list(mE[0]) + list(mE[1])
        for ed in r["edists"]:
            npv = 0 if ed["pv_x"] is None else len(ed["pv_x"])
            I += [ed["law"], len(ed["data"]), npv]
            D += list(ed["data"])
            if npv:
                D += list(ed["pv_x"]) + list(ed["pv_y"])
    return np.array(I, dtype=np.int32), np.array(D, dtype=np.float64)


# ---- BASELINE configs[2] / SURVEY 8(d) #3: a U-238-like nuclide -----------------------------
def _lin_table(cs, pdf):
    """[JJ=2, NP, cosines, pdf, cdf] of one lin-lin ACE angular table, normalised."""
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(cs))])
    return [2.0, float(len(cs))] + list(cs) + list(pdf / cdf[-1]) + list(cdf / cdf[-1])


def _forward_adist(energies, a_of, b_of, npts=33):
    """DistAngle with an isotropic first row and tabular lin-lin rows
    f = 1/2 (1 + a(E) mu + b(E) P2(mu)) on npts cosines."""
    cs = np.linspace(-1.0, 1.0, npts)
    data, typ, loc = [0.0], [1], [0]
    for E in energies[1:]:
        typ.append(3)
        loc.append(len(data))
        data += _lin_table(cs, 0.5 * (1 + a_of(E) * cs + b_of(E) * (1.5 * cs * cs - 0.5)))
    return (np.asarray(energies, dtype=np.float64), np.array(typ, dtype=np.int32),
            np.array(loc, dtype=np.int32), np.array(data))


def u238_case(n_grid=50000, n_levels=40, n_el_rows=200, groups=2, order=7, mu_bins=2001,
              freegas_cutoff_kT=400.0, extend_pts=50, inel_extend_pts=30):
    """The nuclide of BASELINE configs[2] as SURVEY 8(d) #3 makes it concrete: A = 236.0058,
    293.6 K; elastic with n_el_rows tabular lin-lin angular tables (33 cosines) on 1e-5..20 MeV;
    n_levels level reactions (MT 51...), Q_k = -(0.0449 + 0.05 k) MeV, CM, isotropic -> mildly
    forward; MT 91 law-44 continuum in CM (30 incoming energies x 40 outgoing points); MT 22
    law 4 + angular table in the lab; MT 16 (n,2n) evaporation (law 9), multiplicity 2.
    n_grid log-spaced nuclide energies.  groups = 2 (the shipped structure) or 70 (log grid)."""
    awr, kT = 236.0058, 2.53e-8
    energy = 1e-11 * (20.0 / 1e-11) ** (np.arange(n_grid) / (n_grid - 1.0))
    energy[-1] = 20.0
    elastic = 9.0 + 3.0 / (1.0 + 50.0 * energy)
    el_E = np.concatenate([[1e-11], np.logspace(-5, np.log10(20.0), n_el_rows)])
    el_E[-1] = 20.0
    el_ad = _forward_adist(el_E, lambda E: 0.8 * E / 20.0, lambda E: 0.5 * (E / 20.0) ** 2)

    def thr_of(Q):  # first grid point at or above the kinematic threshold
        return int(np.searchsorted(energy, -Q * (awr + 1.0) / awr, side="left")) + 1

    def sigma_of(Q, thr, step):
        E = energy[thr - 1:]
        return step * (1.0 - np.exp(-(E + Q * (awr + 1.0) / awr).clip(0.0) / 0.1)) + 1e-6

    reactions = [dict(MT=2, Q=0.0, mult=1, thr=1, in_cm=1, sigma=None, adist=el_ad, edists=[]),
                 dict(MT=102, Q=4.8, mult=0, thr=1, in_cm=0, sigma=2.7 / np.sqrt(energy / 2.53e-8), adist=None,
                      edists=[])]
    for k in range(n_levels):
        Q = -(0.0449 + 0.05 * k)
        thr = thr_of(Q)
        ad = _forward_adist([energy[thr - 1], 20.0], lambda E: 0.3, lambda E: 0.1)
        reactions.append(dict(MT=51 + k, Q=Q, mult=1, thr=thr, in_cm=1, sigma=sigma_of(Q, thr, 0.05 + 0.002 * k),
                              adist=ad, edists=[dict(law=3, data=np.array([-Q * (awr + 1.0) / awr,
                                                                           (awr / (awr + 1.0)) ** 2]),
                                                     pv_x=None, pv_y=None)]))
    pv = ([1e-11, 20.0], [1.0, 1.0])      # every energy distribution carries its p_valid TAB1
    Qc = -(0.0449 + 0.05 * n_levels)
    thr = thr_of(Qc)
    e44 = np.logspace(np.log10(energy[thr - 1]), np.log10(20.0), 30)
    e44[0], e44[-1] = energy[thr - 1], 20.0
    reactions.append(dict(MT=91, Q=Qc, mult=1, thr=thr, in_cm=1, sigma=sigma_of(Qc, thr, 1.2), adist=None,
                          edists=[dict(law=44, data=ace_edist(44, e44, 40, 40, seed=238), pv_x=pv[0], pv_y=pv[1])]))
    Q22 = -4.0
    thr = thr_of(Q22)
    e4 = np.logspace(np.log10(energy[thr - 1]), np.log10(20.0), 12)
    e4[0], e4[-1] = energy[thr - 1], 20.0
    # (a reaction with both an angular and a law-4 / law-9 energy distribution is converted row by
    # row on the ENERGY distribution's incoming grid, scattdata_header.F90:236-250: the angular
    # tables must sit on the same energies)
    ad22 = _forward_adist(list(e4), lambda E: 0.4 * E / 20.0, lambda E: 0.0)
    reactions.append(dict(MT=22, Q=Q22, mult=1, thr=thr, in_cm=0, sigma=sigma_of(Q22, thr, 0.1), adist=ad22,
                          edists=[dict(law=4, data=ace_edist(4, e4, 20, 20, seed=22), pv_x=pv[0], pv_y=pv[1])]))
    Q16 = -6.15
    thr = thr_of(Q16)
    e9 = np.logspace(np.log10(energy[thr - 1]), np.log10(20.0), 8)
    ad16 = _forward_adist(list(e9), lambda E: 0.2, lambda E: 0.0)
    reactions.append(dict(MT=16, Q=Q16, mult=2, thr=thr, in_cm=0, sigma=sigma_of(Q16, thr, 0.8), adist=ad16,
                          edists=[dict(law=9, data=law9_edata(energy[thr - 1], 20.0, n=8, U=-Q16 * (awr + 1) / awr),
                                       pv_x=pv[0], pv_y=pv[1])]))
    reactions.append(dict(MT=18, Q=190.0, mult=1, thr=1, in_cm=0, sigma=np.full(n_grid, 1e-5), adist=None, edists=[]))
    bins = np.array([0.0, 6.25e-7, 20.0]) if groups == 2 else \
        np.concatenate([[0.0], np.logspace(-11, np.log10(20.0), groups)])
    bins[-1] = 20.0
    return dict(awr=awr, kT=kT, freegas_cutoff=freegas_cutoff_kT * kT, energy=energy, elastic=elastic,
                reactions=reactions, bins=bins, order=order, mu_bins=mu_bins, extend_pts=extend_pts,
                inel_extend_pts=inel_extend_pts)


def library_nuclide(awr, seed, n_grid=None, kT=2.53e-8, groups=2, order=5, mu_bins=2001,
                    freegas_cutoff_kT=400.0, scale=1.0, extend_pts=50, inel_extend_pts=30):
    """One nuclide of the synthetic library of BASELINE configs[4] / SURVEY 8(d) #5: the shape of
    u238_case with table sizes drawn (seeded) around the config-3 sizes and scaled with the mass:
    elastic angular tables on every nuclide; level reactions, a law-44 continuum (CM), a law-4
    reaction with an angular table (lab) and an (n,2n) evaporation spectrum appear with
    increasing mass.  The nuclide grid has n_grid log-spaced energies, about half of them below
    the free-gas cutoff, so that the free-gas part of the incoming grid -- where the time goes --
    has 200..800 points with the ~150 points the grid builder adds around the group edges."""
    rng = np.random.default_rng(seed)
    if n_grid is None:
        n_grid = int(rng.integers(100, 1301) * scale) + 20
    energy = 1e-11 * (20.0 / 1e-11) ** (np.arange(n_grid) / (n_grid - 1.0))
    energy[-1] = 20.0
    elastic = 4.0 + 16.0 * rng.uniform(0.2, 1.0) / (1.0 + 30.0 * energy)
    n_el_rows = int(np.clip(rng.lognormal(np.log(10 + 150 * awr / 240.0), 0.4), 3, 300))
    el_E = np.concatenate([[1e-11], np.logspace(-5, np.log10(20.0), n_el_rows)])
    el_E[-1] = 20.0
    a1, b1 = rng.uniform(0.3, 0.9), rng.uniform(0.1, 0.5)
    el_ad = _forward_adist(el_E, lambda E: a1 * E / 20.0, lambda E: b1 * (E / 20.0) ** 2)

    def thr_of(Q):
        return min(int(np.searchsorted(energy, -Q * (awr + 1.0) / awr, side="left")) + 1, n_grid - 2)

    def sigma_of(Q, thr, step):
        E = energy[thr - 1:]
        return step * (1.0 - np.exp(-(E + Q * (awr + 1.0) / awr).clip(0.0) / 0.1)) + 1e-6

    reactions = [dict(MT=2, Q=0.0, mult=1, thr=1, in_cm=1, sigma=None, adist=el_ad, edists=[]),
                 dict(MT=102, Q=4.8, mult=0, thr=1, in_cm=0, sigma=2.7 / np.sqrt(energy / 2.53e-8), adist=None,
                      edists=[])]
    pv = ([1e-11, 20.0], [1.0, 1.0])
    n_levels = 0 if awr < 4.0 else int(np.clip(rng.lognormal(np.log(2 + 38 * awr / 240.0), 0.3), 1, 40))
    q0 = 0.0449 + 2.0 / max(awr, 4.0)
    for k in range(n_levels):
        Q = -(q0 + 0.05 * k)
        thr = thr_of(Q)
        ad = _forward_adist([energy[thr - 1], 20.0], lambda E: 0.3, lambda E: 0.1)
        reactions.append(dict(MT=51 + k, Q=Q, mult=1, thr=thr, in_cm=1, sigma=sigma_of(Q, thr, 0.05 + 0.002 * k),
                              adist=ad, edists=[dict(law=3, data=np.array([-Q * (awr + 1.0) / awr,
                                                                           (awr / (awr + 1.0)) ** 2]),
                                                     pv_x=None, pv_y=None)]))
    if awr >= 10.0:
        Qc = -(q0 + 0.05 * n_levels)
        thr = thr_of(Qc)
        ne44 = int(np.clip(rng.lognormal(np.log(8 + 22 * awr / 240.0), 0.3), 4, 40))
        np44 = int(np.clip(rng.lognormal(np.log(10 + 30 * awr / 240.0), 0.3), 6, 60))
        e44 = np.logspace(np.log10(energy[thr - 1]), np.log10(20.0), ne44)
        e44[0], e44[-1] = energy[thr - 1], 20.0
        reactions.append(dict(MT=91, Q=Qc, mult=1, thr=thr, in_cm=1, sigma=sigma_of(Qc, thr, 1.2), adist=None,
                              edists=[dict(law=44, data=ace_edist(44, e44, np44, np44, seed=seed + 1), pv_x=pv[0],
                                           pv_y=pv[1])]))
    if awr >= 20.0:
        Q22 = -4.0
        thr = thr_of(Q22)
        e4 = np.logspace(np.log10(energy[thr - 1]), np.log10(20.0), 8)
        e4[0], e4[-1] = energy[thr - 1], 20.0
        ad22 = _forward_adist(list(e4), lambda E: 0.4 * E / 20.0, lambda E: 0.0)
        reactions.append(dict(MT=22, Q=Q22, mult=1, thr=thr, in_cm=0, sigma=sigma_of(Q22, thr, 0.1), adist=ad22,
                              edists=[dict(law=4, data=ace_edist(4, e4, 12, 12, seed=seed + 2), pv_x=pv[0],
                                           pv_y=pv[1])]))
    if awr >= 30.0:
        Q16 = -6.15
        thr = thr_of(Q16)
        e9 = np.logspace(np.log10(energy[thr - 1]), np.log10(20.0), 6)
        ad16 = _forward_adist(list(e9), lambda E: 0.2, lambda E: 0.0)
        reactions.append(dict(MT=16, Q=Q16, mult=2, thr=thr, in_cm=0, sigma=sigma_of(Q16, thr, 0.8), adist=ad16,
                              edists=[dict(law=9, data=law9_edata(energy[thr - 1], 20.0, n=6,
                                                                  U=-Q16 * (awr + 1) / awr),
                                           pv_x=pv[0], pv_y=pv[1])]))
    bins = np.array([0.0, 6.25e-7, 20.0]) if groups == 2 else \
        np.concatenate([[0.0], np.logspace(-11, np.log10(20.0), groups)])
    bins[-1] = 20.0
    return dict(awr=float(awr), kT=kT, freegas_cutoff=freegas_cutoff_kT * kT, energy=energy, elastic=elastic,
                reactions=reactions, bins=bins, order=order, mu_bins=mu_bins, extend_pts=extend_pts,
                inel_extend_pts=inel_extend_pts)


def synthetic_library(n_nuclides=423, n_thermal=20, n_fissionable=30, seed=2024, scale=1.0, order=5, **nuc_kw):
    """The library of SURVEY 8(d) #5: n_nuclides nuclide descriptors (masses log-uniform in
    [1, 250], the .71c count of the reference's NNDC listing), n_thermal thermal tables (half
    discrete, half continuous, two with elastic parts) and chi inputs for the n_fissionable
    heaviest nuclides.  Everything seeded; `scale` shrinks the grids for tests, nuc_kw goes to
    library_nuclide (e.g. a small free-gas region so that the reference can afford goldens)."""
    rng = np.random.default_rng(seed)
    awr = np.sort(np.exp(rng.uniform(np.log(1.0), np.log(250.0), n_nuclides)))
    nucs = [library_nuclide(awr[k], seed=seed * 1000 + k, scale=scale, order=order, **nuc_kw) for k in range(n_nuclides)]
    thermal = []
    for k in range(n_thermal):
        mode = 1 if k % 2 == 0 else 2
        el = "coherent" if k == 3 else ("incoherent" if k == 7 else None)
        nei = max(8, int(116 * scale))
        thermal.append(sab_table(mode, seed=seed + 100 + k, NEi=nei, NEo=max(8, int(64 * scale)) if mode == 1 else 16,
                                 NMU=16 if mode == 1 else 20, elastic=el))
    fissionable = list(range(n_nuclides - n_fissionable, n_nuclides))
    chis = [chi_case(seed=seed + 500 + k) for k in range(n_fissionable)]
    return dict(awr=awr, nuclides=nucs, thermal=thermal, fissionable=fissionable, chi=chis)


# ---- file-4 two-body kinematics (integrate_file4_cm_leg) beyond mu_bins = 2001 -------------
FILE4_M = (5, 64, 65, 129, 1000, 2001)
FILE4_L = (1, 3, 4, 5, 6, 7, 8, 9, 10, 11)          # every LMAX template (4, 6, 8, 11) and L below it
FILE4_G = (1, 2, 63, 64, 65, 128, 129, 300)
FILE4_KINDS = ("quadratic", "step", "kink", "ramp", "exp", "random", "negative", "negative kink")
# the kinds whose values need + - * / and comparisons only: the same bits with every numpy
FILE4_EXACT_KINDS = (0, 1, 2, 3, 6, 7)


def file4_tables(mu, seed):
    """The f(mu) tables of FILE4_KINDS as consecutive rows, [8][len(mu)]: smooth quadratic, step at
    0.2137, kink, a run of zeros followed by a ramp, a forward peak, seeded uniform random, and
    the quadratic and the kink negated.  The last two are no distributions: with them a
    zero-width piece at mu = 1 gives -0.0 in both rows of a blend, so a group that the reference
    skips (+0.0) and a kernel does not differs in the sign bit, which the tests compare.
    Adjacent rows are unlike, so a blend of rows k and k + 1 mixes two shapes."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([
        0.5 * (1 + 0.4 * mu + 0.3 * (1.5 * mu * mu - 0.5)),
        np.where(mu < 0.2137, 0.25, 1.0),
        np.abs(mu - 0.3331) + 0.05,
        np.maximum(0.0, mu - 0.5),
        np.exp(8.0 * (mu - 1.0)),
        rng.uniform(0.0, 1.0, len(mu)),
        -0.5 * (1 + 0.4 * mu + 0.3 * (1.5 * mu * mu - 0.5)),
        -(np.abs(mu - 0.3331) + 0.05)]))


def file4_kinematics():
    """(awr, Q): R < 1 (awr < 1), hydrogen, awr = 1 exactly, two thresholds (light and heavy),
    heavy elastic, exothermic."""
    return [(0.5, 0.0), (0.999167, 0.0), (1.0, 0.0), (15.8575, -6.05), (236.0058, -0.0449),
            (236.0058, 0.0), (26.75, 1.2)]


def file4_bins(G):
    """G = 1: [0, 20]; G = 2: the shipped two-group structure; else the fine structures
    [0] + geomspace(1e-9, 20, G)."""
    if G == 1:
        return np.array([0.0, 20.0])
    if G == 2:
        return np.array([0.0, 6.25e-7, 20.0])
    bins = np.concatenate([[0.0], np.geomspace(1e-9, 20.0, G)])
    bins[-1] = 20.0
    return bins


def file4_threshold(awr, Q):
    return -Q * (awr + 1.0) / awr if Q < 0.0 else 0.0


def file4_energies(awr, Q, n_ladder=7):
    """Incoming energies of one file-4 call, never below the threshold (there the reference takes
    the square root of a negative number): a geometric ladder from max(1e-6, thr (1 + 1e-7)) to
    19.5, that lower end times 1.0000001, the top bin edge 20 and 25 above it."""
    lo = max(1e-6, file4_threshold(awr, Q) * (1.0 + 1e-7))
    return np.concatenate([np.geomspace(lo, 19.5, n_ladder), [lo * 1.0000001, 20.0, 25.0]])


def file4_matrix():
    """The (M, L, G, awr, Q) combinations that the oracle-vs-Fortran sweep and the GPU tests share:
    every (M, L) pair, 60 cases; case k = 10 iM + iL takes the (G, kinematics) pair number
    11 k mod 56 of the 8 x 7 pairs in row-major order.  11 and 56 are coprime, so cases 0..55
    visit every (G, kinematics) pair once and the last four visit four of them again."""
    kin = file4_kinematics()
    cases = []
    for iM, M in enumerate(FILE4_M):
        for iL, L in enumerate(FILE4_L):
            pair = (11 * (10 * iM + iL)) % (len(FILE4_G) * len(kin))
            G, (awr, Q) = FILE4_G[pair // len(kin)], kin[pair % len(kin)]
            cases.append((M, L, G, awr, Q))
    return cases


def file4_batch(M, L, G, awr, Q):
    """Inputs of one elastic_leg_batch call of the matrix: the eight tables, the energies and, per
    energy, a random lower row and a blend weight in [0, 1] with exactly 0 and exactly 1 among
    them.  Seeded by the combination (the random table by M alone), so every caller sees the same
    numbers."""
    seed = 1000003 * M + 10007 * L + 101 * G + int(1000 * awr) + int(100 * abs(Q))
    rng = np.random.default_rng(seed)
    mu = mu_grid(M)
    ein = file4_energies(awr, Q)
    row_lo = rng.integers(0, len(FILE4_KINDS) - 1, len(ein)).astype(np.int32)
    w_hi = rng.uniform(0.0, 1.0, len(ein))
    w_hi[1], w_hi[-2] = 0.0, 1.0
    row_lo[[0, 4]] = len(FILE4_KINDS) - 2        # the two negative rows blended: -0.0 can come out
    return dict(mu=mu, f_tab=file4_tables(mu, M), bins=file4_bins(G), ein=ein, row_lo=row_lo, w_hi=w_hi)


def file4_bound_classes(M, awr, Q, Ein, bins):
    """file4_bounds of the kernel (scattdata_header.F90:986-1015) restated: per group the clamped
    CM cosines and 1-based cells of its two bounds.  Returns (wlo, whi, ilo, ihi)."""
    mu = mu_grid(M)
    dw = mu[1] - mu[0]
    R = awr * np.sqrt(1.0 + Q * (awr + 1.0) / (awr * Ein))
    a, b, c = (1.0 + awr) * (1.0 + awr), 1.0 + R * R, 0.5 / (R * Ein)
    w = np.clip((np.asarray(bins) * a - Ein * b) * c, -1.0, 1.0)
    iw = ((w + 1.0) / dw).astype(np.int64) + 1
    return w[:-1], w[1:], iw[:-1], iw[1:]


def file4_golden_cases(g, M=None):
    """The calls recorded in tests/golden/file4_cm_edges.npz (g: the loaded file), optionally
    those of one M: (M, L, G, awr, Q, Ein, kind, fw, bins, what the Fortran returned [G][L]).
    Tables up to M = 129 and the group structures are read from the file; the larger tables are
    of the kinds that are rebuilt exactly (FILE4_EXACT_KINDS)."""
    off = 0
    for k in range(int(g["n"])):
        Mk, L, G, kind = int(g["M"][k]), int(g["L"][k]), int(g["G"][k]), int(g["kind"][k])
        ref = g["out"][off:off + G * L].reshape(G, L)
        off += G * L
        if M is not None and Mk != M:
            continue
        if Mk <= 129:
            fw = g[f"tab_{Mk}"][kind]
        else:
            assert kind in FILE4_EXACT_KINDS
            fw = file4_tables(mu_grid(Mk), int(g["seed"][k]))[kind]
        if int(g["top"][k]):
            bins = g[f"bins_top_{Mk}"]
        else:
            bins = g[f"bins_{G}"]
        yield (Mk, L, G, float(g["A"][k]), float(g["Q"][k]), float(g["Ein"][k]), kind,
               np.ascontiguousarray(fw), np.ascontiguousarray(bins), ref)


FILE4_TOP_AWR = 15.8575


def file4_top_inputs(M):
    """Inputs on which the VALUE the top-of-grid branch returns can be seen.  Where a bound is
    clamped to +1 the branch's value is multiplied by the zero width 1 - mu[M - 1]; it counts
    only when a bound BELOW +1 lands in cell M: within rounding of +1, so that (w + 1) / dw
    rounds up to M - 1.  For elastic scattering w(E') = 1 at E' = E_in, so the bin edges tried are
    E_in stepped down by a few ulps, for awr = 15.8575; kept are those whose cosine is below 1 and
    in cell M (found by the restated bounds, IEEE arithmetic only: the same everywhere).
    Returns (ein, bins): the energies that have such an edge, and [0, those edges, 20].  The
    group above such an edge is one piece [w, 1] of width ~1e-16 that starts in cell M; the group
    below it ends there, at a cosine left of the grid's last point (a last piece of negative
    width, as in the reference).  Nothing for M = 2001: there +1 itself is in cell M - 1."""
    ein, edges = [], []
    for Ein in (1e-3, 0.7, 1.5, 3.3, 12.0):
        e = Ein
        for _ in range(8):
            e = float(np.nextafter(e, 0.0))
            wlo, _, ilo, _ = file4_bound_classes(M, FILE4_TOP_AWR, 0.0, Ein, np.array([e, 20.0]))
            if wlo[0] < 1.0 and ilo[0] == M:
                ein.append(Ein)
                edges.append(e)
                break
    return np.array(ein), np.concatenate([[0.0], edges, [20.0]])


def same_bits(a, b):
    """a and b have the same shape and the same bit patterns: np.array_equal that also tells -0.0
    from +0.0 (and takes equal NaNs as equal)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())
