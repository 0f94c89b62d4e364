"""ACE table reader: turns the tables a cross_sections.xml lists into the dicts the library's
entry points take (ndpp_amd.lib: AceNuclide.from_desc for scatt_nuclide / scatt_library /
scatt_*_tab, chi_structs for chi_batch / chi_egrid_lib, SabFlat.from_dict for sab_batch /
sab_egrid_lib).  Nothing is integrated or converted here: energy-distribution laws are passed on
as their raw LDAT blocks, and ndpp_scattdata_shape / ndpp_convert_distro decide what is used.

The ACE layout (the public MCNP / NJOY format):

* ASCII (type 1): a table starts on line `location` of its file.  Line 1 holds the name (A10),
  the atomic weight ratio and the temperature in MeV (2G12.0) and the date; line 2 a comment
  (A70) and the material (A10); four lines of (I7, F11.0) x 4 pairs (ZAIDs of a thermal table);
  NXS(16) and JXS(32) as 8I9 lines; then XSS(NXS(1)) in 4G20.0 lines.
* Binary (type 2): fixed-length direct-access records of `record_length` bytes.  Record
  `location` holds the same header (name A10, awr and kT as float64, date A10, comment A70,
  material A10, 16 x (int32 ZAID, float64 AWR), NXS, JXS as int32); records location + 1, ...
  hold XSS, `entries` float64 words each.  Little-endian.

Neutron tables (JXS / NXS, 1-based positions in XSS):
  ESZ JXS(1): energies, total, absorption, elastic, heating (NXS(3) each); NU JXS(2);
  MTR / LQR / TYR / LSIG JXS(3..6) (NXS(4) reactions, the first NXS(5) emit neutrons);
  SIG JXS(7): [IE, NE, sigma(NE)] per reaction; LAND / AND JXS(8, 9) (elastic + the NXS(5)
  neutron producers); LDLW / DLW JXS(10, 11): chains of [LNW, LAW, IDAT, NR, NBT, INT, NE,
  x(NE), y(NE)] law headers, each with its LDAT block at DLW + IDAT - 1 (also the home of the
  energy-dependent multiplicities, TYR > 100); DNU JXS(24), BDD JXS(25), DNEDL / DNED JXS(26,
  27) for NXS(8) delayed-neutron precursor groups.
Thermal tables: ITIE JXS(1), ITXE JXS(3), ITCE JXS(4), ITCA JXS(6); NXS(3) cosines (discrete
modes: NMU - 1, continuous: NMU + 1), NXS(4) outgoing energies, NXS(5) elastic mode, NXS(6)
elastic cosines - 1, NXS(7) secondary mode.

A table that does not hold together (XSS shorter than NXS(1), a locator outside XSS, a count that
runs past its block) raises ValueError naming the table and the block."""
from __future__ import annotations

import itertools
import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

FISSION_MTS = (18, 19, 20, 21, 38)
ANGLE_ISOTROPIC, ANGLE_32_EQUI, ANGLE_TABULAR = 1, 2, 3
SAB_ELASTIC_DISCRETE = 3
_HEADER_BYTES = 10 + 8 + 8 + 10 + 70 + 10 + 16 * (4 + 8) + 16 * 4 + 32 * 4


@dataclass
class AceTable:
    """One table as it sits in the file: header, NXS, JXS and XSS (XSS[0] is XSS(1))."""
    name: str                       # the A10 field as read (leading blanks kept)
    awr: float
    kT: float
    zaids: list
    nxs: list                       # NXS(1..16) as nxs[0..15]
    jxs: list                       # JXS(1..32) as jxs[0..31]
    xss: np.ndarray = field(repr=False)

    @property
    def kind(self) -> str:
        n = self.name.strip()
        return "neutron" if n.endswith("c") else "thermal" if n.endswith("t") else "other"


class _Xss:
    """1-based, bounds-checked view of XSS that names the table and the block in its errors."""

    def __init__(self, t: AceTable):
        self.t, self.x = t, t.xss

    def fail(self, block: str, what: str):
        raise ValueError(f"ACE table {self.t.name.strip()}: {block}: {what}")

    def word(self, i: int, block: str) -> float:
        if not 1 <= i <= len(self.x):
            self.fail(block, f"position {i} outside XSS (length {len(self.x)})")
        return float(self.x[i - 1])

    def int(self, i: int, block: str) -> int:
        v = self.word(i, block)
        if v != v or abs(v) > 2 ** 31:
            self.fail(block, f"XSS({i}) = {v} is not a count or locator")
        return int(round(v))

    def count(self, i: int, block: str) -> int:
        n = self.int(i, block)
        if n < 0:
            self.fail(block, f"negative count {n} at XSS({i})")
        return n

    def arr(self, i: int, n: int, block: str) -> np.ndarray:
        if n < 0 or i < 1 or i + n - 1 > len(self.x):
            self.fail(block, f"XSS({i}..{i + n - 1}) outside XSS (length {len(self.x)})")
        return self.x[i - 1:i - 1 + n].copy()

    def jxs(self, k: int, block: str) -> int:
        j = self.t.jxs[k - 1]
        if not 1 <= j <= len(self.x):
            self.fail(block, f"JXS({k}) = {j} outside XSS (length {len(self.x)})")
        return j


# ---- reading a table ---------------------------------------------------------------------------
def _f(s: str) -> float:
    s = s.strip().replace("D", "E").replace("d", "e")
    return float(s) if s else 0.0


def _i(s: str) -> int:
    s = s.strip()
    return int(s) if s else 0


def read_table(path, location: int = 1, filetype: str = "ascii", record_length: int = 0,
               entries: int = 0, expect_name: str | None = None) -> AceTable:
    """The table at `location` (ASCII: its first line, 1-based; binary: its first record) of the
    file at `path`.  expect_name: the cross_sections.xml name the header must carry."""
    path = Path(path)
    label = expect_name or f"{path.name}@{location}"
    if location < 1:
        raise ValueError(f"ACE table {label}: location {location} must be at least 1")
    if filetype == "ascii":
        t = _read_ascii(path, location, label)
    elif filetype == "binary":
        t = _read_binary(path, location, record_length, entries, label)
    else:
        raise ValueError(f"ACE table {label}: unknown filetype {filetype!r}")
    if expect_name is not None and t.name.strip() != expect_name.strip():
        raise ValueError(f"ACE table {expect_name}: header: {t.name.strip()!r} found at location {location} instead")
    return t


def _read_ascii(path: Path, location: int, label: str) -> AceTable:
    with open(path, "r") as fh:
        it = itertools.islice(fh, location - 1, None)
        head = list(itertools.islice(it, 12))
        if len(head) < 12:
            raise ValueError(f"ACE table {label}: header: file ends before the header is complete")
        l1 = head[0].rstrip("\n")
        try:
            name, awr, kT = l1[0:10], _f(l1[10:22]), _f(l1[22:34])
            zaids = []
            for line in head[2:6]:
                for k in range(4):
                    zaids.append(_i(line[18 * k:18 * k + 7]))
            nxs = [_i(line[9 * k:9 * k + 9]) for line in head[6:8] for k in range(8)]
            jxs = [_i(line[9 * k:9 * k + 9]) for line in head[8:12] for k in range(8)]
        except ValueError as e:
            raise ValueError(f"ACE table {label}: header: {e}") from None
        n = nxs[0]
        if n <= 0:
            raise ValueError(f"ACE table {label}: NXS: XSS length NXS(1) = {n}")
        vals = []
        for line in itertools.islice(it, (n + 3) // 4):
            vals.extend(line.split())
        if len(vals) < n:
            raise ValueError(f"ACE table {label}: XSS: {len(vals)} of NXS(1) = {n} words present (truncated)")
        try:
            xss = np.array([_f(v) for v in vals[:n]], dtype=np.float64)
        except ValueError as e:
            raise ValueError(f"ACE table {label}: XSS: {e}") from None
    return AceTable(name, awr, kT, zaids, nxs, jxs, xss)


def _read_binary(path: Path, location: int, record_length: int, entries: int, label: str) -> AceTable:
    if record_length < _HEADER_BYTES or entries < 1 or 8 * entries > record_length:
        raise ValueError(f"ACE table {label}: binary files need record_length >= {_HEADER_BYTES} bytes and "
                         f"1 <= entries <= record_length / 8 (got {record_length}, {entries})")
    raw = path.read_bytes()
    at = (location - 1) * record_length
    if at + _HEADER_BYTES > len(raw):
        raise ValueError(f"ACE table {label}: header: record {location} lies past the end of the file")
    h = raw[at:at + _HEADER_BYTES]
    name = h[0:10].decode("ascii", "replace")
    awr, kT = struct.unpack_from("<dd", h, 10)
    pairs = struct.unpack_from("<" + "id" * 16, h, 116)
    zaids = list(pairs[0::2])
    nxs = list(struct.unpack_from("<16i", h, 308))
    jxs = list(struct.unpack_from("<32i", h, 372))
    n = nxs[0]
    if n <= 0:
        raise ValueError(f"ACE table {label}: NXS: XSS length NXS(1) = {n}")
    xss = np.empty(n)
    for r in range((n + entries - 1) // entries):
        j1 = r * entries
        j2 = min(n, j1 + entries)
        off = (location + r) * record_length
        if off + 8 * (j2 - j1) > len(raw):
            raise ValueError(f"ACE table {label}: XSS: file ends at word {j1 + 1} of NXS(1) = {n} (truncated)")
        xss[j1:j2] = np.frombuffer(raw, dtype="<f8", count=j2 - j1, offset=off)
    return AceTable(name, awr, kT, zaids, nxs, jxs, xss)


def write_binary(path, tables, record_length: int = 4096, entries: int = 512) -> list:
    """Write AceTables as one binary (type 2) file; returns each table's first record (its
    `location`).  The inverse of the binary reader, for converting ASCII libraries."""
    if record_length < _HEADER_BYTES or 8 * entries > record_length:
        raise ValueError("record_length must hold the header and `entries` float64 words")
    out, locs = bytearray(), []
    for t in tables:
        locs.append(len(out) // record_length + 1)
        h = bytearray(record_length)
        struct.pack_into("<10sdd10s70s10s", h, 0, t.name.encode()[:10].ljust(10), t.awr, t.kT,
                         b" " * 10, b" " * 70, b" " * 10)
        z = (list(t.zaids) + [0] * 16)[:16]
        struct.pack_into("<" + "id" * 16, h, 116, *[v for k in range(16) for v in (int(z[k]), 0.0)])
        struct.pack_into("<16i", h, 308, *[int(v) for v in t.nxs])
        struct.pack_into("<32i", h, 372, *[int(v) for v in t.jxs])
        out += h
        x = np.asarray(t.xss, dtype="<f8")
        for j1 in range(0, len(x), entries):
            rec = bytearray(record_length)
            chunk = x[j1:j1 + entries].tobytes()
            rec[:len(chunk)] = chunk
            out += rec
    Path(path).write_bytes(bytes(out))
    return locs


# ---- neutron tables ----------------------------------------------------------------------------
def _ldat_length(X: _Xss, lc: int, law: int, block: str) -> int:
    """Words of a law's LDAT block that starts at XSS(lc + 1) (the ACE layout of each law; laws
    the format does not size here -- 22, 24 -- carry no data, as in the reference reader)."""
    d = lambda k: X.count(lc + 1 + k, block)               # LDAT word k (0-based) as a count
    if law in (2, 3, 66):
        return 2
    if law == 1:
        NR = d(0)
        NE = d(1 + 2 * NR)
        return 3 + 2 * NR + NE + 3 * d(2 + 2 * NR + NE) * NE
    if law == 5:
        NR = d(0)
        NE = d(1 + 2 * NR)
        return 3 + 2 * NR + 2 * NE + d(2 + 2 * NR + 2 * NE)
    if law in (7, 9):
        NR = d(0)
        return 3 + 2 * NR + 2 * d(1 + 2 * NR)
    if law == 11:
        NRa = d(0)
        NEa = d(1 + 2 * NRa)
        NRb = d(2 + 2 * (NRa + NEa))
        NEb = d(3 + 2 * (NRa + NEa + NRb))
        return 5 + 2 * (NRa + NEa + NRb + NEb)
    if law == 67:
        NR = d(0)
        NE = d(1 + 2 * NR)
        return 4 + 2 * (NR + NE + d(3 + 2 * NR + 2 * NE))
    if law in (4, 44, 61):
        NR = d(0)
        NE = d(1 + 2 * NR)
        locs = [X.int(lc + 3 + 2 * NR + NE + i, block) for i in range(NE)]
        n = 2 + 2 * NR + 2 * NE
        for i in range(NE):
            if locs[i] in locs[i + 1:]:
                continue                                   # a row shared with a later E_in
            NP = d(n + 1)
            if law == 4:
                n += 2 + 3 * NP
            elif law == 44:
                n += 2 + 5 * NP
            else:
                n += 2 + 4 * NP
                for _ in range(NP):
                    n += 2 + 3 * d(n + 1)
        return n
    return 0


def _rebase(data: np.ndarray, law: int, shift: float) -> None:
    """Laws 4 / 44 / 61 locate their rows (law 61 also its cosine tables) relative to the DLW
    block; the library takes them relative to the law's LDAT: subtract LOCC + header length."""
    if law not in (4, 44, 61):
        return
    NR = int(data[0])
    NE = int(data[1 + 2 * NR])
    at = 2 + 2 * NR + NE
    locs = [int(v) for v in data[at:at + NE]]
    if law == 61:
        n = 2 + 2 * NR + 2 * NE
        for i in range(NE):
            if locs[i] in locs[i + 1:]:
                continue
            NP = int(data[n + 1])
            for j in range(NP):
                k = n + 2 + 3 * NP + j
                if data[k] != 0:
                    data[k] -= shift
            n += 2 + 4 * NP
            for _ in range(NP):
                n += 2 + 3 * int(data[n + 1])
    data[at:at + NE] -= shift


def _law_chain(X: _Xss, base: int, locc: int, block: str) -> list:
    """The laws of one reaction (or one precursor group): base = JXS of the block (DLW / DNED),
    locc the 1-based locator of the first law header relative to it."""
    out, seen = [], set()
    while locc > 0:
        if locc in seen:
            X.fail(block, f"law chain loops back to locator {locc}")
        seen.add(locc)
        h = base + locc - 1
        LNW, LAW, IDAT, NR = (X.int(h + k, block) for k in range(4))
        if NR < 0:
            X.fail(block, f"negative NR {NR}")
        nbt = [X.int(h + 4 + k, block) for k in range(NR)]
        itp = [X.int(h + 4 + NR + k, block) for k in range(NR)]
        NE = X.count(h + 4 + 2 * NR, block)
        pv_x = X.arr(h + 5 + 2 * NR, NE, block)
        pv_y = X.arr(h + 5 + 2 * NR + NE, NE, block)
        lid = 5 + 2 * (NR + NE)
        lc = base + IDAT - 2                               # LDAT word k sits at XSS(lc + 1 + k)
        n = _ldat_length(X, lc, LAW, f"{block} (law {LAW})")
        data = X.arr(lc + 1, n, f"{block} (law {LAW})")
        _rebase(data, LAW, float(locc + lid))
        out.append(dict(law=LAW, data=data, pv_x=pv_x, pv_y=pv_y, pv_nbt=nbt or None, pv_int=itp or None))
        locc = LNW
    return out


def _tab1(X: _Xss, at: int, block: str) -> tuple:
    """[NR, NBT(NR), INT(NR), NE, x(NE), y(NE)] at XSS(at): (length, nbt, int, x, y)"""
    NR = X.count(at, block)
    NE = X.count(at + 1 + 2 * NR, block)
    return (2 + 2 * NR + 2 * NE, [X.int(at + 1 + k, block) for k in range(NR)],
            [X.int(at + 1 + NR + k, block) for k in range(NR)], X.arr(at + 2 + 2 * NR, NE, block),
            X.arr(at + 2 + 2 * NR + NE, NE, block))


def _nu_array(X: _Xss, knu: int, block: str) -> tuple:
    """(LNU, data) of one nu array at XSS(knu): polynomial [NC, C(NC)] or tabular TAB1"""
    lnu = X.int(knu, block)
    if lnu == 1:
        n = X.count(knu + 1, block) + 1
    elif lnu == 2:
        n = _tab1(X, knu + 1, block)[0]
    else:
        X.fail(block, f"LNU = {lnu} (1: polynomial, 2: tabular)")
    return lnu, X.arr(knu + 1, n, block)


def _nu_block(X: _Xss) -> dict | None:
    t = X.t
    if t.jxs[1] == 0:
        return None
    knu = X.jxs(2, "NU")
    if X.word(knu, "NU") > 0:
        nu_t_type, nu_t = _nu_array(X, knu, "NU")
    else:                                                   # prompt first, then total
        nu_t_type, nu_t = _nu_array(X, knu + int(abs(X.word(knu, "NU"))) + 1, "NU")
    nu = dict(nu_t_type=nu_t_type, nu_t_data=nu_t, nu_d_type=0, nu_d_data=np.zeros(0), n_prec=0,
              prec_data=np.zeros(0), delayed=[])
    if t.jxs[23] > 0:
        kd = X.jxs(24, "DNU")
        n = _tab1(X, kd + 1, "DNU")[0]
        npcr = t.nxs[7]
        if npcr < 0:
            X.fail("BDD", f"NXS(8) = {npcr} precursor groups")
        bdd = X.jxs(25, "BDD")
        n_bdd = 0
        for _ in range(npcr):
            n_bdd += 1 + _tab1(X, bdd + n_bdd + 1, "BDD")[0]
        led, ldis = X.jxs(26, "DNEDL"), X.jxs(27, "DNED")
        delayed = []
        for i in range(npcr):
            chain = _law_chain(X, ldis, X.int(led + i, "DNEDL"), "DNED")
            delayed.append(chain[0])                          # one spectrum per precursor group
        nu.update(nu_d_type=2, nu_d_data=X.arr(kd + 1, n, "DNU"), n_prec=npcr,
                  prec_data=X.arr(bdd, n_bdd, "BDD"), delayed=delayed)
    return nu


def neutron(t: AceTable) -> dict:
    """The nuclide dict of AceNuclide.from_desc (+ name, zaid, nu; freegas_cutoff is the
    caller's: cross_sections.xml / ndpp.xml give it in kT).  Reactions: elastic first, then the
    MTR order of the table."""
    X = _Xss(t)
    nxs = t.nxs
    NES, NMT, NMTN = nxs[2], nxs[3], nxs[4]
    if NES < 2 or NMT < 0 or not 0 <= NMTN <= NMT:
        X.fail("NXS", f"NES = {NES}, NTR = {NMT}, NR = {NMTN}")
    esz = X.jxs(1, "ESZ")
    energy = X.arr(esz, NES, "ESZ")
    elastic = X.arr(esz + 3 * NES, NES, "ESZ")
    el = dict(MT=2, Q=0.0, mult=1, thr=1, in_cm=1, sigma=None, adist=None, edists=[])
    rx = []
    if NMT > 0:
        mtr, lqr, tyr = X.jxs(3, "MTR"), X.jxs(4, "LQR"), X.jxs(5, "TYR")
        lsig, sig = X.jxs(6, "LSIG"), X.jxs(7, "SIG")
        for i in range(NMT):
            ty = X.int(tyr + i, "TYR")
            r = dict(MT=X.int(mtr + i, "MTR"), Q=X.word(lqr + i, "LQR"), mult=abs(ty), in_cm=int(ty < 0),
                     adist=None, edists=[])
            loca = X.int(lsig + i, "LSIG")
            r["thr"] = X.int(sig + loca - 1, "SIG")
            n = X.count(sig + loca, "SIG")
            if r["thr"] < 1 or r["thr"] + n - 1 > NES:
                X.fail("SIG", f"MT {r['MT']}: IE = {r['thr']}, NE = {n} outside the {NES}-point grid")
            r["sigma"] = X.arr(sig + loca + 1, n, "SIG")
            if abs(ty) > 100:                                 # energy-dependent yield, in DLW
                _, nbt, itp, x, y = _tab1(X, X.jxs(11, "DLW") + abs(ty) - 101, "DLW (yield)")
                r.update(mult_E=(x, y), mult_E_nbt=nbt, mult_E_int=itp)
            rx.append(r)
    # angular distributions: elastic + the NXS(5) neutron producers
    land, and_ = t.jxs[7], t.jxs[8]
    for k, r in enumerate([el] + rx[:NMTN]):
        if land == 0:
            break
        locb = X.int(X.jxs(8, "LAND") + k, "LAND")
        if locb <= 0:
            continue
        a0 = X.jxs(9, "AND")
        NE = X.count(a0 + locb - 1, "AND")
        e = X.arr(a0 + locb, NE, "AND")
        lcs = [X.int(a0 + locb + NE + j, "AND") for j in range(NE)]
        typ, n = [], 0
        for lc in lcs:
            if lc == 0:
                typ.append(ANGLE_ISOTROPIC)
            elif lc > 0:
                typ.append(ANGLE_32_EQUI)
                n += 33
            else:
                typ.append(ANGLE_TABULAR)
                n += 2 + 3 * X.count(a0 + abs(lc), "AND")
        data = X.arr(a0 + locb + 2 * NE, n, "AND")
        shift = locb + 2 * NE + 1
        loc = np.array([0 if lc == 0 else abs(lc) - shift for lc in lcs], dtype=np.int32)
        r["adist"] = (e, np.array(typ, dtype=np.int32), loc, data)
    # energy distributions of the neutron producers
    for i, r in enumerate(rx[:NMTN]):
        ldlw = X.jxs(10, "LDLW")
        r["edists"] = _law_chain(X, X.jxs(11, "DLW"), X.int(ldlw + i, "LDLW"), f"DLW (MT {r['MT']})")
    fiss = [r for r in rx if r["MT"] in FISSION_MTS]
    return dict(name=t.name, zaid=nxs[1], awr=t.awr, kT=t.kT, energy=energy, elastic=elastic,
                reactions=[el] + rx, nu=_nu_block(X) if fiss else None, fissionable=bool(fiss))


def chi_case(nuc: dict) -> dict:
    """The dict chi_structs takes, from a fissionable neutron() dict: the fission reactions in
    table order with their law chains, the table's fission cross section (the sum of the fission
    reactions, as the ACE reader of NDPP forms it) and the nu / delayed-neutron data."""
    fis = [r for r in nuc["reactions"] if r["MT"] in FISSION_MTS]
    nu = nuc.get("nu")
    if not fis or nu is None:
        raise ValueError(f"ACE table {nuc['name'].strip()}: NU: chi needs fission reactions and nu data")
    n = len(nuc["energy"])
    fission = np.zeros(n)
    for r in fis:
        fission[r["thr"] - 1:r["thr"] - 1 + len(r["sigma"])] += r["sigma"]
    return dict(n_grid=n, energy=nuc["energy"], fission=fission, nu_t_type=nu["nu_t_type"],
                nu_t_data=nu["nu_t_data"], nu_d_type=nu["nu_d_type"], nu_d_data=nu["nu_d_data"],
                n_prec=nu["n_prec"], prec_data=nu["prec_data"], mts=[r["MT"] for r in fis],
                thr=[r["thr"] for r in fis], sig=[r["sigma"] for r in fis],
                nnest=[len(r["edists"]) for r in fis],
                spectra=[(ed["law"], ed["data"], ed) for r in fis for ed in r["edists"]],
                delayed=[(ed["law"], ed["data"], ed) for ed in nu["delayed"]])


# ---- thermal tables ----------------------------------------------------------------------------
def thermal(t: AceTable) -> dict:
    """The dict of SabFlat.from_dict (+ name, awr, kT, zaids): secondary modes 0 (equal), 1
    (skewed) and 2 (continuous), elastic modes 3 (discrete cosines) and 4 (exact, coherent)."""
    X = _Xss(t)
    nxs = t.nxs
    mode = nxs[6]
    if mode not in (0, 1, 2):
        X.fail("NXS", f"secondary mode NXS(7) = {mode} (0, 1 or 2)")
    itie = X.jxs(1, "ITIE")
    NEi = X.count(itie, "ITIE")
    if NEi < 2:
        X.fail("ITIE", f"{NEi} incoming energies")
    ei, sig = X.arr(itie + 1, NEi, "ITIE"), X.arr(itie + 1 + NEi, NEi, "ITIE")
    z1 = np.zeros(1)
    out = dict(name=t.name, awr=t.awr, kT=t.kT, zaids=[z for z in t.zaids if z],
               threshold_inelastic=float(ei[-1]), threshold_elastic=0.0, NEi=NEi, NEo=nxs[3], mode=mode,
               ei=ei, sig=sig, e_out=z1, mu=z1, cptr=np.zeros(NEi + 1, dtype=np.int32), ce_out=z1, cpdf=z1,
               cmu=z1, el_mode=SAB_ELASTIC_DISCRETE, NEe=0, NMUe=0, ee=z1, eP=z1, emu=z1)
    if mode in (0, 1):
        NMU, NEo = nxs[2] + 1, nxs[3]
        if NMU < 1 or NEo < 1:
            X.fail("NXS", f"{NEo} outgoing energies, {NMU} cosines")
        rec = X.arr(X.jxs(3, "ITXE"), NEi * NEo * (1 + NMU), "ITXE").reshape(NEi, NEo, 1 + NMU)
        out.update(NMU=NMU, e_out=rec[:, :, 0].ravel().copy(), mu=rec[:, :, 1:].ravel().copy())
    else:
        NMU = nxs[2] - 1
        if NMU < 1:
            X.fail("NXS", f"{NMU} cosines")
        locc = [X.int(itie + 1 + 2 * NEi + i, "ITXE") for i in range(NEi)]
        counts = [X.count(itie + 1 + 3 * NEi + i, "ITXE") for i in range(NEi)]
        ce, cp, cm = [], [], []
        for i in range(NEi):
            r = X.arr(locc[i] + 1, counts[i] * (3 + NMU), "ITXE").reshape(counts[i], 3 + NMU)
            ce.append(r[:, 0])
            cp.append(r[:, 1])
            cm.append(r[:, 3:].ravel())
        out.update(NMU=NMU, cptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                   ce_out=np.concatenate(ce), cpdf=np.concatenate(cp), cmu=np.concatenate(cm))
    if t.jxs[3] != 0:
        itce = X.jxs(4, "ITCE")
        NEe = X.count(itce, "ITCE")
        ee, eP = X.arr(itce + 1, NEe, "ITCE"), X.arr(itce + 1 + NEe, NEe, "ITCE")
        NMUe = nxs[5] + 1
        if NMUe < 0:
            X.fail("NXS", f"{NMUe} elastic cosines")
        out.update(el_mode=nxs[4], NEe=NEe, NMUe=NMUe, ee=ee, eP=eP, threshold_elastic=float(ee[-1]) if NEe else 0.0)
        if NMUe > 0:
            out["emu"] = X.arr(X.jxs(6, "ITCA"), NEe * NMUe, "ITCA")
    return out
