"""The host half every batch entry point shares, no GPU needed: one table over the entry points,
and for each the same calls -- its leading pointer NULL (-22), one row_lo out of range (-22, the
message names row_lo), for law 9 a bad NR in edata (-22), and valid arguments, which on a machine
without a device are the device error (-5): an invalid argument is reported before the missing
device is."""
import ctypes as C

import numpy as np
import pytest

from conftest import dp, ip
from synth import chi_case, sab_table

M = 65
BINS = np.array([0.0, 1.0, 20.0])
EDATA = np.array([0, 2, 1e-5, 20.0, 1e-6, 1e-6, 0.0])


def _elastic_like(hip):
    p = hip.Params.default(4, M)
    ein, row, w = np.array([1.0, 2.0]), np.zeros(2, np.int32), np.array([0.5, 0.25])
    f, out, st = np.full((2, M), 0.5), np.zeros(2 * 2 * 8), np.zeros(2, np.int32)
    return p, ein, row, w, f, out, st


def _file6(hip, n_tab):
    p, ein, row, _, _, out, st = _elastic_like(hip)
    eg, rp = np.array([1e-5, 20.0]), np.array([0, 2, 4], np.int32)
    eo, pd, it, ff = np.array([0.0, 1.0, 0.0, 1.0]), np.ones(4), np.array([2, 2], np.int32), np.full((4, M), 0.5)
    hold = (p, ein, row, eg, rp, eo, pd, it, ff, out, st)
    head = [C.byref(p)] + ([n_tab] if n_tab else [])
    args = head + [12.0, 1, 2, dp(ein), ip(row), 2, dp(eg), ip(rp), dp(eo), dp(pd), ip(it), dp(ff), 2, dp(BINS),
                   dp(out), ip(st)]
    return hold, args, dict(row_lo=len(head) + 4)


def _law9(hip, n_tab):
    p, ein, row, w, f, out, st = _elastic_like(hip)
    hold = (p, ein, row, w, f, out, st)
    head = [C.byref(p)] + ([n_tab] if n_tab else [])
    args = head + [2, dp(ein), ip(row), dp(w), 2, dp(f), len(EDATA), dp(EDATA), 2, dp(BINS), dp(out), ip(st)]
    return hold, args, dict(row_lo=len(head) + 2, edata=len(head) + 7)


def _elastic_tab(hip):
    p, ein, row, w, f, out, st = _elastic_like(hip)
    hold = (p, ein, row, w, f, out, st)
    args = [C.byref(p), 8, 1.0, 2.5e-8, 0.0, 0.0, 2, dp(ein), ip(row), dp(w), 2, dp(f), 2, dp(BINS), dp(out), ip(st),
            None]
    return hold, args, dict(row_lo=8)


def _sab(hip):
    p = hip.Params.default(4, M)
    t = hip.SabFlat.from_dict(sab_table(0, 1))
    ein, mat = np.array([1e-8, 1e-7]), np.zeros(2 * 2 * 4)
    return (p, t, ein, mat), [C.byref(p), C.byref(t), 2, dp(ein), 2, dp(BINS), None, None, dp(mat)], {}


def _sab_tab(hip):
    p = hip.Params.default(4, M)
    t = hip.SabFlat.from_dict(sab_table(0, 1))
    ein, mat = np.array([1e-8, 1e-7]), np.zeros(2 * 2 * 8)
    return (p, t, ein, mat), [C.byref(p), C.byref(t), 8, 2, dp(ein), 2, dp(BINS), None, None, dp(mat), None], {}


def _chi(hip):
    c = chi_case()
    nuc, PA, npr, DA, nd, keep = hip.chi_structs(c)
    bins, grid = np.ascontiguousarray(c["bins"], dtype=np.float64), np.array([1e-6, 1.0])
    G = len(bins) - 1
    ct, cp, cd = np.zeros((2, G)), np.zeros((2, G)), np.zeros((max(nd, 1), 2, G))
    hold = (nuc, PA, DA, keep, bins, grid, ct, cp, cd)
    return hold, [C.byref(nuc), npr, PA, nd, DA, G, dp(bins), 2, dp(grid), dp(ct), dp(cp), dp(cd)], {}


def _convert(hip):
    rxn = hip.AceReaction.make(2, 0, None)          # the fabricated isotropic two-point table
    is_init, law, NE, tot = hip.scattdata_shape(rxn)
    assert (is_init, NE, tot) == (1, 2, 2)
    eg, rp, it = np.zeros(NE), np.zeros(NE + 1, np.int32), np.zeros(NE, np.int32)
    eo, pd, cd, f = np.zeros(tot), np.zeros(tot), np.zeros(tot), np.zeros((tot, 5))
    hold = (rxn, eg, rp, it, eo, pd, cd, f)
    return hold, [5, C.byref(rxn), 2, dp(BINS), NE, tot, dp(eg), ip(rp), dp(eo), dp(pd), dp(cd), ip(it), dp(f)], \
        dict(null=1)


def _expand(hip):
    m, mu, o = np.ones((2, 4)), np.linspace(-1, 1, 21), np.zeros((2, 21))
    return (m, mu, o), [2, 4, dp(m), 4, 21, dp(mu), dp(o)], dict(null=2)


def _rows(n, G, L, seed):
    rng = np.random.default_rng(seed)
    return np.geomspace(1.0, 16.0, n), rng.uniform(0.5, 1.5, (n, G, L))


def _grid(hip):
    x, y = _rows(5, 2, 3, 1)
    xm, ym = np.sqrt(x[1:] * x[:-1]), 0.5 * (y[1:] + y[:-1])
    err, arg = np.zeros(4), np.zeros(4, np.int32)
    return (x, y, xm, ym, err, arg), [3, 2, 5, dp(x), dp(y), dp(xm), dp(ym), dp(err), ip(arg)], dict(null=3)


def _thin(hip):
    x, y = _rows(5, 2, 3, 2)
    kept, n_kept, max_err = np.zeros(5, np.int32), np.zeros(1, np.int32), np.zeros(1)
    hold = (x, y, kept, n_kept, max_err)
    return hold, [3, 2, 5, dp(x), dp(y), None, 0, None, 1e-3, 4, ip(kept), ip(n_kept), dp(max_err)], dict(null=3)


def _compare(hip):
    xa, ya = _rows(5, 2, 3, 3)
    xb, yb = _rows(4, 2, 2, 4)
    xq, err, arg = np.array([1.5, 3.0, 9.0]), np.zeros(3), np.zeros(3, np.int32)
    hold = (xa, ya, xb, yb, xq, err, arg)
    return hold, [2, 3, 2, 5, dp(xa), dp(ya), 4, dp(xb), dp(yb), 3, dp(xq), dp(err), ip(arg), None], dict(null=4)


ENTRIES = {
    "ndpp_file6_leg_batch": lambda hip: _file6(hip, 0),
    "ndpp_file6_tab_batch": lambda hip: _file6(hip, 8),
    "ndpp_law9_leg_batch": lambda hip: _law9(hip, 0),
    "ndpp_law9_tab_batch": lambda hip: _law9(hip, 8),
    "ndpp_elastic_tab_batch": _elastic_tab,
    "ndpp_sab_batch": _sab,
    "ndpp_sab_tab_batch": _sab_tab,
    "ndpp_chi_batch": _chi,
    "ndpp_convert_distro": _convert,
    "ndpp_expand_moments": _expand,
    "ndpp_grid_error": _grid,
    "ndpp_thin_bounded": _thin,
    "ndpp_lib_compare": _compare,
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_batch_entry_refuses_before_the_device(hip, name):
    lib = hip.load()
    fn = getattr(lib, name)
    hold, args, pos = ENTRIES[name](hip)

    def call(at, value):
        a = list(args)
        a[at] = value
        return fn(*a)

    # the params, or where an entry point has none its leading array or structure
    assert call(pos.get("null", 0), None) == -22
    if "row_lo" in pos:
        for bad in ([0, 1], [-1, 0]):                        # n_rows = 2: only row 0 has a row above it
            rows = np.array(bad, np.int32)
            assert call(pos["row_lo"], ip(rows)) == -22
            assert b"row_lo" in lib.ndpp_last_error()
    if "edata" in pos:
        for nr in (-1.0, 3.0):                               # 2 + 2 NR words do not fit the 7 of EDATA
            ed = EDATA.copy()
            ed[0] = nr
            assert call(pos["edata"], dp(ed)) == -22
            assert b"NR" in lib.ndpp_last_error()
    if lib.ndpp_device_count() == 0:
        assert fn(*args) == -5
        assert b"no HIP device" in lib.ndpp_last_error()
    del hold


@pytest.mark.parametrize("n_tab", (0, 8))
def test_sab_entries_refuse_a_bad_cont_ptr_before_the_device(hip, n_tab):
    """A continuous table whose cont_ptr is missing, or does not start at 0, is an invalid argument for
    both thermal entry points, device or none."""
    lib = hip.load()
    p = hip.Params.default(4, M)
    t = hip.SabFlat.from_dict(sab_table(2, 1))
    ein, mat = np.array([1e-8, 1e-7]), np.zeros(2 * 2 * 8)
    fn = lib.ndpp_sab_tab_batch if n_tab else lib.ndpp_sab_batch
    args = [C.byref(p), C.byref(t)] + ([n_tab] if n_tab else []) + [2, dp(ein), 2, dp(BINS), None, None, dp(mat)] + \
        ([None] if n_tab else [])
    ptr = np.ctypeslib.as_array(t.cont_ptr, shape=(t.n_inelastic_e_in + 1,))
    ptr[0] = 1
    assert fn(*args) == -22 and b"cont_ptr[0] must be 0" in lib.ndpp_last_error()
    ptr[0] = 0
    t.cont_ptr = None
    assert fn(*args) == -22 and b"continuous mode without cont_ptr" in lib.ndpp_last_error()
