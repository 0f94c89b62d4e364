"""Tabular scattering output, host side (no GPU): refusals, the no-device path, and the output
chain -- tolerance rule, gmin/gmax trim, BINARY / ASCII writers, header -- on hand-made tabular
matrices, read back with reader.py."""
import numpy as np
import pytest

from ndpp_amd import reader, validate

N_BAD = (0, -1, 129)


def _p(hip):
    return hip.Params.default(4, 65)


def _f_tab():
    return np.full((2, 65), 0.5)


def test_constants(hip):
    assert (hip.SCATT_LEGENDRE, hip.SCATT_TABULAR, hip.MAX_TAB_BINS) == (0, 1, 128)
    assert (reader.SCATT_TYPE_LEGENDRE, reader.SCATT_TYPE_TABULAR) == (0, 1)


@pytest.mark.parametrize("n_tab", N_BAD)
def test_bin_count_refused_by_every_entry(hip, n_tab):
    import ctypes as C
    p = _p(hip)
    lib = hip.load()
    ein, row, w, bins = np.array([1.0]), np.zeros(1, np.int32), np.array([0.5]), np.array([0.0, 1.0, 20.0])
    f = _f_tab()
    out = np.zeros(64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.ndpp_elastic_tab_batch(C.byref(p), n_tab, 1.0, 2.5e-8, 0.0, 0.0, 1, dp(ein), ip(row), dp(w), 2, dp(f),
                                      2, dp(bins), dp(out), None, None) == -22
    assert b"n_tab" in lib.ndpp_last_error()
    edata = np.array([0, 2, 1e-5, 20.0, 1e-6, 1e-6, 0.0])
    assert lib.ndpp_law9_tab_batch(C.byref(p), n_tab, 1, dp(ein), ip(row), dp(w), 2, dp(f), len(edata), dp(edata),
                                   2, dp(bins), dp(out), None) == -22
    eg, rp = np.array([1e-5, 20.0]), np.array([0, 2, 4], np.int32)
    eo, pd, it, ff = np.array([0.0, 1.0, 0.0, 1.0]), np.ones(4), np.array([2, 2], np.int32), np.full((4, 65), 0.5)
    assert lib.ndpp_file6_tab_batch(C.byref(p), n_tab, 12.0, 1, 1, dp(ein), ip(row), 2, dp(eg), ip(rp), dp(eo),
                                    dp(pd), ip(it), dp(ff), 2, dp(bins), dp(out), None) == -22
    with pytest.raises(hip.NdppError):
        hip.elastic_tab_batch(p, n_tab, 1.0, 2.5e-8, 0.0, 0.0, ein, row, w, f, bins)
    from synth import nuclide_case
    c = nuclide_case()
    with pytest.raises(hip.NdppError, match="-22"):
        hip.scatt_nuclide_tab(p, n_tab, c, c["bins"])
    with pytest.raises(hip.NdppError, match="-22"):
        hip.scatt_library_tab(p, n_tab, [c], c["bins"])


def test_null_pointers_refused(hip):
    import ctypes as C
    p = _p(hip)
    lib = hip.load()
    ein, bins = np.array([1.0]), np.array([0.0, 1.0, 20.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ndpp_elastic_tab_batch(None, 8, 1.0, 2.5e-8, 0.0, 0.0, 1, dp(ein), None, None, 2, None, 2, dp(bins),
                                      None, None, None) == -22
    assert lib.ndpp_elastic_tab_batch(C.byref(p), 8, 1.0, 2.5e-8, 0.0, 0.0, 1, dp(ein), None, None, 2, None, 2,
                                      dp(bins), None, None, None) == -22
    assert lib.ndpp_law9_tab_batch(C.byref(p), 8, 1, None, None, None, 2, None, 7, None, 2, None, None, None) == -22
    assert lib.ndpp_file6_tab_batch(C.byref(p), 8, 12.0, 0, 1, None, None, 2, None, None, None, None, None, None,
                                    2, None, None, None) == -22
    assert lib.ndpp_file6_tab_batch(None, 8, 12.0, 0, 1, None, None, 2, None, None, None, None, None, None,
                                    2, None, None, None) == -22
    assert lib.ndpp_scatt_nuclide_tab(C.byref(p), 8, None, 3, dp(bins), 0, None) == -22
    assert lib.ndpp_scatt_library_tab(C.byref(p), 8, 1, None, 3, dp(bins), 0, None) == -22


def test_no_device_path(hip):
    if hip.load().ndpp_device_count() > 0:
        pytest.skip("a device is present: the compute paths run (tests/test_gpu_tabular.py)")
    p = _p(hip)
    ein, row, w, bins = np.array([1.0]), np.zeros(1, np.int32), np.array([0.5]), np.array([0.0, 1.0, 20.0])
    with pytest.raises(hip.NdppError, match="-5"):
        hip.elastic_tab_batch(p, 8, 1.0, 2.5e-8, 0.0, 0.0, ein, row, w, _f_tab(), bins)
    with pytest.raises(hip.NdppError, match="-5"):
        hip.law9_tab_batch(p, 8, ein, row, w, _f_tab(), [0, 2, 1e-5, 20.0, 1e-6, 1e-6, 0.0], bins)
    with pytest.raises(hip.NdppError, match="-5"):
        hip.file6_tab_batch(p, 8, 12.0, 1, ein, row, [1e-5, 20.0], [0, 2, 4], [0.0, 1.0, 0.0, 1.0], np.ones(4),
                            [2, 2], np.full((4, 65), 0.5), bins)
    from synth import nuclide_case
    c = nuclide_case()
    pp = hip.Params.default(c["order"] + 1, c["mu_bins"])
    with pytest.raises(hip.NdppError, match="-5"):
        hip.scatt_nuclide_tab(pp, 8, c, c["bins"])
    with pytest.raises(hip.NdppError, match="-5"):
        hip.scatt_library_tab(pp, 8, [c], c["bins"])


# ---- output chain on hand-made tabular matrices ----------------------------------------------
N, G = 4, 4
BINS = np.array([1e-11, 1e-6, 1e-3, 1.0, 20.0])


def hand_made():
    """Two elastic rows, three inelastic rows.  Elastic row 0: edge groups 0 and 3 have bin 0 equal
    to 0 but a positive bin sum (a P0-only test would trim them); group 3's sum is below the
    tolerance.  Inelastic row 1 is all zero."""
    el = np.zeros((2, G, N))
    el[0, 0] = [0.0, 0.1, 0.2, 0.05]
    el[0, 1] = [0.1, 0.1, 0.1, 0.1]
    el[0, 2] = [0.05, 0.05, 0.1, 0.1]
    el[0, 3] = [0.0, 0.0, 0.0, 5e-9]
    el[1, 1] = [0.2, 0.3, 0.3, 0.2]
    inel = np.zeros((3, G, N))
    inel[0, 2] = [0.0, 0.0, 0.5, 0.5]
    inel[2, 0] = [0.0, 0.25, 0.25, 0.0]
    inel[2, 3] = [0.1, 0.1, 0.1, 0.2]
    return dict(ein_el=np.array([1e-8, 10.0]), el_mat=el, ein_inel=np.array([1.0, 5.0, 10.0]), inel_mat=inel,
                nuinel_mat=2.0 * inel)


def opts(hip, fmt, scatt_type=1, tol=1e-8):
    return hip.OutputOptions(lib_format=fmt, scatt_type=scatt_type, scatt_order=N, nuscatter=1, integrate_chi=0,
                             mu_bins=2001, print_tol=tol, thin_tol=0.0)


def test_finish_scatt_tabular_tolerance_on_bin_sums(hip):
    r = hand_made()
    fin, _ = hip.finish_scatt(opts(hip, hip.FMT_BINARY), r, BINS)
    el = fin["el_mat"]
    # group 3 of row 0 (bin sum 5e-9 < 1e-8) is zeroed and the row renormalised to its total
    assert (el[0, 3] == 0).all()
    tot = r["el_mat"][0].sum()
    assert abs(el[0].sum() - tot) < 1e-15
    assert np.allclose(el[0, :3], r["el_mat"][0, :3] * tot / r["el_mat"][0, :3].sum(), rtol=1e-15, atol=0)
    # group 0 (bin 0 = 0, bin sum 0.35) stays: tested on the bin sum, not on bin 0
    assert el[0, 0].sum() > 0.3
    assert np.array_equal(fin["inel_mat"], r["inel_mat"])


@pytest.mark.parametrize("fmt", ["binary", "ascii"])
def test_tabular_file_trim_header_and_read_back(hip, fmt):
    f = hip.FMT_BINARY if fmt == "binary" else hip.FMT_ASCII
    o = opts(hip, f, tol=0.0)
    r = hand_made()
    data = hip.nuclide_file(o, "%10s" % "1001.71c", 2.53e-8, r, BINS)
    t = (reader.read_binary if fmt == "binary" else reader.read_ascii)(data)
    assert t.scatt_type == 1 and t.scatt_order == N and t.moments == N and t.groups == G
    # gmin / gmax from the bin sums: row 0 keeps groups 1..4 although bin 0 of groups 1 and 4 is 0
    assert list(t.elastic.gmin) == [1, 2] and list(t.elastic.gmax) == [4, 2]
    assert list(t.inelastic.gmin) == [3, 0, 1] and list(t.inelastic.gmax) == [3, 0, 4]
    if fmt == "binary":
        assert np.array_equal(t.elastic.mat, r["el_mat"])
        assert np.array_equal(t.inelastic.mat, r["inel_mat"])
        assert np.array_equal(t.nuinelastic.mat, r["nuinel_mat"])
    else:
        assert np.allclose(t.elastic.mat, r["el_mat"], rtol=1e-12, atol=0)
        assert np.allclose(t.nuinelastic.mat, r["nuinel_mat"], rtol=1e-12, atol=0)
    # the same matrices written as Legendre rows (P3: 4 moments) trim on the first entry, P0
    leg_opts = opts(hip, hip.FMT_BINARY, scatt_type=0, tol=0.0)
    leg_opts.scatt_order = N - 1
    leg = reader.read_binary(hip.nuclide_file(leg_opts, "%10s" % "1001.71c",
                                              2.53e-8, r, BINS)) if fmt == "binary" else None
    if leg is not None:
        assert leg.scatt_type == 0 and list(leg.elastic.gmin) == [2, 2] and list(leg.elastic.gmax) == [3, 2]


def test_thermal_table_as_tabular_refused(hip):
    o = opts(hip, hip.FMT_BINARY)
    r = hand_made()
    r = dict(r, ein_inel=None, inel_mat=None, nuinel_mat=None)
    with pytest.raises(hip.NdppError, match="S\\(alpha,beta\\)"):
        hip.nuclide_file(o, "hh2o.71t", 2.53e-8, r, BINS, is_sab=True)
    assert hip.load().ndpp_last_error().startswith(b"nuclide_file: tabular")


def test_validate_counts_negative_and_nan_bins(hip, tmp_path, capsys):
    r = hand_made()
    r["el_mat"][1, 1, 2] = -1e-3
    r["inel_mat"][2, 3, 1] = np.nan
    rep = validate.tab_positivity(r)
    assert rep.sections["elastic"].negative == 1 and rep.sections["elastic"].offending == [(1, 1)]
    assert rep.sections["elastic"].offending_mu == [2] and rep.sections["elastic"].min_value == -1e-3
    assert rep.sections["inelastic"].negative == 1 and rep.sections["inelastic"].offending == [(2, 3)]
    assert rep.sections["inelastic"].rows == 3 * G and not rep.positive and rep.n_moments == N
    assert validate.tab_positivity(hand_made()).positive
    # the CLI on a written tabular library: exit 1 with the offending rows, 0 once they are gone
    for bad, want in ((r, 1), (hand_made(), 0)):
        o = opts(hip, hip.FMT_BINARY, tol=0.0)
        (tmp_path / "1001.71c").write_bytes(hip.nuclide_file(o, "%10s" % "1001.71c", 2.53e-8, bad, BINS))
        (tmp_path / "ndpp_lib.xml").write_bytes(hip.lib_xml(
            str(tmp_path), hip.FMT_BINARY, [dict(alias="1001.71c", awr=0.99917, name="1001.71c", path="1001.71c",
                                                kT=2.53e-8, zaid=1001, metastable=0, freegas_cutoff=0.0)],
            BINS, 1, N, 2001, 1, 0, 0.0, 0.0))
        assert validate.main([str(tmp_path)]) == want
        out = capsys.readouterr().out
        assert "tabular" in out and (want == 0 or "negative       1" in out)


def test_reader_sizes_tabular_rows():
    """reader.py's n_moments rule: N entries per group for tabular, scatt_order + 1 for Legendre"""
    t = reader.NdppTable("x", 0.0, BINS, 1, 7, False, False, 2001, 0.0)
    assert t.moments == 7
    assert reader.NdppTable("x", 0.0, BINS, 0, 7, False, False, 2001, 0.0).moments == 8
