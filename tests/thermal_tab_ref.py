"""Numpy restatement of the tabular output of a thermal S(alpha,beta) table (TEST INFRASTRUCTURE;
include/ndpp_hip.h, ndpp_sab_tab_batch).  It shares nothing with the kernels: it builds the list of
(E_in, group, cosine, weight) masses of each mode with array operations, drops them into bins with
np.add.at and normalises.  Cosines and interpolation factors are elementwise IEEE operations, so
every mass lands in the bin it lands in on the device; only the order of the sums differs.
Used by test_gpu_thermal_tabular.py and tools/bench_thermal_tabular.py; t is a synth.sab_table dict."""
import math

import numpy as np

ST_NONFINITE, ST_RANGE = 1, 2


def bin_of(mu, N):
    """the bin of a cosine: floor((mu + 1) * (0.5 * N)) clamped to 0 .. N-1; -1 where not finite"""
    mu = np.asarray(mu, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        q = np.floor((mu + 1.0) * (0.5 * N))
    k = np.clip(np.where(np.isfinite(q), q, 0.0), 0, N - 1).astype(np.int64)
    return np.where(np.isfinite(mu), k, -1)


def bracket(grid, v):
    """1-based i with grid[i-1] <= v < grid[i] (v == grid[-1] gives n-1), for v inside the grid"""
    return np.clip(np.searchsorted(grid, v, side="right"), 1, len(grid) - 1)


def weights(t):
    """the discrete modes' weight per outgoing energy (sab.F90:167-186)"""
    NEo, NMU = t["NEo"], t["NMU"]
    if t["mode"] == 0:
        return np.full(NEo, 1.0 / (float(NEo) * float(NMU)))
    w = np.ones(NEo)
    w[[0, -1]] = 0.1
    w[[1, -2]] = 0.4
    return w / (math.fsum(w) * float(NMU))


def _drop(out, status, i, g, mu, w, N):
    """add the masses w (cosines mu, E_in index i, group g: arrays of one shape) to out[i, g, bin]"""
    k = bin_of(mu, N)
    ok = k >= 0
    np.add.at(out, (i[ok], g[ok], k[ok]), w[ok])
    np.bitwise_or.at(status, i[~ok], ST_NONFINITE)


def elastic(t, ein, bins, N, status):
    ein, bins = np.asarray(ein, dtype=np.float64), np.asarray(bins, dtype=np.float64)
    G = len(bins) - 1
    out = np.zeros((len(ein), G, N))
    if t["threshold_elastic"] == 0.0:
        return out
    ee, eP = np.asarray(t["ee"], dtype=np.float64), np.asarray(t["eP"], dtype=np.float64)
    live = (ein >= ee[0]) & (ein < t["threshold_elastic"])
    rng = live & (ein > ee[-1])
    status[rng] |= ST_RANGE
    live &= ~rng & (ein >= bins[0]) & (ein <= bins[G])
    i = np.nonzero(live)[0]
    E = ein[i]
    isab = bracket(ee, E)
    f = (E - ee[isab - 1]) / (ee[isab] - ee[isab - 1])
    g = bracket(bins, E) - 1
    if t["NMUe"] == 0:
        sig = eP[isab - 1] / E if t["el_mode"] == 4 else (1.0 - f) * eP[isab - 1] + f * eP[isab]
        _drop(out, status, i, g, 1.0 - ee[isab - 1] / E, np.ones(len(i)), N)
    elif t["el_mode"] == 3:
        NMU = t["NMUe"]
        emu = np.asarray(t["emu"], dtype=np.float64).reshape(len(ee), NMU)
        sig = (1.0 - f) * eP[isab - 1] + f * eP[isab]
        mu = (1.0 - f)[:, None] * emu[isab - 1] + f[:, None] * emu[isab]
        shape = mu.shape
        _drop(out, status, np.broadcast_to(i[:, None], shape), np.broadcast_to(g[:, None], shape), mu,
              np.full(shape, 1.0 / float(NMU)), N)
    else:
        return out
    out[i] = sig[:, None, None] * out[i]
    return out


def inelastic_discrete(t, ein, bins, N, status):
    ein, bins = np.asarray(ein, dtype=np.float64), np.asarray(bins, dtype=np.float64)
    G, NEi, NEo, NMU = len(bins) - 1, t["NEi"], t["NEo"], t["NMU"]
    ei, sg = np.asarray(t["ei"], dtype=np.float64), np.asarray(t["sig"], dtype=np.float64)
    eo = np.asarray(t["e_out"], dtype=np.float64).reshape(NEi, NEo)
    mus = np.asarray(t["mu"], dtype=np.float64).reshape(NEi, NEo, NMU)
    thr = t["threshold_inelastic"]
    out = np.zeros((len(ein), G, N))
    below, at = ein < ei[0], ein == thr
    rng = ~below & (ein < thr) & (ein > ei[-1])
    status[rng] |= ST_RANGE
    i = np.nonzero((ein <= thr) & ~rng)[0]
    E = ein[i]
    isab = np.where(below[i], 1, np.where(at[i], NEi - 1, bracket(ei, E)))
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(below[i], 0.0, np.where(at[i], 1.0, (E - ei[isab - 1]) / (ei[isab] - ei[isab - 1])))
    sig = (1.0 - f) * sg[isab - 1] + f * sg[isab]
    Eout = (1.0 - f)[:, None] * eo[isab - 1] + f[:, None] * eo[isab]                       # [n][NEo]
    ok = (Eout >= bins[0]) & (Eout < bins[G])
    g = bracket(bins, Eout) - 1
    mu = (1.0 - f)[:, None, None] * mus[isab - 1] + f[:, None, None] * mus[isab]           # [n][NEo][NMU]
    shape = mu.shape
    sel = np.broadcast_to(ok[:, :, None], shape)
    _drop(out, status, np.broadcast_to(i[:, None, None], shape)[sel], np.broadcast_to(g[:, :, None], shape)[sel],
          mu[sel], np.broadcast_to(weights(t)[None, :, None], shape)[sel], N)
    out[i] = sig[:, None, None] * out[i]
    return out


def continuous_rows(t, bins, N):
    """stage 1 (sab.F90:292-378): per table E_in and group the masses of the lower edge term, the
    upper edge term and the interior points, / NMU.  Returns distro[NEi][G][N] and, per table row,
    whether a cosine that is not finite was among them."""
    bins = np.asarray(bins, dtype=np.float64)
    G, NEi, NMU = len(bins) - 1, t["NEi"], t["NMU"]
    ptr = np.asarray(t["cptr"])
    distro = np.zeros((NEi, G, N))
    lost = np.zeros(NEi, dtype=bool)
    for k in range(NEi):
        Eo = np.asarray(t["ce_out"], dtype=np.float64)[ptr[k]:ptr[k + 1]]
        pd = np.asarray(t["cpdf"], dtype=np.float64)[ptr[k]:ptr[k + 1]]
        mu = np.asarray(t["cmu"], dtype=np.float64).reshape(-1, NMU)[ptr[k]:ptr[k + 1]]
        NP = len(Eo)
        pdfw = np.concatenate([pd[:-1] * (Eo[1:] - Eo[:-1]), [0.0]])       # pdf(j), j = 1 .. NP, at [j-1]
        for g in range(G):
            eg, eg1 = bins[g], bins[g + 1]
            ms, ws = [], []
            if eg < Eo[0]:
                lo = 1
            elif eg >= Eo[-1]:
                continue
            else:
                j = int(bracket(Eo, eg))
                f = (eg - Eo[j - 1]) / (Eo[j] - Eo[j - 1])
                ms.append((1.0 - f) * mu[j - 1] + f * mu[j])
                ws.append(np.full(NMU, f * pdfw[j - 1]))
                lo = j + 1
            if eg1 < Eo[0]:
                continue
            elif eg1 >= Eo[-1]:
                hi = NP - 1
            else:
                j = int(bracket(Eo, eg1))
                f = (eg1 - Eo[j - 1]) / (Eo[j] - Eo[j - 1])
                ms.append((1.0 - f) * mu[j - 1] + f * mu[j])
                ws.append(np.full(NMU, f * pdfw[j - 1]))
                hi = j - 1
            if hi >= lo:
                ms.append(mu[lo - 1:hi].ravel())
                ws.append(np.repeat(pdfw[lo - 1:hi], NMU))
            m, w = np.concatenate(ms), np.concatenate(ws)
            kb = bin_of(m, N)
            lost[k] |= bool((kb < 0).any())
            np.add.at(distro[k, g], kb[kb >= 0], w[kb >= 0])
            distro[k, g] = distro[k, g] / float(NMU)
    return distro, lost


def inelastic_continuous(t, ein, bins, N, status):
    ein = np.asarray(ein, dtype=np.float64)
    ei, sg = np.asarray(t["ei"], dtype=np.float64), np.asarray(t["sig"], dtype=np.float64)
    thr = t["threshold_inelastic"]
    distro, lost = continuous_rows(t, bins, N)
    out = np.zeros((len(ein),) + distro.shape[1:])
    low = ein <= ei[0]
    out[low] = distro[0] * sg[0]
    status[low & lost[0]] |= ST_NONFINITE
    mid = ~low & (ein < thr)
    rng = mid & (ein > ei[-1])
    status[rng] |= ST_RANGE
    i = np.nonzero(mid & ~rng)[0]
    isab = bracket(ei, ein[i])
    f = (ein[i] - ei[isab - 1]) / (ei[isab] - ei[isab - 1])
    sig = (1.0 - f) * sg[isab - 1] + f * sg[isab]
    out[i] = ((1.0 - f)[:, None, None] * distro[isab - 1] + f[:, None, None] * distro[isab]) * sig[:, None, None]
    status[i[lost[isab - 1] | lost[isab]]] |= ST_NONFINITE
    return out


def combine(el, inel):
    """combine_sab_grid with the bin sums for P0: rows scaled by 1 / sum over (g, k); the last point
    copies its neighbour"""
    tot = el + inel
    mat = np.zeros_like(tot)
    for i in range(len(tot)):
        s = math.fsum(tot[i].ravel())
        if s > 0.0:
            mat[i] = tot[i] * (1.0 / s)
    if len(mat) >= 2:
        mat[-1] = mat[-2]
    return mat


def sab_tab(t, ein, bins, N):
    """(scatt_mat, el, inel, status), each as ndpp_sab_tab_batch returns it"""
    status = np.zeros(len(ein), dtype=np.int32)
    el = elastic(t, ein, bins, N, status)
    inel = (inelastic_continuous if t["mode"] == 2 else inelastic_discrete)(t, ein, bins, N, status)
    return combine(el, inel), el, inel, status


def masses_per_bin(t):
    """the largest number of masses one bin can receive: (inelastic, elastic)"""
    n_in = (int(np.diff(t["cptr"]).max()) if t["mode"] == 2 else t["NEo"]) * t["NMU"]
    n_el = 0 if t["threshold_elastic"] == 0.0 else max(t["NMUe"], 1)
    return n_in, n_el
