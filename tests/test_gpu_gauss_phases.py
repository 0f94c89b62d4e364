"""The free-gas Gauss stage run by phases (fg_device.h fg_gauss_phased_kernel, the default) against
the previous kernel, one candidate per lane (NDPP_HIP_GAUSS_PHASED=0): the same phase functions
(fg_pipeline.h mu_gauss_phase), so the same decisions, rows and values whichever candidates share a
wave.  Needs a real MI355X:  pytest -m gpu"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

STRICT_LIB = os.environ.get("NDPP_HIP_STRICT") == "1"   # no Gauss stage in the reference arithmetic


def headline_slice(n, L, groups=None):
    """n points of the headline's 1e5-point grid (H-1, M = 2001), L orders; `groups` equal-lethargy
    groups instead of the headline's two."""
    sys.path.insert(0, str(ROOT))
    import bench
    wl = bench.make_workload(100000, 6)
    sel = np.unique(np.linspace(0, 99999, n).astype(np.int64))
    bins = wl["bins"] if groups is None else np.concatenate([[0.0], np.geomspace(1e-11, 20.0, groups)])
    return L, (wl["A"], wl["kT"], 1e300, 0.0, wl["ein"][sel], wl["row_lo"][sel], wl["w_hi"][sel],
               wl["f_tab"], bins)


def run(hip, monkeypatch, case, **env):
    L, args = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out, status, st = hip.elastic_leg_batch(hip.Params.default(L, args[7].shape[1]), *args, want_stats=True)
    for k in env:
        monkeypatch.delenv(k)
    assert (status == 0).all()
    return out, st


CASES = {
    "headline_p5": lambda: headline_slice(4096, 6),
    "p7_g70": lambda: headline_slice(512, 8, groups=70),
    "p10_single_row": lambda: headline_slice(1024, 11),     # L > 8: one row per job (R = 1)
}


@pytest.mark.skipif(STRICT_LIB, reason="the Gauss stage belongs to the product arithmetic")
@pytest.mark.parametrize("name", sorted(CASES))
def test_phased_gauss_stage_has_the_bits_of_the_lane_per_candidate_kernel(hip, monkeypatch, name):
    case = CASES[name]()
    new, st_new = run(hip, monkeypatch, case)
    old, st_old = run(hip, monkeypatch, case, NDPP_HIP_GAUSS_PHASED="0")
    print(f"{name}: {st_new.gauss_integrals} integrals by the rule; Gauss stage {st_old.gauss_ms:.1f} ms "
          f"-> {st_new.gauss_ms:.1f} ms")
    assert st_new.gauss_integrals > 0
    assert np.array_equal(new, old)
    assert st_new.gauss_integrals == st_old.gauss_integrals and st_new.k_evals == st_old.k_evals


@pytest.mark.skipif(STRICT_LIB, reason="the Gauss stage belongs to the product arithmetic")
def test_phased_gauss_stage_joint_single_row_and_split_have_the_same_bits(hip, monkeypatch):
    """A row's result does not depend on the other row of its job (joint == single-row), nor on
    whether the walk after the stage splits its integrals (split == unsplit)."""
    case = headline_slice(2048, 6)
    joint, _ = run(hip, monkeypatch, case)
    single, _ = run(hip, monkeypatch, case, NDPP_HIP_NO_JOINT="1")
    assert np.array_equal(joint, single)
    g = load_golden("freegas_h1_p5")
    small = (int(g["L"]), (float(g["A"]), float(g["kT"]), 1e300, 0.0, g["ein"], g["row_lo"], g["w_hi"],
                           g["f_tab"], g["bins"]))
    one, st1 = run(hip, monkeypatch, small, NDPP_HIP_NO_SPLIT="1")
    many, st16 = run(hip, monkeypatch, small, NDPP_HIP_NO_SPLIT="0")
    old, _ = run(hip, monkeypatch, small, NDPP_HIP_NO_SPLIT="0", NDPP_HIP_GAUSS_PHASED="0")
    assert st1.gauss_integrals > 0 and st1.gauss_integrals == st16.gauss_integrals
    assert np.array_equal(one, many) and np.array_equal(many, old)
