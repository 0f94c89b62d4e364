"""ndpp_amd -- MI355X (gfx950) implementation of NDPP's scattering-moment
integration hot path, behind a C ABI (include/ndpp_hip.h)."""
from .lib import (_check, Params, Stats, NdppError, load, library_path, mu_grid,  # noqa: F401
                  integrate_freegas_leg, integrate_file4_cm_leg,
                  elastic_leg_batch, elastic_leg_batch_device,
                  file6_leg_batch, law9_leg_batch, SabFlat, sab_batch, apply_tol_scatt, ChiSpectrum, ChiNuclide,
                  chi_structs, chi_batch, AceReaction, scattdata_shape, convert_distro,
                  SdGrid, merge_grids, create_ein_grid, AceNuclide, scatt_nuclide, scatt_library,
                  elastic_leg_multi, elastic_leg_multi_device,
                  group_index, scatt_wire, chi_wire, header_wire, DeviceArray, thin_grid, sab_egrid_lib, chi_egrid_lib,
                  OutputOptions, FMT_ASCII, FMT_BINARY, FMT_NONE, scatt_ascii, chi_ascii, header_ascii,
                  real_to_str, ascii_array, lib_xml, finish_scatt, nuclide_file,
                  set_device, freegas_rough_rows, mapped_runtimes, profile_reset, profile_get,
                  ST_NONFINITE, ST_RANGE, ST_ORDER_NOISE,
                  Positivity, scatt_positivity, expand_moments,
                  Minimum, scatt_minimum, MIN_POSITIVE, MIN_UNDECIDED, MIN_NEGATIVE, MIN_NONFINITE,
                  MIN_UNSETTLED, MIN_MAX_EVALS,
                  Repair, scatt_repair, REPAIR_BEST, REPAIR_HEAT, REPAIR_UNIFORM, HOW_UNEXAMINED, HOW_UNTOUCHED,
                  HOW_HEAT, HOW_UNIFORM, HOW_UNREPAIRABLE, HOW_NONFINITE,
                  SCATT_LEGENDRE, SCATT_TABULAR, MAX_TAB_BINS, elastic_tab_batch, file6_tab_batch,
                  law9_tab_batch, sab_tab_batch, scatt_nuclide_tab, scatt_library_tab, scatt_library_at, grid_error,
                  thin_segments, thin_bounded, lib_compare,
                  scatt_sample, sample_brackets, SAMPLE_OK, SAMPLE_SKIPPED, SAMPLE_BADROW, SAMPLE_ZEROROW, SAMPLE_NEGDENSITY,
                  scatt_score, scatt_score_info, SCORE_OK, SCORE_SKIPPED, SCORE_BADROW, SCORE_ZEROROW,
                  nbody_leg_batch, nbody_rule, set_nbody, get_nbody,
                  nbody_tab_batch, set_nbody_tab, get_nbody_tab,
                  derive_tables, derive_groups, derive_bins, derive_moments, DERIVE_NONFINITE, DERIVE_NEGBIN,
                  DERIVE_ZERO, NDPP_EINVAL, NDPP_EDEVICE)
from .scatt import binary_search, elastic_brackets, calc_elastic_grid  # noqa: F401

__version__ = "0.2.0"
from .grid import merge, add_one_more_point, sab_egrid, chi_egrid  # noqa: F401,E402
