// file4_device.h -- what the file-4 two-body kernels of file4_kernels.hip (moments) and
// tab_kernels.hip (bins) share: the kinematics of an incoming energy, a group's bounds in the CM
// cosine and the tabulated distribution at a bound (scattdata_header.F90:986-1034).  Both
// translation units are built with -DNDPP_FAST=0 -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include "ndpp_math.h"

namespace ndpp {
namespace {

// One group of one incoming energy (scattdata_header.F90:986-1015): the CM cosines of the
// group's bounds clamped to [-1, 1], the 1-based cells of the cosine grid they fall in, and
// whether the reference skips the group (both bounds clamped to the same end).
struct F4Bounds {
  double wlo, whi;
  int ilo, ihi;
  bool skip;
};
struct F4Kin {
  double R, onepawr2, onepR2, inv2REin;
};
__device__ inline F4Kin file4_kin(double Ein, double awr, double Q) {
  F4Kin k;
  k.R = awr * sqrt((1.0 + Q * (awr + 1.0) / (awr * Ein)));
  k.onepawr2 = (1.0 + awr) * (1.0 + awr);
  k.onepR2 = 1.0 + k.R * k.R;
  k.inv2REin = 0.5 / (k.R * Ein);
  return k;
}
__device__ inline F4Bounds file4_bounds(const F4Kin& k, double Ein, double dw, double eg, double eg1) {
  F4Bounds b;
  double wlo = (eg * k.onepawr2 - Ein * k.onepR2) * k.inv2REin;
  if (wlo < -1.0) wlo = -1.0; else if (wlo > 1.0) wlo = 1.0;
  b.ilo = (int)((wlo + 1.0) / dw) + 1;  // 1-based like the reference
  double whi = (eg1 * k.onepawr2 - Ein * k.onepR2) * k.inv2REin;
  if (whi < -1.0) whi = -1.0; else if (whi > 1.0) whi = 1.0;
  b.ihi = (int)((whi + 1.0) / dw) + 1;
  b.wlo = wlo;
  b.whi = whi;
  b.skip = (wlo == whi) && (wlo == -1.0 || wlo == 1.0);
  return b;
}
// the tabulated distribution at a bound (:1019-1034)
__device__ inline double file4_f_at(const MuGrid& grid, const double* fw, double w, int iw) {
  if (iw >= grid.M) return fw[grid.M - 1];
  const double interp = (w - grid.at(iw - 1)) / (grid.at(iw) - grid.at(iw - 1));
  return (1.0 - interp) * fw[iw - 1] + interp * fw[iw];
}

}  // namespace
}  // namespace ndpp
