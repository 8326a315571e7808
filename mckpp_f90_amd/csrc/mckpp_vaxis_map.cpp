// mckpp_vaxis_map.cpp - the table of the vertical interpolation between a caller's axis and the model's
// (include/mckpp_hip_vaxis.h states the interpolation).  Host code without HIP, so that it is tested where no GPU is.
//
// The branch tests and the bracket are the reference's src/mckpp_initialize_ocean_profiles_mod.F90:138-153.  Its DO
// WHILE carries kin from one target to the next; the targets descend, so what it finds is the smallest index whose
// lower level is not above the target - the rule the header states - and the search here is carried the same way.  t
// and dz depend on the two axes alone and are one rounded subtraction each, the same bits wherever they are formed.
#include <cmath>

#include "../../include/mckpp_hip_vaxis.h"
#include "../../include/mckpp_hip_vrecords.h"

namespace {
bool strictly_decreasing(int32_t n, const double *z)
{
  for (int32_t k = 0; k < n; ++k)
    if (!std::isfinite(z[k]) || (k > 0 && !(z[k] < z[k - 1]))) return false;
  return true;
}
}  // namespace

extern "C" int mckpp_host_vaxis_map(int32_t ns, const double *zs, int32_t nt, const double *zt, int32_t *branch, int32_t *kin,
                                    double *t, double *dz)
{
  if (!zs || !zt || !branch || !kin || !t || !dz || ns < 2 || nt < 1) return -1;
  if (!strictly_decreasing(ns, zs) || !strictly_decreasing(nt, zt)) return -1;
  int32_t k = 0;   // (the search may start where the last target's ended: the targets descend)
  for (int32_t j = 0; j < nt; ++j) {
    const double z = zt[j];
    if (z > zs[0]) {                 // :139
      branch[j] = MCKPP_VAXIS_ABOVE; kin[j] = 0; t[j] = 0.0; dz[j] = 1.0;
    } else if (z < zs[ns - 1]) {     // :142
      branch[j] = MCKPP_VAXIS_BELOW; kin[j] = ns - 1; t[j] = 0.0; dz[j] = 1.0;
    } else {                         // :146-152; zs[ns-1] <= z ends the search at ns - 2 at the latest
      while (zs[k + 1] > z) ++k;
      branch[j] = MCKPP_VAXIS_BRACKET;
      kin[j] = k;
      t[j] = z - zs[k];
      dz[j] = zs[k] - zs[k + 1];
    }
  }
  return 0;
}

// The level rule of include/mckpp_hip_vrecords.h: which model levels an out table reads, against the levels a schedule
// keeps.  A clamp reads kin, a bracket kin and kin + 1; the first caller level that reads outside lev0 .. lev0 + nlev - 1
// is reported with the first such level it reads.
extern "C" int mckpp_host_vrecords_rule(int32_t nt, const int32_t *branch, const int32_t *kin, int32_t lev0, int32_t nlev,
                                        int32_t *caller_level, int32_t *model_level)
{
  if (!branch || !kin || nt < 1 || nlev < 1) return -1;
  for (int32_t j = 0; j < nt; ++j) {
    const int32_t reads = branch[j] == MCKPP_VAXIS_BRACKET ? 2 : 1;
    for (int32_t m = 0; m < reads; ++m) {
      const int64_t lev = (int64_t)kin[j] + m;
      if (lev >= lev0 && lev < (int64_t)lev0 + nlev) continue;
      if (caller_level) *caller_level = j;
      if (model_level) *model_level = (int32_t)lev;
      return 1;
    }
  }
  return 0;
}
