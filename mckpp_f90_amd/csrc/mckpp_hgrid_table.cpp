// mckpp_hgrid_table.cpp - the weight tables of a caller's horizontal grid (include/mckpp_hip_hgrid.h states the
// arithmetic and the device layout): the checks of a define, the remap of one level exactly as the header writes it -
// the yardstick every device result is compared with - and the sliced ELL the kernels read.  Host code without HIP, so
// that it is tested where no GPU is.  Compiled with -ffp-contract=off: every product and sum below is rounded once.
#include <cmath>
#include <cstdio>

#include "../../include/mckpp_hip_hgrid.h"

extern "C" int mckpp_host_hgrid_check(const char *name, int64_t nrows, int64_t nsrc, const mckpp_hgrid_table_c *t, char *msg,
                                      int64_t msglen)
{
  auto refuse = [&](const char *fmt, auto... a) {
    if (msg && msglen > 0) snprintf(msg, (size_t)msglen, fmt, a...);
    return -1;
  };
  if (!name) name = "?";
  if (!t || !t->ptr || nrows < 0 || nsrc < 0) return refuse("table %s: a null table or ptr, or a negative size", name);
  if (t->ptr[0] != 0) return refuse("table %s: row 0: ptr[0]=%lld, not 0", name, (long long)t->ptr[0]);
  for (int64_t r = 0; r < nrows; ++r) {
    if (t->ptr[r + 1] < t->ptr[r])
      return refuse("table %s: row %lld: ptr decreases (ptr[%lld]=%lld, ptr[%lld]=%lld)", name, (long long)r, (long long)r,
                    (long long)t->ptr[r], (long long)(r + 1), (long long)t->ptr[r + 1]);
    if (t->ptr[r + 1] - t->ptr[r] > INT32_MAX)
      return refuse("table %s: row %lld: %lld entries, more than a row's length holds", name, (long long)r,
                    (long long)(t->ptr[r + 1] - t->ptr[r]));
    if (t->ptr[r + 1] > t->ptr[r] && (!t->idx || !t->w)) return refuse("table %s: row %lld: idx or w is null", name, (long long)r);
    for (int64_t e = t->ptr[r]; e < t->ptr[r + 1]; ++e) {
      if (t->idx[e] < 0 || t->idx[e] >= nsrc)
        return refuse("table %s: row %lld: entry %lld: index %d is outside 0..%lld", name, (long long)r, (long long)e, (int)t->idx[e],
                      (long long)nsrc - 1);
      if (!std::isfinite(t->w[e]))
        return refuse("table %s: row %lld: entry %lld: the weight is not finite", name, (long long)r, (long long)e);
    }
  }
  return 0;
}

extern "C" int mckpp_host_hgrid_apply(int64_t nrows, const mckpp_hgrid_table_c *t, const double *x, const unsigned char *used,
                                      int norm, int fill, double land_value, double *out)
{
  if (!t || !t->ptr || !x || !out || nrows < 0 || norm > MCKPP_HGRID_NORM_USED) return -1;
  for (int64_t r = 0; r < nrows; ++r) {
    double a = 0.0, d = 0.0;
    bool any = false;
    for (int64_t e = t->ptr[r]; e < t->ptr[r + 1]; ++e) {
      const int32_t i = t->idx[e];
      if (used && !used[i]) continue;
      const double w = t->w[e];
      const double wx = w * x[i];
      if (!any) { a = wx; d = w; }           // the first used entry: an assignment
      else { a = a + wx; d = d + w; }
      any = true;
    }
    if (norm < 0) { out[r] = a; continue; }  // the in direction
    if (norm == MCKPP_HGRID_NORM_USED && d == 0.0) any = false;
    if (!any) { if (fill) out[r] = land_value; continue; }
    out[r] = norm == MCKPP_HGRID_NORM_USED ? a / d : a;
  }
  return 0;
}

extern "C" int64_t mckpp_host_hgrid_slices(int64_t nlist, const int64_t *rows, const mckpp_hgrid_table_c *t, const unsigned char *keep,
                                           int64_t *slice_off, int32_t *len, int32_t *idx_out, double *w_out)
{
  if (!t || !t->ptr || !slice_off || (nlist > 0 && !len) || nlist < 0 || (idx_out && !w_out)) return -1;
  const int64_t nslices = (nlist + 63) / 64;
  slice_off[0] = 0;
  for (int64_t s = 0; s < nslices; ++s) {
    int64_t width = 0;
    for (int64_t j = 64 * s; j < 64 * s + 64 && j < nlist; ++j) {
      const int64_t r = rows ? rows[j] : j;
      int32_t n = 0;
      for (int64_t e = t->ptr[r]; e < t->ptr[r + 1]; ++e)
        if (!keep || keep[t->idx[e]]) ++n;
      len[j] = n;
      if (n > width) width = n;
    }
    slice_off[s + 1] = slice_off[s] + 64 * width;
  }
  if (!idx_out) return slice_off[nslices];
  for (int64_t i = 0; i < slice_off[nslices]; ++i) { idx_out[i] = 0; w_out[i] = 0.0; }
  for (int64_t j = 0; j < nlist; ++j) {
    const int64_t r = rows ? rows[j] : j;
    int64_t at = slice_off[j / 64] + j % 64;
    for (int64_t e = t->ptr[r]; e < t->ptr[r + 1]; ++e) {
      if (keep && !keep[t->idx[e]]) continue;
      idx_out[at] = t->idx[e];
      w_out[at] = t->w[e];
      at += 64;
    }
  }
  return slice_off[nslices];
}
