// mckpp_kernels.hip - the small gfx950 kernels around the column step: layout conversion between the
// Fortran arrays (column index fastest) and the device rows (level fastest), surface-flux assembly
// (mckpp_fluxes), the bottom-temperature override, output-window reductions, and the batch probes the
// parity tests use.  The column step itself lives in mckpp_kernels_ps.hip.
//
// Arithmetic is written operation-for-operation in the reference's expression order and built with
// -ffp-contract=off, so results are bitwise reproducible against the CPU oracle (tests/).
#include "mckpp_colmath.h"

namespace {

using namespace mckpp_dev;

// ---------------------------------------------------------------------------
// small batch kernels used by the parity tests
// ---------------------------------------------------------------------------
__global__ void k_eos_batch(int64_t n, const double *s, const double *t, const double *p,
                            double *alpha, double *beta, double *sig0, double *cp)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a, b, s0;
  abk80_dev(s[i], t[i], p[i], a, b, s0);
  alpha[i] = a; beta[i] = b; sig0[i] = s0;
  cp[i] = cpsw_dev(s[i], t[i], p[i]);
}

// the exact-division helpers of mckpp_colmath.h, one quotient per thread:
// q[0] = div_fast, q[1] = div_fast_guarded, q[2] = div_by_refined, q[3] = the compiler's n / d
__global__ void k_div_batch(int64_t n, const double *num, const double *den, double *q)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = num[i], d = den[i], r = rcp_refine(d);
  q[i] = div_fast(a, d, r);
  q[n + i] = div_fast_guarded(a, d, r);
  q[2 * n + i] = div_by_refined(a, d, r);
  q[3 * n + i] = a / d;
}

__global__ void k_exp_batch(int64_t n, const double *x, double *y)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = mckpp_exp(x[i]);
}

// ---------------------------------------------------------------------------
// The move between device rows and caller planes, stated once for the nine kernels that make it (k_gather_rows,
// k_scatter_rows, k_record_pack, k_fetch_planes, k_record_planes, k_put_planes, k_vaxis_fetch_planes,
// k_vaxis_record_planes, k_vaxis_put_planes; k_fetch_planes and k_vaxis_put_planes have the routines below written out in their bodies, for
// the reasons given there).
//
// Rows are [nrow][ld] doubles with a row's levels contiguous; a plane is plane(npoints, nlev) with points fastest, and
// row r belongs at position map[r] of it.  A workgroup of 256 threads takes 64 rows (blockIdx.x) by 64 levels
// (blockIdx.y, origin l0) through `__shared__ double tile[64][65]`, which the kernel declares: tx = thread & 63 runs
// along whichever side is being read or written, ty = thread >> 6 strides the other side by 4, so both sides move
// whole 512-B segments, and the 65th column keeps the transposed access off one LDS bank.  A tile lane outside
// nrow x nlev holds 0.0 and is never written out, so what a kernel's arithmetic makes of that zero is of no account.
//
// The barrier rule: every thread of a workgroup that reaches the tile reaches its __syncthreads().  Exits before the
// barrier depend on blockIdx and on the plane alone (the level tile beyond the plane, the one-level path and its idle
// workgroups, the fill); exits that depend on the thread (a row or a level past the end) come after it.
//
// ONE_LEVEL: a plane of one level has nothing to transpose and takes a row per thread.  The grid's x extent is that of
// 64-row tiles, so every fourth workgroup takes 256 rows and the others leave.  The four plane kernels set it;
// k_gather_rows and k_scatter_rows send one level through the tile like any other.
// ---------------------------------------------------------------------------

// Rows to points.  load(r, lev, in_range) is the kernel's value of row r at level lev of the plane, formed in fp64, 0.0
// for a lane out of range; the one conversion to T is at the write.  map == nullptr: row r is position r.
template <bool ONE_LEVEL, class T, class Load>
__device__ __forceinline__ void tile_rows_to_points(double (*tile)[65], int64_t nrow, int nlev, int l0,
                                                    const int *__restrict__ map, int64_t npoints, T *__restrict__ dst,
                                                    Load load)
{
  if (l0 >= nlev) return;   // (the grid's level tiles are those of the deepest plane)
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  if (ONE_LEVEL && nlev == 1) {
    if (blockIdx.x & 3) return;
    const int64_t r = r0 + threadIdx.x;
    if (r < nrow) dst[map ? (int64_t)map[r] : r] = (T)load(r, 0, true);
    return;
  }
  for (int rr = ty; rr < 64; rr += 4) {       // read: levels fastest
    const int64_t r = r0 + rr;
    const int lev = l0 + tx;
    tile[tx][rr] = load(r, lev, r < nrow && lev < nlev);
  }
  __syncthreads();
  const int64_t r = r0 + tx;
  if (r >= nrow) return;
  const int64_t pos = map ? (int64_t)map[r] : r;
  for (int l = ty; l < 64; l += 4) {          // write: points fastest
    const int lev = l0 + l;
    if (lev < nlev) dst[(int64_t)lev * npoints + pos] = (T)tile[l][tx];
  }
}

// Points to rows: the opposite direction.  The plane's element, widened exactly, travels through the tile, and
// store(r, lev, v) is what the kernel does with it on the row side.  The map is read as it is: it must not be null.
template <bool ONE_LEVEL, class T, class Store>
__device__ __forceinline__ void tile_points_to_rows(double (*tile)[65], int64_t nrow, int nlev, int l0,
                                                    const int *__restrict__ map, int64_t npoints, const T *__restrict__ src,
                                                    Store store)
{
  if (l0 >= nlev) return;   // (the grid's level tiles are those of the deepest plane)
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  if (ONE_LEVEL && nlev == 1) {
    if (blockIdx.x & 3) return;
    const int64_t r = r0 + threadIdx.x;
    if (r < nrow) store(r, 0, (double)src[map[r]]);
    return;
  }
  {
    const int64_t r = r0 + tx;
    const int64_t pos = r < nrow ? (int64_t)map[r] : 0;
    for (int l = ty; l < 64; l += 4) {        // read: points fastest
      const int lev = l0 + l;
      double v = 0.0;
      if (r < nrow && lev < nlev) v = (double)src[(int64_t)lev * npoints + pos];
      tile[l][tx] = v;
    }
  }
  __syncthreads();
  const int lev = l0 + tx;
  if (lev >= nlev) return;
  for (int rr = ty; rr < 64; rr += 4) {       // write: levels fastest
    const int64_t r = r0 + rr;
    if (r < nrow) store(r, lev, tile[tx][rr]);
  }
}

// The fill of a position list: workgroup `ftile` of those behind a plane's row tiles takes 64 entries of the list of
// positions that are no row and writes v there, a thread per position, the levels of its level tile in turn.  No tile,
// no barrier.
template <class T>
__device__ __forceinline__ void fill_positions(int64_t ftile, int nlev, int l0, const int *__restrict__ list, int64_t n,
                                               int64_t npoints, T *__restrict__ dst, T v)
{
  if (l0 >= nlev) return;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t i = ftile * 64 + tx;
  if (i >= n) return;
  const int64_t pos = list[i];
  for (int l = ty; l < 64; l += 4)
    if (l0 + l < nlev) dst[(int64_t)(l0 + l) * npoints + pos] = v;
}

// Upload: the Fortran slab A(npts, nlev), as it is.
__global__ __launch_bounds__(256) void k_gather_rows(const double *__restrict__ src3d, int64_t npts,
                                                     int nlev, int lev_off, const int *__restrict__ ipt,
                                                     int64_t ncol, double *__restrict__ dst, int ld,
                                                     int dst_off)
{
  __shared__ double tile[64][65];
  tile_points_to_rows<false>(tile, ncol, nlev, blockIdx.y * 64, ipt, npts, src3d + (int64_t)lev_off * npts,
                             [&](int64_t c, int lev, double v) { dst[c * ld + dst_off + lev] = v; });
}

// Download, and window_fetch / window_record_fetch through a map of their own: the row's element, as it is.
__global__ __launch_bounds__(256) void k_scatter_rows(const double *__restrict__ src, int ld, int src_off,
                                                      const int *__restrict__ ipt, int64_t ncol,
                                                      double *__restrict__ dst3d, int64_t npts, int nlev,
                                                      int lev_off)
{
  __shared__ double tile[64][65];
  tile_rows_to_points<false>(tile, ncol, nlev, blockIdx.y * 64, ipt, npts, dst3d + (int64_t)lev_off * npts,
                             [&](int64_t c, int lev, bool in) { return in ? src[c * ld + src_off + lev] : 0.0; });
}

// ---------------------------------------------------------------------------
// Surface-flux assembly + non-turbulent flux: mckpp_fluxes,
// src/mckpp_fluxes_mod.F90:35-89, and its ntflux call (:93-118).  One thread
// per column; inputs are the eight forcing fields compacted to resident columns.
// ---------------------------------------------------------------------------
// The arithmetic, stated once as a function of the column's eight values: k_fluxes loads them from the compacted
// staging, k_fluxes_dev from the caller's device arrays through the column map.
__device__ __forceinline__ void fluxes_column(const mckpp_kparams &p, int c, int ntime, double taux, double tauy, double swf,
                                              double lwf, double lhf, double shf, double rain, double snow, int l_rest,
                                              double flsn, double el)
{
  double *cs = p.cs + (size_t)c * MCKPP_CS;
  const int *ci = p.ci + (size_t)c * MCKPP_CI;
  if ((taux == 0.0) && (tauy == 0.0)) taux = 1.e-10;            // :57-58
  double s1, s2, s3, s4, s5, s6;
  if (!l_rest) {                                                // :60-69
    s1 = taux; s2 = tauy; s3 = swf;
    s4 = lwf + lhf + shf - snow * flsn;
    s5 = 1e-10;
    s6 = rain + snow + (lhf / el);
  } else {                                                      // :70-77
    s1 = 1.e-10; s2 = 0.00; s3 = 300.00; s4 = -300.00; s5 = 0.00; s6 = 0.00;
  }
  cs[CS_SFLUX1] = s1; cs[CS_SFLUX2] = s2; cs[CS_SFLUX3] = s3;
  cs[CS_SFLUX4] = s4; cs[CS_SFLUX5] = s5; cs[CS_SFLUX6] = s6;
  if (p.diag && ntime >= 1) {                                   // ntflux, :110-116
    const size_t ro = (size_t)c * p.ld;
    const double rho0 = p.rho[ro], cp0 = p.cp[ro];
    const int jer = ci[CI_JERLOV];
    for (int k = 0; k <= p.nz; ++k) p.wXNT1[ro + k] = -s3 * p.swdk_tab[jer * p.ldc + k] / (rho0 * cp0);
  }
}

__global__ void k_fluxes(mckpp_kparams p, int ntime, const double *__restrict__ f8, int l_rest, double flsn,
                         double el)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= p.ncol) return;
  if (!p.ci[(size_t)c * MCKPP_CI + CI_LOCEAN]) return;          // fluxes_mod.F90:55
  const size_t n = (size_t)p.ncol;
  fluxes_column(p, c, ntime, f8[c], f8[n + c], f8[2 * n + c], f8[3 * n + c], f8[4 * n + c], f8[5 * n + c], f8[6 * n + c],
                f8[7 * n + c], l_rest, flsn, el);
}

// mckpp_hip_fluxes_dev: the eight fields are (npts) device arrays of the caller's, read through the column map
__global__ void k_fluxes_dev(mckpp_kparams p, int ntime, mckpp_dev_fields f, const int *__restrict__ ipt, int l_rest,
                             double flsn, double el)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= p.ncol) return;
  if (!p.ci[(size_t)c * MCKPP_CI + CI_LOCEAN]) return;          // fluxes_mod.F90:55
  const int64_t i = ipt[c];
  fluxes_column(p, c, ntime, f.f[0][i], f.f[1][i], f.f[2][i], f.f[3][i], f.f[4][i], f.f[5][i], f.f[6][i], f.f[7][i],
                l_rest, flsn, el);
}

// mckpp_hip_flux_ring_put_dev: the same arrays compacted into a slot of the flux ring, [8][ncol] like a record that
// mckpp_hip_flux_ring_put compacts on the host; a thread per column, the eight loads independent of one another
__global__ __launch_bounds__(256) void k_flux_gather(mckpp_dev_fields f, const int *__restrict__ ipt, int64_t ncol,
                                                     double *__restrict__ slot)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const int64_t i = ipt[c];
#pragma unroll
  for (int m = 0; m < 8; ++m) slot[(int64_t)m * ncol + c] = f.f[m][i];
}

// ---------------------------------------------------------------------------
// The caller's horizontal grids (include/mckpp_hip_hgrid.h): forcing in and fields out by remap weights.  The header
// states the arithmetic; hgrid_row_sums is that statement, once, for the three kernels below.  A thread takes row r of
// a sliced ELL table and a wave the slice r / 64 (the launches use workgroups of 256 with r = blockIdx.x * 256 +
// threadIdx.x, so a wave's rows are one slice's).  The trip count is the slice's width, the same for the whole wave;
// per trip the lanes read consecutive elements of idx and of w (256 B + 512 B a wave) and that one index and weight
// feed NF independent gathers, products and sums.  Padding is never loaded: a lane whose row has ended is predicated
// off.  The first entry assigns - a = w * x, d = w -, every further one adds; -ffp-contract=off keeps the product and
// the sum two rounded operations.  x(m, i): source value i of field m.  Returns the row's length (0 past the table).
// ---------------------------------------------------------------------------
template <int NF, bool DEN, class X>
__device__ __forceinline__ int hgrid_row_sums(const mckpp_hgrid_ell &t, int64_t r, X x, double (&a)[NF], double &d)
{
  const int lane = threadIdx.x & 63;
  const int64_t first = r - lane;             // the slice's first row
  int64_t base = 0;
  int width = 0;
  if (first < t.nrows) {                      // (a wave past the table has no slice: off[] ends with the last one's end)
    const int64_t s = first >> 6;
    base = t.off[s];
    width = (int)((t.off[s + 1] - base) >> 6);
  }
  width = __builtin_amdgcn_readfirstlane(width);
  const int len = r < t.nrows ? t.len[r] : 0;
#pragma unroll
  for (int m = 0; m < NF; ++m) a[m] = 0.0;
  d = 0.0;
  for (int k = 0; k < width; ++k) {
    if (k >= len) continue;
    const int64_t e = base + (int64_t)k * 64 + lane;
    const int i = t.idx[e];
    const double w = t.w[e];
    if (k == 0) {
#pragma unroll
      for (int m = 0; m < NF; ++m) a[m] = w * x(m, i);
      if (DEN) d = w;
    } else {
#pragma unroll
      for (int m = 0; m < NF; ++m) a[m] = a[m] + w * x(m, i);
      if (DEN) d = d + w;
    }
  }
  return len;
}

// mckpp_hip_hgrid_fluxes_dev: k_fluxes_dev with the column's eight values summed from the caller grid's arrays; the
// table's rows are the resident columns in column order
__global__ __launch_bounds__(256) void k_hgrid_fluxes(mckpp_kparams p, int ntime, mckpp_hgrid_ell t, mckpp_dev_fields f,
                                                      int l_rest, double flsn, double el)
{
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double a[8], d;
  hgrid_row_sums<8, false>(t, c, [&](int m, int i) { return f.f[m][i]; }, a, d);
  if (c >= p.ncol) return;
  if (!p.ci[(size_t)c * MCKPP_CI + CI_LOCEAN]) return;          // fluxes_mod.F90:55, as k_fluxes_dev
  fluxes_column(p, (int)c, ntime, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], l_rest, flsn, el);
}

// mckpp_hip_hgrid_flux_ring_put_dev: k_flux_gather likewise, into a slot [8][ncol] of the flux ring
__global__ __launch_bounds__(256) void k_hgrid_flux_gather(mckpp_hgrid_ell t, mckpp_dev_fields f, int64_t ncol,
                                                           double *__restrict__ slot)
{
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double a[8], d;
  hgrid_row_sums<8, false>(t, c, [&](int m, int i) { return f.f[m][i]; }, a, d);
  if (c >= ncol) return;
#pragma unroll
  for (int m = 0; m < 8; ++m) slot[(int64_t)m * ncol + c] = a[m];
}

// The second stage of mckpp_hip_hgrid_fetch_dev: a thread per caller point, the level on blockIdx.y, the plane on
// blockIdx.z.  The source is the staging plane k_fetch_planes wrote, points fastest, so the spatially local stencils
// of a remap gather within shared sectors.  The out table holds the entries of resident points only, so there is no
// mask: a point without a used entry has a row of length 0.
template <class T>
__device__ __forceinline__ void hgrid_out_plane(const mckpp_hgrid_plane &e)
{
  const int lev = blockIdx.y;
  if (lev >= e.nlev) return;   // (the grid's levels are those of the deepest plane)
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double *__restrict__ x = e.stage + (int64_t)lev * e.npts;
  double a[1], d;
  const int len = hgrid_row_sums<1, true>(e.t, j, [&](int, int i) { return x[i]; }, a, d);
  if (j >= e.t.nrows) return;
  T *dst = static_cast<T *>(e.out) + (int64_t)lev * e.t.nrows + j;
  const bool used = e.norm == 1;   // MCKPP_HGRID_NORM_USED
  if (len == 0 || (used && d == 0.0)) {
    if (e.fill) *dst = (T)e.land_value;
    return;
  }
  const double v = used ? a[0] / d : a[0];
  *dst = (T)v;
}

__global__ __launch_bounds__(256) void k_hgrid_out(const mckpp_hgrid_plane *__restrict__ tab)
{
  const mckpp_hgrid_plane e = tab[blockIdx.z];
  if (e.f32) hgrid_out_plane<float>(e);
  else hgrid_out_plane<double>(e);
}

// ---------------------------------------------------------------------------
// mckpp_physics_overrides_bottomtemp, src/mckpp_physics_overrides.F90:12-24:
// prescribed temperature of the bottom grid point; one thread per column.
// ---------------------------------------------------------------------------
__global__ void k_bottomtemp(mckpp_kparams p, const double *__restrict__ bt)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= p.ncol) return;
  const size_t ro = (size_t)c * p.ld;
  const double b = bt[c];
  const double tinc = b - p.T[ro + p.nzp1 - 1];                                   // :16
  p.tinc_fcorr[ro + p.nzp1] = tinc;
  p.ocnTcorr[ro + p.nzp1] = tinc * p.rho[ro + p.nzp1] * p.cp[ro + p.nzp1] / p.dto;   // :17-19
  p.T[ro + p.nzp1 - 1] = b;                                                       // :20
}

// ---------------------------------------------------------------------------
// Output-window reductions: what XIOS does with the fields mckpp_xios_output_control
// sends (src/mckpp_xios_io.F90:74-210; operations instant / average / minimum / maximum of
// run/iodef.xml:88-157), on the device so that only reduced fields cross PCIe / xGMI.
// One output field = nlev values per column taken from a device row array (element src_off + l of
// the column's row, row length src_ld) or from the column record (src_ld = MCKPP_CS, nlev = 1),
// optionally plus the column's Sref (the reference sends S = X(:,:,2) + Sref).  One thread per
// (column, level): either one sample into `inst`, or the running sum / min / max.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_out_sample(const double *__restrict__ src, int src_ld, int src_off,
                                                   const double *__restrict__ cs, int add_sref, int64_t ncol, int nlev,
                                                   int ld_out, double *__restrict__ sum, double *__restrict__ mn,
                                                   double *__restrict__ mx, int first, double *__restrict__ inst)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)ncol * ld_out) return;
  const int64_t c = (int64_t)(i / ld_out);
  const int l = (int)(i - (size_t)c * ld_out);
  double v = 0.0;
  if (l < nlev) {
    v = src[(size_t)c * src_ld + src_off + l];
    if (add_sref) v = v + cs[(size_t)c * MCKPP_CS + CS_SREF];
  }
  if (inst) { inst[i] = v; return; }
  double s_ = sum[i], a = mn[i], b = mx[i];
  if (first) { s_ = 0.0; a = v; b = v; }
  sum[i] = s_ + v;
  mn[i] = v < a ? v : a;
  mx[i] = v > b ? v : b;
}

__global__ void k_window_mean(const double *__restrict__ sum, double *__restrict__ out, size_t n, double count)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = sum[i] / count;
}

// ---------------------------------------------------------------------------
// The plane kernels: one launch moves every plane of a call, the planes on blockIdx.z and described by a device
// table; the grid's level tiles are those of the deepest plane.  The move is the one stated above (rows to points, or
// points to rows for the put); what follows says what each kernel's value is.
// ---------------------------------------------------------------------------

// Export of an output schedule's records (mckpp_hip_window_export): every plane of one record into its export slot,
// in the layout the host wants - no ld padding, through the column map (null: the columns themselves, a shard's
// compact form) - so that the fetch is a plain copy.  The value: the ring row's element, of a mean divided by the
// period (k_window_mean's one division), then narrowed where T is float.  Only resident columns are written: the
// slot's land points were filled when the export was set.
template <class T>
__global__ __launch_bounds__(256) void k_record_pack(const mckpp_pack_plane *__restrict__ tab, int ring_slot, double period,
                                                     const int *__restrict__ ipt, int64_t ncol, int64_t npts,
                                                     char *__restrict__ dst_slot)
{
  __shared__ double tile[64][65];
  const mckpp_pack_plane e = tab[blockIdx.z];
  const bool mean = e.op == 0;
  const double *__restrict__ src = e.src + (long long)ring_slot * e.slot_stride;
  tile_rows_to_points<true>(tile, ncol, e.nlev, blockIdx.y * 64, ipt, npts, reinterpret_cast<T *>(dst_slot + e.dst_off),
                            [&](int64_t c, int lev, bool in) {
                              double v = in ? src[c * e.ld + e.off + lev] : 0.0;
                              if (mean) v = v / period;
                              return v;
                            });
}

template <class T>
__global__ void k_export_fill(T *__restrict__ p, size_t n, T v)
{
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// Delivery of output fields into the caller's device arrays (mckpp_hip_fetch_dev): levels off .. off + nlev - 1 of a
// field as it stands on the device, as out(npts, nlev) through the column map; the element type is a plane's own.
// The value: k_out_sample's - the row's element, plus the column's Sref where the field is S - then narrowed where T is
// float.  The first `coltiles` workgroups in x take the resident columns; those after them fill the list of
// non-resident points with the plane's land value, where it asks for that.
//
// This kernel keeps a body of its own: it is tile_rows_to_points<true> and fill_positions written out, with the
// value formed in place.  Through the shared routines the compiler's code for it measured 4 % slower
// (profiles/tiles/README.md), so the text below is what is held to the barrier rule above by hand.
template <class T>
__device__ __forceinline__ void fetch_plane(const mckpp_fetch_plane &e, double (*tile)[65], const int *__restrict__ ipt,
                                            int64_t ncol, int64_t npts, const double *__restrict__ cs,
                                            const int *__restrict__ land, int64_t nland, int coltiles)
{
  const int l0 = blockIdx.y * 64;
  if (l0 >= e.nlev) return;   // (the grid's level tiles are those of the deepest plane)
  T *__restrict__ dst = static_cast<T *>(e.out);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  if ((int)blockIdx.x >= coltiles) {
    if (!e.fill_land) return;
    const int64_t i = (int64_t)((int)blockIdx.x - coltiles) * 64 + tx;
    if (i >= nland) return;
    const int64_t pt = land[i];
    const T v = (T)e.land_value;
    for (int l = ty; l < 64; l += 4)
      if (l0 + l < e.nlev) dst[(int64_t)(l0 + l) * npts + pt] = v;
    return;
  }
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  if (e.nlev == 1) {   // the one-level path
    if (blockIdx.x & 3) return;
    const int64_t c = c0 + threadIdx.x;
    if (c < ncol) {
      double v = e.src[c * e.ld + e.off];
      if (e.add_sref) v = v + cs[c * MCKPP_CS + CS_SREF];
      dst[ipt[c]] = (T)v;
    }
    return;
  }
  for (int cc = ty; cc < 64; cc += 4) {       // read: levels fastest
    const int64_t c = c0 + cc;
    const int lev = l0 + tx;
    double v = 0.0;
    if (c < ncol && lev < e.nlev) {
      v = e.src[c * e.ld + e.off + lev];
      if (e.add_sref) v = v + cs[c * MCKPP_CS + CS_SREF];
    }
    tile[tx][cc] = v;
  }
  __syncthreads();
  const int64_t c = c0 + tx;
  if (c >= ncol) return;
  const int64_t pt = ipt[c];
  for (int l = ty; l < 64; l += 4) {          // write: points fastest
    const int lev = l0 + l;
    if (lev < e.nlev) dst[(int64_t)lev * npts + pt] = (T)tile[l][tx];
  }
}

__global__ __launch_bounds__(256) void k_fetch_planes(const mckpp_fetch_plane *__restrict__ tab, const int *__restrict__ ipt,
                                                      int64_t ncol, int64_t npts, const double *__restrict__ cs,
                                                      const int *__restrict__ land, int64_t nland, int coltiles)
{
  __shared__ double tile[64][65];
  const mckpp_fetch_plane e = tab[blockIdx.z];
  if (e.f32) fetch_plane<float>(e, tile, ipt, ncol, npts, cs, land, nland, coltiles);
  else fetch_plane<double>(e, tile, ipt, ncol, npts, cs, land, nland, coltiles);
}

// Delivery of completed records of output schedules into the caller's device arrays (mckpp_hip_records_dev).  The
// planes may come from any schedules and records, so a plane carries its own geometry in the table: its rows (ring
// slot and operation resolved by the host), their number, the map row -> position of its point axis, the axis' length,
// and the list of positions that are no row.  The value: k_record_pack's - the row's element, of a mean divided by the
// period, then narrowed where T is float.  The grid's x extent is the largest plane's; a plane's first ceil(nrow / 64)
// workgroups in x take its rows, those after them fill its non-row list where it asks for that, and a workgroup beyond
// both leaves before it touches memory.
template <class T>
__device__ __forceinline__ void record_plane(const mckpp_rec_plane &e, double (*tile)[65])
{
  const int l0 = blockIdx.y * 64;
  T *__restrict__ dst = static_cast<T *>(e.out);
  const int64_t rowtiles = (e.nrow + 63) / 64;
  if ((int64_t)blockIdx.x >= rowtiles) {
    if (e.fill) fill_positions((int64_t)blockIdx.x - rowtiles, e.nlev, l0, e.norow, e.nnorow, e.npoints, dst, (T)e.land_value);
    return;
  }
  tile_rows_to_points<true>(tile, e.nrow, e.nlev, l0, e.map, e.npoints, dst, [&](int64_t r, int lev, bool in) {
    double v = in ? e.src[r * e.ld + e.off + lev] : 0.0;
    if (e.mean) v = v / e.period;
    return v;
  });
}

__global__ __launch_bounds__(256) void k_record_planes(const mckpp_rec_plane *__restrict__ tab)
{
  __shared__ double tile[64][65];
  const mckpp_rec_plane e = tab[blockIdx.z];
  if (e.f32) record_plane<float>(e, tile);
  else record_plane<double>(e, tile);
}

// The prognostic state set or incremented from the caller's arrays (mckpp_hip_put_dev, mckpp_hip_put_host): every plane
// - in(npts, nlev), doubles or floats widened exactly, through the column map - applied to elements off .. off + nlev - 1
// of a profile's rows and, where the plane asks for it, of the field's two saved time levels.  Element type, operation
// and flags are a plane's own.  The value travels through the tile as it is, and put_element is what happens to it on
// the row side, the skip decision included: no sentinel, no second tile.  No atomics: the host refused overlapping
// planes and a column is in the map once, so every state element has one writer.  Each operation below is one fp64
// operation, in the order include/mckpp_hip_put.h states (built with -ffp-contract=off).
__device__ __forceinline__ void put_element(const mckpp_put_plane &e, double *__restrict__ cs, int64_t c, int lev, double v)
{
  if (e.skip && v == e.skip_value) return;
  const int64_t i = c * e.ld + e.off + lev;
  double x;
  if (e.add) x = e.row[i] + v;
  else x = e.sub_sref ? v - cs[c * MCKPP_CS + CS_SREF] : v;
  e.row[i] = x;
  if (e.lv0) {
    if (e.add) { e.lv0[i] = e.lv0[i] + v; e.lv1[i] = e.lv1[i] + v; }
    else { e.lv0[i] = x; e.lv1[i] = x; }
  }
  // ocnstep_mod.F90:307-314 for this field: the column's level-1 value is now x
  if (e.ref_slot >= 0 && lev == 0) cs[c * MCKPP_CS + e.ref_slot] = e.ref_sref ? x + cs[c * MCKPP_CS + CS_SREF] : x;
}

__global__ __launch_bounds__(256) void k_put_planes(const mckpp_put_plane *__restrict__ tab, const int *__restrict__ ipt,
                                                    int64_t ncol, int64_t npts, double *__restrict__ cs)
{
  __shared__ double tile[64][65];
  const mckpp_put_plane e = tab[blockIdx.z];
  const int l0 = blockIdx.y * 64;
  const auto put = [&](int64_t c, int lev, double v) { put_element(e, cs, c, lev, v); };
  if (e.f32) tile_points_to_rows<true>(tile, ncol, e.nlev, l0, ipt, npts, static_cast<const float *>(e.in), put);
  else tile_points_to_rows<true>(tile, ncol, e.nlev, l0, ipt, npts, static_cast<const double *>(e.in), put);
}

// State in from planes on a caller's horizontal grid (mckpp_hip_remap_put_dev, include/mckpp_hip_remap.h).  The relayout
// tile of k_put_planes with the value formed on the point side, where tx is a resident column: the in table's rows are
// the columns in column order, so the workgroup's 64 columns are one ELL slice, which its four waves share.  Wave ty
// holds 16 of the tile's levels as the 16 running sums of hgrid_row_sums: an entry's index and weight are loaded once and
// feed 16 gathers, one per level, each along the caller's points.  The sums cross the tile and a byte beside each says
// that its element stays as it is - a value read was the skip value, or the row is empty; put_element is what happens
// to the others on the row side.  A plane of one level takes a column per thread, 256 per workgroup, without the tile
// (ONE_LEVEL above).  The barrier rule is kept by hand: the exits before the barrier depend on blockIdx and the plane.
template <class T>
__device__ __forceinline__ void remap_put_plane(const mckpp_remap_put_plane &e, double (*tile)[65], unsigned char (*hold)[68],
                                                int64_t ncol, double *__restrict__ cs)
{
  const int l0 = blockIdx.y * 64, nlev = e.put.nlev;
  if (l0 >= nlev) return;   // (the grid's level tiles are those of the deepest plane)
  const T *__restrict__ src = static_cast<const T *>(e.put.in);
  const double skip_value = e.put.skip_value;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  if (nlev == 1) {   // the one-level path
    if (blockIdx.x & 3) return;
    const int64_t r = r0 + threadIdx.x;
    double a[1], d;
    bool hit = false;
    const int len = hgrid_row_sums<1, false>(e.t, r, [&](int, int i) {
      const double v = (double)src[i];
      hit = hit || v == skip_value;
      return v;
    }, a, d);
    if (r < ncol && len > 0 && !(e.skip && hit)) put_element(e.put, cs, r, 0, a[0]);
    return;
  }
  {
    const int lw = l0 + ty * 16;              // read: points fastest, 16 levels per wave
    double a[16], d;
    unsigned hit = 0u;
    const int len = hgrid_row_sums<16, false>(e.t, r0 + tx, [&](int m, int i) {
      if (lw + m >= nlev) return 0.0;         // (the wave's: a level past the plane is not read)
      const double v = (double)src[(int64_t)(lw + m) * e.n + i];
      if (v == skip_value) hit |= 1u << m;
      return v;
    }, a, d);
    if (!e.skip) hit = 0u;
    if (len == 0) hit = 0xffffu;              // an empty row, or a lane past the last column
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      tile[ty * 16 + m][tx] = a[m];
      hold[ty * 16 + m][tx] = (hit >> m) & 1u;
    }
  }
  __syncthreads();
  const int lev = l0 + tx;
  if (lev >= nlev) return;
  for (int rr = ty; rr < 64; rr += 4) {       // write: levels fastest
    const int64_t r = r0 + rr;
    if (r >= ncol || hold[tx][rr]) continue;
    put_element(e.put, cs, r, lev, tile[tx][rr]);
  }
}

__global__ __launch_bounds__(256) void k_remap_put_planes(const mckpp_remap_put_plane *__restrict__ tab, int64_t ncol,
                                                          double *__restrict__ cs)
{
  __shared__ double tile[64][65];
  __shared__ unsigned char hold[64][68];
  const mckpp_remap_put_plane e = tab[blockIdx.z];
  if (e.put.f32) remap_put_plane<float>(e, tile, hold, ncol, cs);
  else remap_put_plane<double>(e, tile, hold, ncol, cs);
}

// ---------------------------------------------------------------------------
// The caller's vertical axes (include/mckpp_hip_vaxis.h): planes on levels that are not the model's.  The interpolation
// is stated there; vaxis_value is its per-element part - one subtraction, one product, one quotient, one sum, each a
// rounded fp64 operation (-ffp-contract=off, the compiler's IEEE divide) - on the one or two source values an entry of
// the axis table names.  The table is indexed by the target level, which a wave shares on the side where it is read.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double vaxis_value(const mckpp_vaxis_ent &a, double va, double vb)
{
  if (a.branch != 2) return va;
  const double dv = va - vb;
  const double p = dv * a.t;
  const double q = p / a.dz;
  return va + q;
}

// State in on a caller's axis (mckpp_hip_vaxis_put_dev / _put_host, and the four profiles of
// mckpp_hip_vaxis_init_profiles).  The relayout tile of k_put_planes, with the value formed on the point side: there
// tx is a column and a wave shares the model level, so the loads of the bracket's two input levels are whole segments
// along the points and the table entry is the wave's.  The value travels through the tile and a byte beside it says
// whether a value the branch read was the skip value; put_element is what happens to it on the row side.  A body of
// its own for that byte; the barrier rule above is kept by hand: the one exit before the barrier depends on blockIdx
// and the plane alone.
template <class T>
__device__ __forceinline__ void vaxis_put_plane(const mckpp_vaxis_put_plane &e, double (*tile)[65], unsigned char (*hold)[68],
                                                const int *__restrict__ ipt, int64_t ncol, int64_t npts,
                                                double *__restrict__ cs)
{
  const int l0 = blockIdx.y * 64, nlev = e.put.nlev;
  if (l0 >= nlev) return;
  const T *__restrict__ src = static_cast<const T *>(e.put.in);
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  {
    const int64_t r = r0 + tx;
    const int64_t pos = r < ncol ? (int64_t)ipt[r] : 0;
    for (int l = ty; l < 64; l += 4) {        // read: points fastest, a model level per wave
      const int lev = l0 + l;
      double v = 0.0;
      bool skipped = false;
      if (r < ncol && lev < nlev) {
        const mckpp_vaxis_ent a = e.tab[lev];
        const double va = (double)src[(int64_t)a.kin * npts + pos];
        double vb = va;
        if (a.branch == 2) vb = (double)src[(int64_t)(a.kin + 1) * npts + pos];
        skipped = e.skip && (va == e.put.skip_value || vb == e.put.skip_value);
        v = vaxis_value(a, va, vb);
      }
      tile[l][tx] = v;
      hold[l][tx] = skipped;
    }
  }
  __syncthreads();
  const int lev = l0 + tx;
  if (lev >= nlev) return;
  bool kelvin = false;
  for (int rr = ty; rr < 64; rr += 4) {       // write: levels fastest
    const int64_t r = r0 + rr;
    if (r >= ncol || hold[tx][rr]) continue;
    const double v = tile[tx][rr];
    put_element(e.put, cs, r, lev, v);
    if (e.row2) e.row2[r * e.put.ld + e.put.off + lev] = v;
    if (e.kelvin) kelvin = kelvin || (v > 200.0 && v < 400.0);   // initialize_ocean_profiles_mod.F90:83-84, the temperature plane of the profiles alone
  }
  if (kelvin) atomicOr(e.kelvin, 1u);
}

__global__ __launch_bounds__(256) void k_vaxis_put_planes(const mckpp_vaxis_put_plane *__restrict__ tab,
                                                          const int *__restrict__ ipt, int64_t ncol, int64_t npts,
                                                          double *__restrict__ cs)
{
  __shared__ double tile[64][65];
  __shared__ unsigned char hold[64][68];
  const mckpp_vaxis_put_plane e = tab[blockIdx.z];
  if (e.put.f32) vaxis_put_plane<float>(e, tile, hold, ipt, ncol, npts, cs);
  else vaxis_put_plane<double>(e, tile, hold, ipt, ncol, npts, cs);
}

// The end of mckpp_hip_vaxis_init_profiles (initialize_ocean_profiles_mod.F90:83-85, :104-117), behind the launch that
// wrote T and the whole S and raised *kelvin: a wave per column, four columns per workgroup.  Every lane reads S(1) and
// S(nzp1) before the barrier and the column's S is rewritten after it; the barrier is reached by every thread.
__global__ __launch_bounds__(256) void k_vaxis_init_finish(double *__restrict__ T, double *__restrict__ S, int ld, int nzp1,
                                                           int64_t ncol, double *__restrict__ cs,
                                                           const unsigned *__restrict__ kelvin, double tk0, int l_ssref)
{
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool mine = c < ncol;
  const int64_t ro = mine ? c * ld : 0;
  double s1 = 0.0, sn = 0.0;
  if (mine) { s1 = S[ro]; sn = S[ro + nzp1 - 1]; }
  __syncthreads();
  if (!mine) return;
  const bool in_kelvin = *kelvin != 0u;
  const double sref = (s1 + sn) / 2.;                            // :104-105
  double t1 = 0.0, x1 = 0.0;
  for (int lev = lane; lev < nzp1; lev += 64) {
    double t = T[ro + lev];
    if (in_kelvin) { t = t - tk0; T[ro + lev] = t; }             // :85
    const double x = S[ro + lev] - sref;                         // :108
    S[ro + lev] = x;
    if (lev == 0) { t1 = t; x1 = x; }
  }
  if (lane != 0) return;
  double *q = cs + c * MCKPP_CS;
  q[CS_SREF] = sref;
  q[CS_SSREF] = sref;                                            // :106
  q[CS_TREF] = t1;                                               // :112
  q[CS_SSURF] = l_ssref ? sref : x1 + sref;                      // :113-117
}

// Fields out on a caller's axis (mckpp_hip_vaxis_fetch_dev): k_fetch_planes with the value formed on the row side,
// where tx is a caller level: the row's two bracket levels - S with the column's Sref added to each first - through the
// out table.  kin rises with the caller level, so a wave's loads stay within the row's segments.  The land fill is
// k_record_planes': the workgroups behind the column tiles.
template <class T>
__device__ __forceinline__ void vaxis_fetch_plane(const mckpp_vaxis_fetch_plane &e, double (*tile)[65],
                                                  const int *__restrict__ ipt, int64_t ncol, int64_t npts,
                                                  const double *__restrict__ cs, const int *__restrict__ land,
                                                  int64_t nland, int coltiles)
{
  const mckpp_fetch_plane &f = e.f;
  const int l0 = blockIdx.y * 64;
  T *__restrict__ dst = static_cast<T *>(f.out);
  if ((int)blockIdx.x >= coltiles) {
    if (f.fill_land) fill_positions((int64_t)((int)blockIdx.x - coltiles), f.nlev, l0, land, nland, npts, dst, (T)f.land_value);
    return;
  }
  tile_rows_to_points<false>(tile, ncol, f.nlev, l0, ipt, npts, dst, [&](int64_t c, int lev, bool in) {
    if (!in) return 0.0;
    const mckpp_vaxis_ent a = e.tab[lev];
    const double *row = f.src + c * f.ld + f.off;
    double va = row[a.kin];
    double vb = a.branch == 2 ? row[a.kin + 1] : va;
    if (f.add_sref) {
      const double sref = cs[c * MCKPP_CS + CS_SREF];
      va = va + sref;
      vb = vb + sref;
    }
    return vaxis_value(a, va, vb);
  });
}

__global__ __launch_bounds__(256) void k_vaxis_fetch_planes(const mckpp_vaxis_fetch_plane *__restrict__ tab,
                                                            const int *__restrict__ ipt, int64_t ncol, int64_t npts,
                                                            const double *__restrict__ cs, const int *__restrict__ land,
                                                            int64_t nland, int coltiles)
{
  __shared__ double tile[64][65];
  const mckpp_vaxis_fetch_plane e = tab[blockIdx.z];
  if (e.f.f32) vaxis_fetch_plane<float>(e, tile, ipt, ncol, npts, cs, land, nland, coltiles);
  else vaxis_fetch_plane<double>(e, tile, ipt, ncol, npts, cs, land, nland, coltiles);
}

// Completed records on a caller's axis (mckpp_hip_vrecords_vaxis_dev / _host, the first stage of mckpp_hip_vrecords_hv_dev;
// include/mckpp_hip_vrecords.h): k_record_planes with the value formed on the row side, as vaxis_fetch_plane forms it.
// There tx is a caller level: the row's one or two source elements - kin rebased by the schedule's first kept level, each
// of a mean divided by the period first, k_record_planes' division - go through the axis's out table.  kin rises with the
// caller level, so a wave's loads stay within the row's segments.  An axis has at least two levels: no one-level path.
// The geometry is a plane's own, and the fill of the positions that are no row is k_record_planes': the workgroups
// behind the row tiles.
template <class T>
__device__ __forceinline__ void vaxis_record_plane(const mckpp_vrec_plane &e, double (*tile)[65])
{
  const mckpp_rec_plane &r = e.r;
  const int l0 = blockIdx.y * 64;
  T *__restrict__ dst = static_cast<T *>(r.out);
  const int64_t rowtiles = (r.nrow + 63) / 64;
  if ((int64_t)blockIdx.x >= rowtiles) {
    if (r.fill) fill_positions((int64_t)blockIdx.x - rowtiles, r.nlev, l0, r.norow, r.nnorow, r.npoints, dst, (T)r.land_value);
    return;
  }
  tile_rows_to_points<false>(tile, r.nrow, r.nlev, l0, r.map, r.npoints, dst, [&](int64_t row, int lev, bool in) {
    if (!in) return 0.0;
    const mckpp_vaxis_ent a = e.tab[lev];
    const double *src = r.src + row * r.ld + r.off + (a.kin - e.lev0);
    double va = src[0];
    double vb = a.branch == 2 ? src[1] : va;
    if (r.mean) {
      va = va / r.period;
      vb = vb / r.period;
    }
    return vaxis_value(a, va, vb);
  });
}

__global__ __launch_bounds__(256) void k_vaxis_record_planes(const mckpp_vrec_plane *__restrict__ tab)
{
  __shared__ double tile[64][65];
  const mckpp_vrec_plane e = tab[blockIdx.z];
  if (e.r.f32) vaxis_record_plane<float>(e, tile);
  else vaxis_record_plane<double>(e, tile);
}

// State in from planes on a caller's grid and a caller's axis at once (mckpp_hip_hv_put_dev, include/mckpp_hip_hv.h):
// horizontal first, at the caller's levels, then vertical.  remap_put_plane's shape - the workgroup's 64 columns are one
// ELL slice, which its four waves share, and a tile of 64 model levels - with the 16 running sums of hgrid_row_sums
// holding 8 model levels a pass: sums 2 j and 2 j + 1 are those of the caller levels kin and kin + 1 that the axis's in
// table names for the pass's level j.  The entry is the wave's (the wave id goes through readfirstlane, so the eight
// entries of a pass are scalar loads).  A clamp reads kin for both: every gather is issued unconditionally, the second
// sum of a clamp is formed from the same values and vaxis_value does not look at it, and its skip bit says what the
// first one says.  A level past the axis reads caller level 0 and is never written.  Two passes cover the wave's 16
// levels, so an entry's index and weight are loaded twice a workgroup.  vaxis_value forms the element on the point side;
// it and its hold byte - a value read at a level the branch reads was the skip value, or the row is empty - cross the
// tiles, and put_element is what happens to the others on the row side.  The barrier rule is kept by hand: the one exit
// before the barrier depends on blockIdx and the plane alone.
template <class T>
__device__ __forceinline__ void hv_put_plane(const mckpp_hv_put_plane &e, double (*tile)[65], unsigned char (*hold)[68],
                                             int64_t ncol, double *__restrict__ cs)
{
  const int l0 = blockIdx.y * 64, nlev = e.put.nlev;
  if (l0 >= nlev) return;   // (the grid's level tiles are those of the model's axis)
  const T *__restrict__ src = static_cast<const T *>(e.put.in);
  const double skip_value = e.put.skip_value;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(ty);
  for (int pass = 0; pass < 2; ++pass) {      // read: points fastest, 8 model levels per wave and pass
    const int t0 = wave * 16 + pass * 8;      // the pass's first level of the tile
    mckpp_vaxis_ent ent[8];
    int64_t at[16];                           // where the caller levels of sums 2 j, 2 j + 1 begin in the plane
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int lev = l0 + t0 + j;
      ent[j] = lev < nlev ? e.tab[lev] : mckpp_vaxis_ent{0, 0, 0.0, 1.0};
      at[2 * j] = (int64_t)ent[j].kin * e.n;
      at[2 * j + 1] = (int64_t)(ent[j].branch == 2 ? ent[j].kin + 1 : ent[j].kin) * e.n;
    }
    double a[16], d;
    unsigned hit = 0u;
    const int len = hgrid_row_sums<16, false>(e.t, r0 + tx, [&](int m, int i) {
      const double v = (double)src[at[m] + i];
      if (v == skip_value) hit |= 1u << m;
      return v;
    }, a, d);
    if (!e.skip) hit = 0u;
    if (len == 0) hit = 0xffffu;              // an empty row, or a lane past the last column
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      tile[t0 + j][tx] = vaxis_value(ent[j], a[2 * j], a[2 * j + 1]);
      hold[t0 + j][tx] = (hit >> (2 * j)) & 3u ? 1 : 0;
    }
  }
  __syncthreads();
  const int lev = l0 + tx;
  if (lev >= nlev) return;
  for (int rr = ty; rr < 64; rr += 4) {       // write: levels fastest
    const int64_t r = r0 + rr;
    if (r >= ncol || hold[tx][rr]) continue;
    put_element(e.put, cs, r, lev, tile[tx][rr]);
  }
}

__global__ __launch_bounds__(256) void k_hv_put_planes(const mckpp_hv_put_plane *__restrict__ tab, int64_t ncol,
                                                       double *__restrict__ cs)
{
  __shared__ double tile[64][65];
  __shared__ unsigned char hold[64][68];
  const mckpp_hv_put_plane e = tab[blockIdx.z];
  if (e.put.f32) hv_put_plane<float>(e, tile, hold, ncol, cs);
  else hv_put_plane<double>(e, tile, hold, ncol, cs);
}

// ---------------------------------------------------------------------------
// Records reduced over levels and points (mckpp_hip_records_reduce_dev / _host).  include/mckpp_hip_reduce.h states the
// arithmetic and its order; the four kernels below are that statement, each one launch for all planes of a call
// (blockIdx.z, the table of mckpp_red_plane).  No atomics: every element of `terms` and of `out` has one writer per
// kernel, and the order of a sum does not depend on the grid.
//
//   k_reduce_fill    what no row writes: a slab's non-row terms and padding (+0.0; +-infinity for min / max), the
//                    land value of an axis-only plane's non-row positions
//   k_reduce_terms   64 rows per workgroup, their levels through the relayout tile 64 at a time, so the ring rows are
//                    read as whole 512-B segments whatever the plane reduces (a plane of one level: a row per thread): an axis reduction continues down the
//                    level tiles on the row's own thread in ascending order; a domain-only plane writes its level
//                    slabs points fastest.  Result to `out` (axis only) or, times the point weight, to the slab
//   k_reduce_halve   a slab of n2 > m terms halved in place down to m: thread j owns the elements j, j + m, ... - the
//                    steps t[i] = t[i] + t[i + n], n >= m, never leave a residue, so no thread reads another's
//   k_reduce_finish  the last m (or n2) terms of a level's slab - and of the denominator's - through LDS: the same
//                    halving steps with a barrier between, then the division and the one store
// ---------------------------------------------------------------------------
__device__ __forceinline__ double red_combine(int op, double a, double b)   // t[i] and t[i + n]
{
  if (op == RED_MIN) return b < a ? b : a;
  if (op == RED_MAX) return b > a ? b : a;
  return a + b;
}

__global__ __launch_bounds__(256) void k_reduce_fill(const mckpp_red_plane *__restrict__ tab)
{
  const mckpp_red_plane e = tab[blockIdx.z];
  if (!e.fill) return;
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (e.domain_op == RED_NONE) {
    for (int64_t i = i0; i < e.nnorow; i += step) e.out[e.norow[i]] = e.land_value;
    return;
  }
  const int64_t all = (int64_t)e.nslab * e.n2, valued = e.domain_op == RED_AVERAGE ? all - e.n2 : all;
  const double id = e.domain_op == RED_MIN ? __builtin_inf() : e.domain_op == RED_MAX ? -__builtin_inf() : 0.0;
  for (int64_t i = i0; i < all; i += step) e.terms[i] = i < valued ? id : 0.0;
}

__global__ __launch_bounds__(256) void k_reduce_terms(const mckpp_red_plane *__restrict__ tab)
{
  __shared__ double tile[64][65];
  const mckpp_red_plane e = tab[blockIdx.z];
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  if (r0 >= e.nrow) return;   // (the grid's row tiles are those of the plane with most rows)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r = r0 + tx;
  const bool mine = r < e.nrow;   // on the point side, tx is a row
  const int64_t pos = mine ? (int64_t)e.map[r] : 0;
  const double wp = mine && e.wp ? e.wp[e.point[r]] : 1.0;
  double a = 0.0;
  if (e.nlev == 1) {   // one level: nothing to transpose, a row per thread of the first wave, no barrier on this path
    if (ty != 0 || !mine) return;
    double x = e.src[r * e.ld + e.off];
    if (e.mean) x = x / e.period;
    if (e.axis_op == RED_NONE) e.terms[pos] = e.domain_op <= RED_AVERAGE ? wp * x : x;
    else a = e.axis_op <= RED_AVERAGE && e.wl ? e.wl[0] * x : x;
  }
  for (int l0 = 0; e.nlev > 1 && l0 < e.nlev; l0 += 64) {
    for (int rr = ty; rr < 64; rr += 4) {       // read: levels fastest
      const int64_t q = r0 + rr;
      const int lev = l0 + tx;
      double v = 0.0;
      if (q < e.nrow && lev < e.nlev) {
        v = e.src[q * e.ld + e.off + lev];
        if (e.mean) v = v / e.period;
      }
      tile[tx][rr] = v;
    }
    __syncthreads();
    if (e.axis_op == RED_NONE) {
      if (mine)
        for (int l = ty; l < 64; l += 4)        // write: points fastest
          if (l0 + l < e.nlev) {
            const double x = tile[l][tx];
            e.terms[(int64_t)(l0 + l) * e.n2 + pos] = e.domain_op <= RED_AVERAGE ? wp * x : x;
          }
    } else if (ty == 0 && mine) {               // the row's levels of this tile, ascending
      const int n = e.nlev - l0 < 64 ? e.nlev - l0 : 64;
      for (int l = 0; l < n; ++l) {
        const double x = tile[l][tx];
        if (e.axis_op <= RED_AVERAGE) {
          const double t = e.wl ? e.wl[l0 + l] * x : x;
          a = l0 + l == 0 ? t : a + t;
        } else if (e.axis_op == RED_MIN) {
          a = l0 + l == 0 ? x : (x < a ? x : a);
        } else {
          a = l0 + l == 0 ? x : (x > a ? x : a);
        }
      }
    }
    __syncthreads();   // (the next level tile overwrites this one)
  }
  if (ty != 0 || !mine) return;
  if (e.domain_op == RED_AVERAGE) e.terms[(int64_t)(e.nslab - 1) * e.n2 + pos] = wp;
  if (e.axis_op == RED_NONE) return;
  if (e.axis_op == RED_AVERAGE) a = e.wsum == 0.0 ? e.land_value : a / e.wsum;
  if (e.domain_op == RED_NONE) e.out[pos] = a;
  else e.terms[pos] = e.domain_op <= RED_AVERAGE ? wp * a : a;
}

__global__ __launch_bounds__(256) void k_reduce_halve(const mckpp_red_plane *__restrict__ tab, int m)
{
  const mckpp_red_plane e = tab[blockIdx.z];
  if (e.domain_op == RED_NONE || (int)blockIdx.y >= e.nslab || e.n2 <= m) return;
  double *t = e.terms + (int64_t)blockIdx.y * e.n2;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;   // < m
  // A step's elements are independent of one another; eight of a thread's are loaded before any is stored, so the
  // thread waits for memory once per eight, not once per element (the compiler may not reorder them: t aliases itself).
  for (int64_t n = e.n2 >> 1; n >= m; n >>= 1) {
    int64_t i = j;
    for (; i + 7 * (int64_t)m < n; i += 8 * (int64_t)m) {
      double a[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { a[u] = t[i + u * (int64_t)m]; b[u] = t[i + u * (int64_t)m + n]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) t[i + u * (int64_t)m] = red_combine(e.domain_op, a[u], b[u]);
    }
    for (; i < n; i += m) t[i] = red_combine(e.domain_op, t[i], t[i + n]);
  }
}

__global__ __launch_bounds__(256) void k_reduce_finish(const mckpp_red_plane *__restrict__ tab, int m)
{
  __shared__ double sh[2][MCKPP_RED_M];
  const mckpp_red_plane e = tab[blockIdx.z];
  if (e.domain_op == RED_NONE || (int)blockIdx.x >= (e.axis_op == RED_NONE ? e.nlev : 1)) return;
  if (e.norows) {
    if (threadIdx.x == 0) e.out[blockIdx.x] = e.land_value;
    return;
  }
  const bool avg = e.domain_op == RED_AVERAGE;
  const int n0 = (int)(e.n2 < m ? e.n2 : m);
  const double *t = e.terms + (int64_t)blockIdx.x * e.n2, *w = e.terms + (int64_t)(e.nslab - 1) * e.n2;
  for (int i = threadIdx.x; i < n0; i += 256) {
    sh[0][i] = t[i];
    if (avg) sh[1][i] = w[i];
  }
  __syncthreads();
  for (int n = n0 >> 1; n >= 1; n >>= 1) {      // (the barriers of a workgroup depend on the plane alone)
    for (int i = threadIdx.x; i < n; i += 256) {
      sh[0][i] = red_combine(e.domain_op, sh[0][i], sh[0][i + n]);
      if (avg) sh[1][i] = sh[1][i] + sh[1][i + n];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double v = sh[0][0];
  if (avg) v = sh[1][0] == 0.0 ? e.land_value : v / sh[1][0];
  e.out[blockIdx.x] = v;
}

}  // namespace

hipError_t mckpp_launch_reduce(const mckpp_red_plane *tab, int nplanes, int phase, int maxlev, int maxslab, int64_t xtiles,
                               int m, hipStream_t stream)
{
  if (nplanes <= 0) return hipSuccess;
  const unsigned z = (unsigned)nplanes;
  if (phase == MCKPP_RED_PHASE_FILL)
    hipLaunchKernelGGL(k_reduce_fill, dim3(256, 1, z), dim3(256), 0, stream, tab);
  else if (phase == MCKPP_RED_PHASE_TERMS && xtiles > 0)
    hipLaunchKernelGGL(k_reduce_terms, dim3((unsigned)xtiles, 1, z), dim3(256), 0, stream, tab);
  else if (phase == MCKPP_RED_PHASE_HALVE && maxslab > 0)
    hipLaunchKernelGGL(k_reduce_halve, dim3((unsigned)(m / 256 > 0 ? m / 256 : 1), (unsigned)maxslab, z), dim3(m < 256 ? m : 256), 0,
                       stream, tab, m);
  else if (phase == MCKPP_RED_PHASE_FINISH && maxlev > 0)
    hipLaunchKernelGGL(k_reduce_finish, dim3((unsigned)maxlev, 1, z), dim3(256), 0, stream, tab, m);
  return hipGetLastError();
}

hipError_t mckpp_launch_put_planes(const mckpp_put_plane *tab, int nplanes, int maxlev, const int *ipt, int64_t ncol,
                                   int64_t npts, double *cs, hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0 || ncol <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_put_planes, grid, dim3(256), 0, stream, tab, ipt, ncol, npts, cs);
  return hipGetLastError();
}

hipError_t mckpp_launch_remap_put_planes(const mckpp_remap_put_plane *tab, int nplanes, int maxlev, int64_t ncol, double *cs,
                                         hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0 || ncol <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_remap_put_planes, grid, dim3(256), 0, stream, tab, ncol, cs);
  return hipGetLastError();
}

hipError_t mckpp_launch_hv_put_planes(const mckpp_hv_put_plane *tab, int nplanes, int nzp1, int64_t ncol, double *cs,
                                      hipStream_t stream)
{
  if (nplanes <= 0 || nzp1 <= 0 || ncol <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((nzp1 + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_hv_put_planes, grid, dim3(256), 0, stream, tab, ncol, cs);
  return hipGetLastError();
}

hipError_t mckpp_launch_vaxis_put_planes(const mckpp_vaxis_put_plane *tab, int nplanes, int nzp1, const int *ipt, int64_t ncol,
                                         int64_t npts, double *cs, hipStream_t stream)
{
  if (nplanes <= 0 || nzp1 <= 0 || ncol <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((nzp1 + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_vaxis_put_planes, grid, dim3(256), 0, stream, tab, ipt, ncol, npts, cs);
  return hipGetLastError();
}

hipError_t mckpp_launch_vaxis_fetch_planes(const mckpp_vaxis_fetch_plane *tab, int nplanes, int maxlev, const int *ipt,
                                           int64_t ncol, int64_t npts, const double *cs, const int *land, int64_t nland,
                                           hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0) return hipSuccess;
  const int coltiles = (int)((ncol + 63) / 64), landtiles = (int)((nland + 63) / 64);
  if (coltiles + landtiles == 0) return hipSuccess;
  dim3 grid((unsigned)(coltiles + landtiles), (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_vaxis_fetch_planes, grid, dim3(256), 0, stream, tab, ipt, ncol, npts, cs, land, nland, coltiles);
  return hipGetLastError();
}

hipError_t mckpp_launch_vaxis_init_finish(double *T, double *S, int ld, int nzp1, int64_t ncol, double *cs,
                                          const unsigned *kelvin, double tk0, int l_ssref, hipStream_t stream)
{
  if (ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vaxis_init_finish, dim3((unsigned)((ncol + 3) / 4)), dim3(256), 0, stream, T, S, ld, nzp1, ncol, cs,
                     kelvin, tk0, l_ssref);
  return hipGetLastError();
}

hipError_t mckpp_launch_record_planes(const mckpp_rec_plane *tab, int nplanes, int maxlev, int64_t xtiles, hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0 || xtiles <= 0) return hipSuccess;
  dim3 grid((unsigned)xtiles, (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_record_planes, grid, dim3(256), 0, stream, tab);
  return hipGetLastError();
}

hipError_t mckpp_launch_vaxis_record_planes(const mckpp_vrec_plane *tab, int nplanes, int maxlev, int64_t xtiles, hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0 || xtiles <= 0) return hipSuccess;
  dim3 grid((unsigned)xtiles, (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_vaxis_record_planes, grid, dim3(256), 0, stream, tab);
  return hipGetLastError();
}

hipError_t mckpp_launch_fluxes_dev(const mckpp_kparams &p, int ntime, const mckpp_dev_fields &f, const int *ipt, int l_rest,
                                   double flsn, double el, hipStream_t stream)
{
  if (p.ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fluxes_dev, dim3((unsigned)((p.ncol + 255) / 256)), dim3(256), 0, stream, p, ntime, f, ipt, l_rest,
                     flsn, el);
  return hipGetLastError();
}

hipError_t mckpp_launch_flux_gather(const mckpp_dev_fields &f, const int *ipt, int64_t ncol, double *slot, hipStream_t stream)
{
  if (ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_flux_gather, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, stream, f, ipt, ncol, slot);
  return hipGetLastError();
}

hipError_t mckpp_launch_hgrid_fluxes(const mckpp_kparams &p, int ntime, const mckpp_hgrid_ell &t, const mckpp_dev_fields &f,
                                     int l_rest, double flsn, double el, hipStream_t stream)
{
  if (p.ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_hgrid_fluxes, dim3((unsigned)((p.ncol + 255) / 256)), dim3(256), 0, stream, p, ntime, t, f, l_rest,
                     flsn, el);
  return hipGetLastError();
}

hipError_t mckpp_launch_hgrid_flux_gather(const mckpp_hgrid_ell &t, const mckpp_dev_fields &f, int64_t ncol, double *slot,
                                          hipStream_t stream)
{
  if (ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_hgrid_flux_gather, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, stream, t, f, ncol, slot);
  return hipGetLastError();
}

hipError_t mckpp_launch_hgrid_out(const mckpp_hgrid_plane *tab, int nplanes, int maxlev, int64_t maxn, hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0 || maxn <= 0) return hipSuccess;
  dim3 grid((unsigned)((maxn + 255) / 256), (unsigned)maxlev, (unsigned)nplanes);
  hipLaunchKernelGGL(k_hgrid_out, grid, dim3(256), 0, stream, tab);
  return hipGetLastError();
}

hipError_t mckpp_launch_fetch_planes(const mckpp_fetch_plane *tab, int nplanes, int maxlev, const int *ipt, int64_t ncol,
                                     int64_t npts, const double *cs, const int *land, int64_t nland, hipStream_t stream)
{
  if (nplanes <= 0 || maxlev <= 0) return hipSuccess;
  const int coltiles = (int)((ncol + 63) / 64), landtiles = (int)((nland + 63) / 64);
  if (coltiles + landtiles == 0) return hipSuccess;
  dim3 grid((unsigned)(coltiles + landtiles), (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  hipLaunchKernelGGL(k_fetch_planes, grid, dim3(256), 0, stream, tab, ipt, ncol, npts, cs, land, nland, coltiles);
  return hipGetLastError();
}

hipError_t mckpp_launch_record_pack(const mckpp_pack_plane *tab, int nplanes, int maxlev, int ring_slot, double period,
                                    const int *ipt, int64_t ncol, int64_t npts, void *dst_slot, int f32, hipStream_t stream)
{
  if (ncol <= 0 || nplanes <= 0 || maxlev <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((maxlev + 63) / 64), (unsigned)nplanes);
  if (f32)
    hipLaunchKernelGGL(k_record_pack<float>, grid, dim3(256), 0, stream, tab, ring_slot, period, ipt, ncol, npts,
                       static_cast<char *>(dst_slot));
  else
    hipLaunchKernelGGL(k_record_pack<double>, grid, dim3(256), 0, stream, tab, ring_slot, period, ipt, ncol, npts,
                       static_cast<char *>(dst_slot));
  return hipGetLastError();
}

hipError_t mckpp_launch_export_fill(void *p, size_t nelem, double v, int f32, hipStream_t stream)
{
  if (nelem == 0) return hipSuccess;
  const size_t want = (nelem + 255) / 256;
  const unsigned nb = (unsigned)(want < 8192 ? want : 8192);
  if (f32) hipLaunchKernelGGL(k_export_fill<float>, dim3(nb), dim3(256), 0, stream, static_cast<float *>(p), nelem, (float)v);
  else hipLaunchKernelGGL(k_export_fill<double>, dim3(nb), dim3(256), 0, stream, static_cast<double *>(p), nelem, v);
  return hipGetLastError();
}


// Which XCDs does this device have?  Every workgroup of a large grid ORs the bit of the XCC it runs on (read from
// the hardware) into one word: the ids of the queues of a launch of several steps (k_column_ps, M0).
__global__ void k_xcc_probe(unsigned *mask)
{
  if (threadIdx.x == 0) atomicOr(mask, 1u << (__builtin_amdgcn_s_getreg(((4 - 1) << 11) | 20 /* HW_REG_XCC_ID, bits 3:0 */) & 15));
}

hipError_t mckpp_launch_xcc_probe(unsigned *mask, hipStream_t stream)
{
  hipLaunchKernelGGL(k_xcc_probe, dim3(4096), dim3(64), 0, stream, mask);
  return hipGetLastError();
}

hipError_t mckpp_launch_eos_batch(int64_t n, const double *s, const double *t, const double *p,
                                  double *alpha, double *beta, double *sig0, double *cp,
                                  hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_eos_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, s, t, p,
                     alpha, beta, sig0, cp);
  return hipGetLastError();
}

hipError_t mckpp_launch_div_batch(int64_t n, const double *num, const double *den, double *q, hipStream_t stream)
{
  hipLaunchKernelGGL(k_div_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, num, den, q);
  return hipGetLastError();
}

hipError_t mckpp_launch_exp_batch(int64_t n, const double *x, double *y, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_exp_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, x, y);
  return hipGetLastError();
}

hipError_t mckpp_launch_gather_rows(const double *src3d, int64_t npts, int nlev, int lev_off,
                                    const int *ipt, int64_t ncol, double *dst, int ld, int dst_off,
                                    hipStream_t stream)
{
  if (ncol <= 0 || nlev <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((nlev + 63) / 64));
  hipLaunchKernelGGL(k_gather_rows, grid, dim3(256), 0, stream, src3d, npts, nlev, lev_off, ipt, ncol,
                     dst, ld, dst_off);
  return hipGetLastError();
}

hipError_t mckpp_launch_scatter_rows(const double *src, int ld, int src_off, const int *ipt,
                                     int64_t ncol, double *dst3d, int64_t npts, int nlev, int lev_off,
                                     hipStream_t stream)
{
  if (ncol <= 0 || nlev <= 0) return hipSuccess;
  dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((nlev + 63) / 64));
  hipLaunchKernelGGL(k_scatter_rows, grid, dim3(256), 0, stream, src, ld, src_off, ipt, ncol, dst3d,
                     npts, nlev, lev_off);
  return hipGetLastError();
}

hipError_t mckpp_launch_fluxes(const mckpp_kparams &p, int ntime, const double *f8, int l_rest, double flsn,
                               double el, hipStream_t stream)
{
  if (p.ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fluxes, dim3((unsigned)((p.ncol + 255) / 256)), dim3(256), 0, stream, p, ntime, f8, l_rest,
                     flsn, el);
  return hipGetLastError();
}

hipError_t mckpp_launch_bottomtemp(const mckpp_kparams &p, const double *bt, hipStream_t stream)
{
  if (p.ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bottomtemp, dim3((unsigned)((p.ncol + 255) / 256)), dim3(256), 0, stream, p, bt);
  return hipGetLastError();
}

// The per-column records <-> the caller's (npts) arrays without a host loop, for a context whose columns are all of
// the grid's points or not: forcing slabs sflux(:,1:6,5,0) (six contiguous (npts) slabs) into the records' flux
// slots, and selected record slots out into (npts) slabs in 3-D order (land points of the slabs are not written).
__global__ __launch_bounds__(256) void k_unpack_sflux(const double *__restrict__ slabs, const int *__restrict__ ipt,
                                                      double *__restrict__ cs, int64_t ncol, int64_t npts)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const int64_t i = ipt[c];
#pragma unroll
  for (int m = 0; m < 6; ++m) cs[c * MCKPP_CS + CS_SFLUX1 + m] = slabs[i + npts * m];
}

__global__ __launch_bounds__(256) void k_pack_records(const double *__restrict__ cs, const int *__restrict__ ci,
                                                      const int *__restrict__ ipt, int64_t ncol, int64_t npts,
                                                      mckpp_pack_list l, double *__restrict__ dout, int *__restrict__ iout)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const int64_t i = ipt[c];
  for (int j = 0; j < l.nd; ++j) dout[i + npts * j] = cs[c * MCKPP_CS + l.dslot[j]];
  for (int j = 0; j < l.ni; ++j) iout[i + npts * j] = ci[c * MCKPP_CI + l.islot[j]];
}

hipError_t mckpp_launch_unpack_sflux(const double *slabs, const int *ipt, double *cs, int64_t ncol, int64_t npts, hipStream_t stream)
{
  if (ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_unpack_sflux, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, stream, slabs, ipt, cs, ncol, npts);
  return hipGetLastError();
}

hipError_t mckpp_launch_pack_records(const double *cs, const int *ci, const int *ipt, int64_t ncol, int64_t npts,
                                     const mckpp_pack_list &l, double *dout, int *iout, hipStream_t stream)
{
  if (ncol <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_records, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, stream, cs, ci, ipt, ncol, npts, l, dout, iout);
  return hipGetLastError();
}

hipError_t mckpp_launch_out_sample(const double *src, int src_ld, int src_off, const double *cs, int add_sref,
                                   int64_t ncol, int nlev, int ld_out, double *sum, double *mn, double *mx, int first,
                                   double *inst, hipStream_t stream)
{
  const size_t n = (size_t)ncol * ld_out;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_out_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, src_ld, src_off, cs,
                     add_sref, ncol, nlev, ld_out, sum, mn, mx, first, inst);
  return hipGetLastError();
}

hipError_t mckpp_launch_window_mean(const double *sum, double *out, size_t n, double count, hipStream_t stream)
{
  hipLaunchKernelGGL(k_window_mean, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sum, out, n, count);
  return hipGetLastError();
}
