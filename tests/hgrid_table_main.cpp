// hgrid_table_main.cpp - the three host functions of include/mckpp_hip_hgrid.h on their own, for a build under the
// sanitizers (tests/test_hgrid_cpu.py): compiled together with mckpp_f90_amd/csrc/mckpp_hgrid_table.cpp, without HIP and
// without the library.
//
// Input (argv[1]): any number of cases.  A case is a line "nrows nsrc nnz nlist norm fill" followed by the nrows + 1
// values of ptr, the nnz indices, the nnz weights, the nsrc source values, the nsrc bytes of the used / keep mask, the
// nlist listed rows and the land value - numbers in floating point are hexadecimal.  Every array is a heap block of
// exactly its length, so a read or write past a table, a mask or a slice is seen.
// Output per case: "check rc"; "apply" and the nrows values (norm < 0: the in direction without a mask; otherwise the
// out direction with the mask, every output starting as -7.0); "slices padded", then slice_off, len, and the padded
// idx and w.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mckpp_hip_hgrid.h"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  long long nrows, nsrc, nnz, nlist;
  int norm, fill;
  while (fscanf(f, "%lld %lld %lld %lld %d %d", &nrows, &nsrc, &nnz, &nlist, &norm, &fill) == 6) {
    if (nrows < 0 || nsrc < 0 || nnz < 0 || nlist < 0) return 2;
    std::vector<int64_t> ptr((size_t)nrows + 1), rows((size_t)nlist);
    std::vector<int32_t> idx((size_t)nnz);
    std::vector<double> w((size_t)nnz), x((size_t)nsrc), out((size_t)nrows, -7.0);
    std::vector<unsigned char> mask((size_t)nsrc);
    double land = 0.0;
    for (auto &v : ptr) { long long q; if (fscanf(f, "%lld", &q) != 1) return 2; v = q; }
    for (auto &v : idx) { int q; if (fscanf(f, "%d", &q) != 1) return 2; v = q; }
    for (auto &v : w) if (fscanf(f, "%la", &v) != 1) return 2;
    for (auto &v : x) if (fscanf(f, "%la", &v) != 1) return 2;
    for (auto &v : mask) { int q; if (fscanf(f, "%d", &q) != 1) return 2; v = (unsigned char)q; }
    for (auto &v : rows) { long long q; if (fscanf(f, "%lld", &q) != 1) return 2; v = q; }
    if (fscanf(f, "%la", &land) != 1) return 2;
    const mckpp_hgrid_table_c t{ptr.data(), idx.data(), w.data()};
    std::vector<char> msg(200);
    const int rc = mckpp_host_hgrid_check("t", nrows, nsrc, &t, msg.data(), (int64_t)msg.size());
    printf("check %d\n", rc);
    if (rc != 0) { printf("%s\n", msg.data()); continue; }
    if (mckpp_host_hgrid_apply(nrows, &t, x.data(), norm < 0 ? nullptr : mask.data(), norm, fill, land, out.data()) != 0) return 3;
    printf("apply\n");
    for (double v : out) printf("%a\n", v);
    const size_t nslices = ((size_t)nlist + 63) / 64;
    std::vector<int64_t> off(nslices + 1);
    std::vector<int32_t> len((size_t)nlist);
    const int64_t padded = mckpp_host_hgrid_slices(nlist, rows.data(), &t, mask.data(), off.data(), len.data(), nullptr, nullptr);
    if (padded < 0) return 3;
    std::vector<int32_t> ei((size_t)padded);
    std::vector<double> ew((size_t)padded);
    if (mckpp_host_hgrid_slices(nlist, rows.data(), &t, mask.data(), off.data(), len.data(), ei.data(), ew.data()) != padded) return 3;
    printf("slices %lld\n", (long long)padded);
    for (int64_t v : off) printf("%lld ", (long long)v);
    printf("\n");
    for (int32_t v : len) printf("%d ", v);
    printf("\n");
    for (int32_t v : ei) printf("%d ", v);
    printf("\n");
    for (double v : ew) printf("%a ", v);
    printf("\n");
  }
  fclose(f);
  // the refusals that read nothing
  double one = 0.0;
  int64_t i64 = 0;
  const mckpp_hgrid_table_c none{nullptr, nullptr, nullptr};
  if (mckpp_host_hgrid_check("t", 1, 1, &none, nullptr, 0) != -1) return 4;
  if (mckpp_host_hgrid_apply(1, &none, &one, nullptr, 0, 1, 0.0, &one) != -1) return 4;
  if (mckpp_host_hgrid_slices(0, nullptr, &none, nullptr, &i64, nullptr, nullptr, nullptr) != -1) return 4;
  return 0;
}
