// vaxis_map_main.cpp - mckpp_host_vaxis_map on its own, for a build under the sanitizers (tests/test_vaxis_cpu.py):
// compiled together with mckpp_f90_amd/csrc/mckpp_vaxis_map.cpp, without HIP and without the library.
//
// Input (argv[1]): any number of cases "ns nt" followed by the ns source and the nt target levels, as hexadecimal
// floating-point numbers.  Every array is a heap block of exactly its length, so a read or write past an axis is seen.
// Output: per case a line "rc" and, where rc is 0, a line per target: branch kin t dz (t and dz hexadecimal).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mckpp_hip_vaxis.h"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int ns = 0, nt = 0;
  while (fscanf(f, "%d %d", &ns, &nt) == 2) {
    if (ns < 0 || nt < 0) return 2;
    std::vector<double> zs((size_t)ns), zt((size_t)nt), t((size_t)nt), dz((size_t)nt);
    std::vector<int32_t> branch((size_t)nt), kin((size_t)nt);
    for (double &z : zs)
      if (fscanf(f, "%la", &z) != 1) return 2;
    for (double &z : zt)
      if (fscanf(f, "%la", &z) != 1) return 2;
    const int rc = mckpp_host_vaxis_map(ns, zs.data(), nt, zt.data(), branch.data(), kin.data(), t.data(), dz.data());
    printf("%d\n", rc);
    for (int j = 0; rc == 0 && j < nt; ++j) printf("%d %d %a %a\n", branch[(size_t)j], kin[(size_t)j], t[(size_t)j], dz[(size_t)j]);
  }
  fclose(f);
  // the refusals that read nothing
  double one = 0.0;
  int32_t i = 0;
  if (mckpp_host_vaxis_map(2, nullptr, 1, &one, &i, &i, &one, &one) != -1) return 3;
  if (mckpp_host_vaxis_map(1, &one, 1, &one, &i, &i, &one, &one) != -1) return 3;
  if (mckpp_host_vaxis_map(2, &one, 0, &one, &i, &i, &one, &one) != -1) return 3;
  return 0;
}
