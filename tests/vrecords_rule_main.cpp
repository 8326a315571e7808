// vrecords_rule_main.cpp - mckpp_host_vaxis_map and mckpp_host_vrecords_rule on their own, for a build under the
// sanitizers (tests/test_vrecords_cpu.py): compiled together with mckpp_f90_amd/csrc/mckpp_vaxis_map.cpp, without HIP and
// without the library.
//
// Input (argv[1]): any number of cases "ns nt lev0 nlev" followed by the ns model levels and the nt caller levels, as
// hexadecimal floating-point numbers.  Every array is a heap block of exactly its length, so a read past a table is seen.
// Output: per case a line "rc caller_level model_level" of the rule on the out table of the caller's levels (-1 -1 where
// the rule does not report them).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mckpp_hip_vrecords.h"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int ns = 0, nt = 0, lev0 = 0, nlev = 0;
  while (fscanf(f, "%d %d %d %d", &ns, &nt, &lev0, &nlev) == 4) {
    if (ns < 0 || nt < 0) return 2;
    std::vector<double> zs((size_t)ns), zt((size_t)nt), t((size_t)nt), dz((size_t)nt);
    std::vector<int32_t> branch((size_t)nt), kin((size_t)nt);
    for (double &z : zs)
      if (fscanf(f, "%la", &z) != 1) return 2;
    for (double &z : zt)
      if (fscanf(f, "%la", &z) != 1) return 2;
    if (mckpp_host_vaxis_map(ns, zs.data(), nt, zt.data(), branch.data(), kin.data(), t.data(), dz.data()) != 0) return 2;
    int32_t j = -1, lev = -1;
    const int rc = mckpp_host_vrecords_rule(nt, branch.data(), kin.data(), lev0, nlev, &j, &lev);
    printf("%d %d %d\n", rc, j, lev);
    // the places of the report may be null
    if (mckpp_host_vrecords_rule(nt, branch.data(), kin.data(), lev0, nlev, nullptr, nullptr) != rc) return 3;
  }
  fclose(f);
  // the refusals that read nothing
  int32_t i = 0;
  if (mckpp_host_vrecords_rule(1, nullptr, &i, 0, 1, &i, &i) != -1) return 3;
  if (mckpp_host_vrecords_rule(1, &i, nullptr, 0, 1, &i, &i) != -1) return 3;
  if (mckpp_host_vrecords_rule(0, &i, &i, 0, 1, &i, &i) != -1) return 3;
  if (mckpp_host_vrecords_rule(1, &i, &i, 0, 0, &i, &i) != -1) return 3;
  return 0;
}
