"""The class and the reason of every comparison of oracle/mckpp_oracle.c that survives tools/oracle_boundaries.py with
the edge cases in: {(function, source line, n-th such line, m-th comparison): (class, reason)}.  A loop bound whose
last trip nothing reads is recognised by its text (LAST_TRIP) - the same line recurs in several functions."""

SAME, UNREAD, UNREACHABLE = "same either way", "last trip unread", "not reachable from the reference"

CLASSES = {
    ("orc_cpsw", "if (T < -2.) T = -2.;                                   /* :28-29 */", 0, 0):
        (SAME, "A clamp to the compared value."),
    ("orc_abk80", "if (T < -2.) T = -2.;                                   /* :143-144 */", 0, 0):
        (SAME, "A clamp to the compared value."),
    ("orc_wscale", "if (iz > ni) iz = ni;", 0, 0): (SAME, "A clamp to the compared value."),
    ("orc_wscale", "if (iz < 0) iz = 0;", 0, 0): (SAME, "A clamp to the compared value."),
    ("orc_wscale", "if (ju > nj) ju = nj;", 0, 0): (SAME, "A clamp to the compared value."),
    ("orc_wscale", "if (ju < 0) ju = 0;", 0, 0): (SAME, "A clamp to the compared value."),
    ("tridrhs", "if (npd >= 2) {                                         /* :85-93 */", 0, 0):
        (UNREACHABLE, "ocnint hands tridrhs npd = 1, a constant (ocnint_mod.F90:70), in the reference and here: npd == 2 "
                      "has no input."),
    ("tridrhs", "for (int i = 2; i <= npd; i++)", 0, 0):
        (UNREACHABLE, "Inside `npd >= 2`, which npd = 1 never enters."),
    ("tridrhs", "if (nzi > 1) {                                          /* :102-106 */", 0, 0):
        (UNREACHABLE, "nzi == 1 is a grid of one level, on which bldepth's loop from level 2 to km = NZ does not run and "
                      "hbl, kbl stay unset in the reference; the library refuses fewer than 2 levels."),
    ("orc_tridmat_2e", "if (nzi < 2) return orc_tridmat(cu, cc, cl, rhs, yo, nzi, yn, gam);", 0, 0):
        (UNREACHABLE, "Solver mode 1 is the library's own order of operations, the reference has none to record; nzi == 2 "
                      "is a grid of two levels, below the 12 levels of the smallest recorded case.  Tried: nothing beyond "
                      "the mode-1 pass over the cases."),
    ("ntflux", "if (ntime <= 1)                                         /* :103-108 */", 0, 0):
        (SAME, "At ntime == 1 the branch recomputes swdk_opt from dm and jerlov, which init_ocean (ntime = 0) already "
               "did from the same values."),
    ("ddmix", "if ((aDT > bDS) && (bDS > 0.)) {                      /* :31-36 */", 0, 1):
        (SAME, "At bDS == 0 the arm needs aDT > 0, so aDT / bDS = +inf, Rrho = Rrho0, (Rrho - 1) / (Rrho0 - 1) = 1 and "
               "diffdd = 0 exactly: the arm adds +0 to dift and difs.  edge_ldd_equal_nz40 holds the column (betaDS = 0 "
               "under a falling temperature) and the reference agrees on it; no output can tell the two operators apart."),
    ("ddmix", "} else if ((aDT < 0.0) && (bDS < 0.0) && (aDT < bDS)) { /* :39-48 */", 0, 0):
        (SAME, "At aDT == 0 the arm also needs bDS < 0 and aDT < bDS, and 0 < bDS is then false."),
    ("ddmix", "if (Rrho > 0.5) prandtl = (1.85 - 0.85 / Rrho) * Rrho;", 0, 0):
        (UNREACHABLE, "Inside the arm aDT < bDS < 0, so Rrho = aDT / bDS >= 1 after rounding: it is never 0.5 (and never "
                      "below it: the false branch has no input either, profiles/coverage/oracle_branches.md)."),
    ("hbl_winner", "if (floor < others) return p | ORC_PATH_HBL_SEAFLOOR;", 0, 0):
        (SAME, "hbl_winner only names the limit that won in the `paths` word, test bookkeeping that no compared output "
               "reads; bldepth takes hbl from fmin2 of the four, which a tie does not move.  (The device has no "
               "counterpart of this comparison.)"),
    ("bldepth", "if (ntime <= 1 && kl == 2) swfrac_opt(c, q, hbf);     /* :113-115 */", 0, 0):
        (SAME, "At ntime == 1 swfrac is recomputed from zm and jerlov, as init_ocean (ntime = 0) left it."),
    ("bldepth", "if (dmo[ku] <= (-zm[kl])) {                                           /* :148-153 */", 0, 0):
        (SAME, "At dmo(ku) == -zm(kl) the interpolation gives hmonob = -zm(kl), which is not `< -zm(kl)`: no hit at this "
               "level with either operator, and the next level meets the same dmo.  Tried: the fifth triple of "
               "edge_zero_flux_nz40 (0.02 N/m2, 55.73046706341893 W/m2 over uniform water: dmo = 7.5 m by the same "
               "operations in numpy); the mutant leaves every bit of it alike.  A rounding of the interpolation below "
               "-zm(kl) would tell them apart; none was met."),
    ("vmix", "if (zref >= zm[kl]) break;                          /* :119 */", 0, 0):
        (SAME, "At zref == zm(kl) going on gives wz = MIN(zm(kl) - zm(kl+1), zm(kl) - zref) = 0: the trip subtracts "
               "0 * (...) / zref from uref, vref and bref, and the next level breaks.  (On a uniform grid 0.1 zm(n) is "
               "no level centre: n - 1/2 = 10 (kl - 1/2) has no integer solution.)"),
    ("rhsmod", "if (mode <= 0) return;                                  /* :207 */", 0, 0):
        (SAME, "A mode of 0 that is let through matches none of the modes 1 ... 7 and returns at the end "
               "(adv_modes_nz60 has zero modes between live ones)."),
    ("rhsmod", "do { n1 = n1 + 1; } while (c->zm[n1] >= -100. && n1 < nzi + 1);", 0, 1):
        (UNREACHABLE, "The guard is the oracle's and the kernel's own: n1 reaches nzi + 1 only on a grid with no level "
                      "below 100 m, where the reference reads past zm (solvers.F90:258-259).  The device and the oracle "
                      "are compared there (test_mode_4_on_a_grid_shallower_than_100_m_is_a_no_op)."),
}

# loop bounds: what the last trip of the swapped bound no longer writes, and why nothing reads it
LAST_TRIP = {
    ("blmix", "for (int ki = 1; ki <= km; ki++) {                                        /* :110-133 */"):
        "blmc(km,:) and ghat(km): kppmix copies blmc only for ki < kbl <= km, and vmix sets ghat(nz) = 0 after it.",
    ("kppmix", "for (int ki = 0; ki <= km; ki++) {                      /* :65-69 */"):
        "The zeroing of difm, difs, dift at km = NZ: vmix overwrites levels NZ and NZP1 with the background values "
        "(verticalmixing_mod.F90:154-158), after rimix has rewritten 1 ... km.  With LRI = 0 (lri0) rimix does not, and "
        "what the previous step left at km, those same background values, would be read by blmix alone and only at "
        "kn + 1 = km: a boundary layer ending in the last level, which lri0 does not have.",
    ("kppmix", "for (int ki = 1; ki <= km; ki++) {                    /* :103-111 */"):
        "ki = km is never below kbl <= km, so the trip only sets ghat(km) = 0, which vmix does again (:159).",
    ("vmix", "for (int kl = 1; kl <= nz; kl++) {"):
        "The loop leaves through `zref >= zm(kl)` long before kl = nz: zref = 0.1 zm(n) lies above the last level.",
    ("rhsmod", "for (int n = n1; n <= nzi; n++) {"):
        "Mode 6 meets dmax by n = km - 1 < nzi (tests/ref_step_cases.py, 'prescribed advection'): the trip n = nzi "
        "does not happen with either bound.",
    ("ocnint", "for (int k = 0; k <= NZP1; k++) diff[k] = q->difm[k];   /* :45-47 */"):
        "diff(NZP1): tridcof reads diff(0 ... NZ) only.",
    ("ocnint", "for (int k = 1; k <= NZP1; k++) {                       /* :86-90 */"):
        "diff(NZP1), gcap(NZP1), ntflx(NZP1): tridcof and tridrhs read up to NZ.",
    ("ocnint", "for (int k = 0; k <= NZP1; k++) diff[k] = q->difs[k];   /* :165-167 */"):
        "diff(NZP1): tridcof reads diff(0 ... NZ) only.",
    ("ocnint", "for (int k = 0; k <= NZP1; k++) q->ntflx[n][k] = q->wXNT[n][k];         /* :170-172 */"):
        "ntflx(NZP1,2): tridrhs reads up to NZ (and wXNT(:,2) is zero throughout).",
    ("ocnstep", "for (int k = 1; k <= NZP1; k++) {"):
        "The rms sums' term of level NZP1 carries hm(NZP1) = 1e-10 m and a level that ocnint does not change: it adds "
        "exactly zero.",
}

NOTES = """
## What is left, and why

Classes: **pinned**: killed by the edge case named.  **same either way**: at equality both branches compute the
same bits.  **last trip unread**: a loop bound whose final iteration writes only what nothing later reads.  **not
reachable from the reference**: equality needs an input the reference cannot be given, or has no definition on.

- The reference's `iter .gt. (itermax+1)` and `reset_flag .gt. comp_iter_max` (ocnstep_mod.F90:184, :229) only print
  warnings: the reference's outputs cannot pin them.  They set the oracle's and the kernel's status bits, which every
  comparison with the oracle includes.  `iter > itermax + 1` was already killed by the parent commit's cases
  (nz40_diurnal_itermax); edge_itermax3_nz40 puts every column that does not deepen on iter == itermax + 1 and those
  that deepen once one past it.
- The prototype of this record counted 68 survivors of 151 mutants on the recorded cases alone; its 151 included the
  lookup-table builder, the batch probes' loops and col_new, which are no sites here (131), and it left out the
  generators' inputs, the mode-1 pass and vmix_only / vmix_batch, which kill some more.
- `rc.canonical` counts -0.0 equal to +0.0 and every NaN equal to every other: a comparison whose two branches differ
  only in the sign of a zero or in which NaN they make is invisible to this record.  That is a separate, smaller
  blind spot, left as it is.
- The values of tests/ref_step_cases.py's EXACT_* and EKMAN_F_EDGE put the end of a rounding chain on its threshold
  bit for bit.  They were found by bisecting the oracle on one input over a few hundred second inputs an ulp apart,
  with the swapped comparison as the probe (where `>=` traps and `>` does not, the two sides are equal); the reference
  was then recorded on them and agrees.

The sites still surviving:
"""
