/* TEST INFRASTRUCTURE - own source.  Linked into oracle/_ref/libmckpp_ref_step_pexp.so with
 * -Wl,--wrap=exp: every EXP the compiled reference evaluates becomes the project's portable exp
 * (mckpp_f90_amd/csrc/mckpp_math.h: mckpp_exp), as the oracle's exp_mode=1 restates it
 * (orc_exp_portable, bit-equal to the device: test_eos_and_exp_kernels_bitexact). */
double orc_exp_portable(double x);

double __wrap_exp(double x) { return orc_exp_portable(x); }
