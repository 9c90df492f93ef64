/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.
 *
 * The long double (x86-64 80-bit) build of cdfdif_oracle.c: the same source
 * with `real` = long double and the `l` math functions, exporting
 * oracle_dmat_cdf_array_ld. See the head of cdfdif_oracle.c.
 */
#define CD_LONG 1
#include "cdfdif_oracle.c"
