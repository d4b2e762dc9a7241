/* Entry points of liblocator_hip.so added after version 1 of the C ABI.  include/locator_hip.h is that version, and
 * tests/test_abi.py pins its list of prototypes; a later entry point is declared here, in the same spelling (one declaration
 * per `;`, comments only as this one), and locator_amd/_abi.py derives its ctypes binding from this file in the same way
 * (EXTENSIONS["ext"]).  The rules of locator_hip.h hold: device pointers unless named h_*, `stream` a hipStream_t, 0 = success,
 * -1 = bad arguments with loc_last_error set and nothing launched. */
#ifndef LOCATOR_HIP_QUERY_H
#define LOCATOR_HIP_QUERY_H
#include "locator_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a kept model on a --dosage query (python -m locator_amd.predict / explain --dosage; locator_amd/query.py) ----
 * The form of loc_query_rows for float dosages: ds = the query's expected alt-allele dosages float32 [n_variants][n_samples]
 * (NaN = missing; every offset 64-bit), X in the q units of a LocatorNet(unit = LOC_DOSAGE_UNIT).  With
 * q = rint(fp32(d) * LOC_DOSAGE_UNIT) clamped to 0..2 * LOC_DOSAGE_UNIT, d = ds[col_variant[k]][sample_order[r]]:
 * X[r][k] = q when col_allele[k] == 1, 2 * LOC_DOSAGE_UNIT - q when col_allele[k] == 0 (REF/ALT swap; the flip follows the
 * quantisation, so a value and its flip sum to 126 exactly), and 0 for an absent or out-of-range column, any other
 * col_allele, or a NaN.  Columns K .. x_pitch are not written.  Bit-identical to genotypes.dosage_q on the host. */
int loc_query_rows_dosage(const float* ds, int64_t n_variants, int n_samples, const int32_t* col_variant,
                          const int8_t* col_allele, int K, const int32_t* sample_order, int n_out, uint8_t* X,
                          int64_t x_pitch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
