/* Entry point of liblocator_hip.so behind `python -m locator_amd.impute` (locator_amd/csrc/impute_kernels.hip): the allele
 * dosage of every site of a recipient haplotype under the copying model of locator_hip_paint.h.  The spelling rules of
 * locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (EXTENSIONS["impute"], and the LOC_IMPUTE_* constants).  As in locator_hip.h: device pointers
 * unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing launched.  The
 * NumPy definition is locator_amd/impute.py: dose_host. */
#ifndef LOCATOR_HIP_IMPUTE_H
#define LOCATOR_HIP_IMPUTE_H
#include "locator_hip_paint.h"

#define LOC_IMPUTE_STORE_RUN 64   /* consecutive sites of a recipient that one store instruction writes: lane j % 64 holds site j */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dosages of R recipients ----
 * h, H, K, pitch, donor, owner, rec, R, rho, theta, block, ll, n_donors, work and stream are loc_paint_copy's, with its sizes,
 * alignments, refusals and the read-back of rec; the donors of a recipient, u, e_j, the forward pass, ll, t, T, g and b_(j-1)
 * are its too, in fp32 by the same operations in the same order: ll and n_donors are the same bits as loc_paint_copy's for the
 * same arguments.  In the backward walk at site j, in place of share and chunks:
 *   A1 = sum_d of g where h[j][d] == 1, A0 = sum_d of g where h[j][d] == 0 (a column with a negative allele adds +0 to both);
 *   S = A0 + A1; dose[i][j] = min(A1 (1 / S), 1) where S >= FLT_MIN, else NaN: no donor holds an allele there, or the sums
 *   have underflowed.  1 / S is a division; the normalisation 1 / G of gamma cancels and G is not formed.
 * A0 and A1 are sums over d by the rule of locator_hip_paint.h: a lane's four column classes in ascending order, the four as
 * (s0 + s1) + (s2 + s3), the lanes by the butterfly 32 .. 1.  dose [R][K] float, row i belongs to rec[i]; a recipient with
 * D = 0 gets a row of NaN, ll = 0, n_donors = 0.  Every element of dose is written exactly once and nothing outside it: lane
 * j % LOC_IMPUTE_STORE_RUN keeps site j's value and the wave stores each run of up to 64 consecutive sites at once.
 * No result depends on `block`, on what scratch or the outputs held, on appended non-donor columns, on appended recipients or
 * on how rec is split over launches, bit for bit.  One wave a recipient; no atomics.
 * work: loc_paint_work_bytes(H, K, R, block) bytes, 16-byte aligned, laid out as for loc_paint_copy.
 * R = 0 or K = 0 launches nothing; K = 0 sets ll and n_donors to zeros and writes no dose. */
int loc_impute_dose(const int8_t* h, int H, int64_t K, int64_t pitch, const uint8_t* donor, const int32_t* owner,
                    const int32_t* rec, int R, const float* rho, float theta, int block,
                    float* dose, double* ll, int32_t* n_donors,
                    void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
