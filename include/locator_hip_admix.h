/* Entry points of liblocator_hip.so behind `python -m locator_amd.admix` (locator_amd/csrc/admix_kernels.hip): one EM step of
 * the model-based ancestry proportions (FRAPPE's map, the model of STRUCTURE and ADMIXTURE).  The spelling rules of
 * locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (EXTENSIONS["admix"], and the LOC_ADMIX_* constants).  As in locator_hip.h: device pointers
 * unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing launched.  The
 * NumPy definition is locator_amd/admix.py: step_host. */
#ifndef LOCATOR_HIP_ADMIX_H
#define LOCATOR_HIP_ADMIX_H
#include "locator_hip.h"

#define LOC_ADMIX_MAX_POPS 16   /* largest number of clusters C */
#define LOC_ADMIX_LL_RUN 1024   /* most terms any fp32 partial sum of ll holds before it continues in double */
#define LOC_ADMIX_TILE 64       /* samples of a tile of the Q-pass: one a lane */
#define LOC_ADMIX_BLOCK 64      /* sites of a block: one a lane in the F-pass, the unit the site groups of the Q-pass own */
#define LOC_ADMIX_SPLIT 4       /* waves of an F-pass workgroup: wave w walks the samples w, w + 4, ... */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one EM step ----
 * c [N][pitch] int8, sample-major: c[i][k] = allele-1 count of sample i at site k, 0 .. P, or negative = missing; columns
 * K .. pitch - 1 are never interpreted.  pitch >= K, pitch a multiple of 16, c 16-byte aligned, N < 2^20, K < 2^31, P 1 or 2,
 * 2 <= C <= LOC_ADMIX_MAX_POPS.  Q [N][C] float (rows on the simplex), F [K][C] float (allele-1 frequency of cluster c at site
 * k, inside (0, 1)); Q_out [N][C], F_out [K][C]; the four are 16-byte aligned and no output overlaps an input or the other
 * output.  ll: one double, 8-byte aligned.
 * With m = [c >= 0], g = m c, r = m (P - c), Fb = 1 - F, EPS = 1e-5, all in fp32 with every operation rounded on its own:
 *   h[i][k] = sum_c Q[i][c] F[k][c], hb[i][k] = sum_c Q[i][c] Fb[k][c] (a sum of its own, not 1 - h), clusters in ascending order;
 *   a = g / h, b = r / hb, formed as g rcp(h), r rcp(hb) with the hardware reciprocal (1 ulp);
 *   A[k][c] = sum_i Q[i][c] a[i][k], B likewise from b: wave w of the site's workgroup adds the samples w, w + 4, ... in
 *   ascending order, the LOC_ADMIX_SPLIT partial sums are added in wave order;
 *   F_out = F A / (F A + Fb B), F where that denominator is 0; then clipped to [EPS, 1 - EPS];
 *   S[i][c] = sum_k F[k][c] a[i][k] + Fb[k][c] b[i][k]: a site group adds its sites in ascending order into its slab of `work`,
 *   the slabs are added in group order; n_i = sum_k m, an integer;
 *   Q_out = Q S / (P n_i), Q where n_i = 0; then max(., EPS) and divided by the sum of the row, clusters in ascending order;
 *   ll = sum g logf(h) + r logf(hb), the log-likelihood of the INPUT (Q, F): a lane of the F-pass adds the two terms of at most
 *   LOC_ADMIX_LL_RUN / 2 consecutive samples of its own in fp32, then continues in double; lanes, waves and workgroups are
 *   added in double in a fixed order.
 * Exact: a missing call contributes exactly 0 to every sum; a sample with no called site keeps its row of Q, bit for bit, up to
 * the floor and renormalisation; a site with no called sample keeps its row of F up to the clip.
 * No floating-point atomics; every scratch byte read was written by this launch; the same arguments give the same bits.
 * k_groups: the groups the site blocks of the Q-pass are split over; 0 = chosen from N, K and the number of compute units.
 * Groups that would own no block are not launched.  Different k_groups add S in different orders.
 * work: loc_admix_work_bytes(N, K, C, k_groups) bytes (-1 on bad sizes), 16-byte aligned.
 * N = 0 or K = 0 launches nothing: K = 0 copies Q to Q_out and sets ll = 0 (no call: no row moves), N = 0 copies F to F_out and sets ll = 0. */
int64_t loc_admix_work_bytes(int N, int64_t K, int C, int k_groups);
int loc_admix_step(const int8_t* c, int N, int64_t K, int64_t pitch, int P, int C, const float* Q, const float* F,
                   float* Q_out, float* F_out, double* ll, int k_groups, void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
