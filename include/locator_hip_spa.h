/* Entry points of liblocator_hip.so behind `python -m locator_amd.spa` (locator_amd/csrc/spa_kernels.hip): logistic
 * allele-frequency surfaces fitted per site, and the genotype log-likelihood of every sample at every node of a grid.  The
 * spelling rules of locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the
 * ctypes binding from this file with the same reader (EXTENSIONS["spa"], and the LOC_SPA_* constants).  As in locator_hip.h: device
 * pointers unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing
 * launched.  The NumPy definitions are locator_amd/spa.py: fit_host and grid_host. */
#ifndef LOCATOR_HIP_SPA_H
#define LOCATOR_HIP_SPA_H
#include "locator_hip.h"

#define LOC_SPA_TILE 128        /* nodes of a tile ... */
#define LOC_SPA_TILE_SAMPLES 256 /* ... and its samples: one workgroup computes 256 samples x 128 nodes */
#define LOC_SPA_BLOCK 32        /* sites per block staged through LDS */
#define LOC_SPA_MAX_STEP 2      /* every component of a Newton step is clamped to +- this */
#define LOC_SPA_MAX_ITERS 64    /* largest number of Newton steps */
#define LOC_SPA_MAX_NODES 16384 /* largest number of grid nodes G: 128 x 128 */
#define LOC_SPA_FIT_SITES 4     /* sites per workgroup of the fit: one wave each */
#define LOC_SPA_FIT_CHUNK 1024  /* samples staged through LDS at a time by the fit: 16 a lane */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the fit: one logistic surface per site ----
 * ct [K][pitch] int8, site-major: ct[k][i] = allele-1 count of sample i at site k, 0 .. P, or negative = missing; columns
 * N .. pitch - 1 are never interpreted.  pitch >= N, pitch a multiple of 16, ct 16-byte aligned, N < 2^20, K < 2^31, P 1 or 2.
 * xy [N][2] float (8-byte aligned), w [N] uint8: site k uses the samples with w[i] == 1 and ct[k][i] >= 0; xy of a sample
 * outside w is never read, and xy of a sample of w enters no sum of a site at which its call is missing.  ridge finite and >= 0, 1 <= iters <= LOC_SPA_MAX_ITERS.
 * Over those samples n = their number, s = sum c.  The site is unused when n = 0, s = 0 or s = P n: theta = 0 0 0 0, used = 0.
 * Otherwise used = 1 and, all in fp32 with every operation rounded on its own: start ax = ay = 0, b = log(s) - log(P n - s);
 * `iters` times: t = (ax x + ay y) + b, f = 1 / (1 + exp(-t)), r = c - P f, v = (P f) (1 - f); gradient
 * (sum r x - ridge ax, sum r y - ridge ay, sum r), matrix of sum v (x, y, 1)(x, y, 1)' + ridge diag(1, 1, 0), solved by the
 * L D L' elimination without pivoting (pivots floored at 1e-30); each component of the step clamped to +- LOC_SPA_MAX_STEP and
 * added.  theta [K][4] float (16-byte aligned) = ax, ay, b, the largest absolute component of the last step.
 * Sums: lane l of the site's wave takes samples 16 l .. 16 l + 15 of every 1024 in ascending order, the 64 lanes are added by
 * a fixed butterfly: the same arguments give the same bits.  K = 0 launches nothing; N = 0 leaves every site unused. */
int loc_spa_fit(const int8_t* ct, int64_t K, int N, int64_t pitch, int P, const float* xy, const uint8_t* w, float ridge,
                int iters, float* theta, uint8_t* used, void* stream);

/* ---- the likelihood grid ----
 * c [Q][pitch] int8, sample-major, values as above; columns K .. pitch - 1 are never interpreted.  pitch >= K, pitch a
 * multiple of 16, c 16-byte aligned, Q < 2^20, K < 2^31, P 1 or 2.  theta [K][4] float (16-byte aligned; the fourth value is
 * not read) and used [K] uint8 as loc_spa_fit writes them; gx, gy [G] float: the node coordinates, 1 <= G <= LOC_SPA_MAX_NODES.
 * t[k][g] = fl(fl(fl(ax gx) + fl(ay gy)) + b), sp = max(t, 0) + log1pf(expf(-|t|)), both 0 for an unused site;
 * ll[q][g] = sum_k max(c, 0) t + sum_k (-P [c >= 0]) sp: two products on v_mfma_f32_32x32x2_f32 into two fp32 accumulators per
 * tile of LOC_SPA_TILE_SAMPLES x LOC_SPA_TILE and site group, added once in fp32 and written to the group's slab of `work`; a second kernel adds the slabs of an element in
 * group order in double and writes ll [Q][G] double (8-byte aligned).  No floating-point atomics; every scratch byte read was
 * written by this launch; the same arguments give the same bits.  A missing call and an unused site contribute exactly 0.
 * k_groups: the groups the site blocks are split over; 0 = chosen from Q, G, K and the number of compute units.  Groups that
 * would own no block are not launched.  work: loc_spa_grid_work_bytes(Q, K, G, k_groups) bytes (-1 on bad sizes), 16-byte
 * aligned.  Q = 0 launches nothing; K = 0 writes ll = 0. */
int64_t loc_spa_grid_work_bytes(int Q, int64_t K, int G, int k_groups);
int loc_spa_grid(const int8_t* c, int Q, int64_t K, int64_t pitch, int P, const float* theta, const uint8_t* used,
                 const float* gx, const float* gy, int G, int k_groups, double* ll, void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
