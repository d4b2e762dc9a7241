/* Entry points of liblocator_hip.so behind `python -m locator_amd.paint` (locator_amd/csrc/paint_kernels.hip): the haplotype
 * copying model of Li & Stephens, one normalised forward-backward recursion a recipient haplotype.  The spelling rules of
 * locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (EXTENSIONS["paint"], and the LOC_PAINT_* constants).  As in locator_hip.h: device pointers
 * unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing launched.  The
 * NumPy definition is locator_amd/paint.py: copy_host. */
#ifndef LOCATOR_HIP_PAINT_H
#define LOCATOR_HIP_PAINT_H
#include "locator_hip.h"

#define LOC_PAINT_MAX_HAPS 4096   /* most haplotype columns H: 64 values a lane */
#define LOC_PAINT_LANE_COLS 4     /* consecutive columns a lane owns in a sweep: column d is value (d / 256) * 4 + d % 4 of lane d % 256 / 4 */
#define LOC_PAINT_LL_RUN 32       /* sites whose c_j are multiplied in double before one log is taken */
#define LOC_PAINT_C_SLOTS 64      /* floats behind a scratch row of a-hat: c_j, once a lane */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- shares and chunk counts of R recipients ----
 * h [K][pitch] int8, site-major: h[j][d] = allele of haplotype column d at site j, 0 or 1, or negative = missing; columns
 * H .. pitch - 1 are never interpreted.  pitch >= H, pitch a multiple of 16, h 16-byte aligned, 1 <= H <= LOC_PAINT_MAX_HAPS,
 * K < 2^31.  donor [H] uint8 flags, owner [H] int32 (the individual of a column), rec [R] int32 (the recipient columns, each
 * 0 .. H - 1, in any order, repeats allowed), rho [K] float in [0, 1] (rho[0] is not read: it counts as 1), 1e-7 <= theta <= 0.5.
 * The launcher reads rec back to check it: one synchronisation of `stream` before the launch.
 * For recipient r = rec[i]: its donors are the columns d with donor[d] != 0 and owner[d] != owner[r], D of them, u = 1 / D.
 * All in fp32, every operation rounded on its own except the two fused multiply-adds named below:
 *   e_j(d) = 0 where d is no donor of r, else 1 where h[j][d] < 0 or h[j][r] < 0, 1 - theta where the two are equal, else theta;
 *   forward, a-hat_(-1) = 0: p = fma(1 - rho_j, a-hat_(j-1), rho_j u), a = e_j p, c_j = sum_d a, a-hat_j = a (1 / c_j);
 *   ll = sum over runs of LOC_PAINT_LL_RUN sites (j / 32 equal) of log(product of the run's c_j), product and log in double;
 *   backward from b_(K-1) = u: t = e_j b_j, T = sum_d t, g = a-hat_j b_j, G = sum_d g, 1/G read as 0 where G < FLT_MIN;
 *   gamma = g (1 / G); b_(j-1) = fma((1 - rho_j) (1 / T), t, rho_j u);
 *   share = (sum_j gamma) / K; chunks = gamma_0 + sum over j >= 1 of t ((rho_j u (1 / G)) (1 / c_j)), which is
 *   gamma rho_j u / p_j written without p_j: no quotient is formed, and rho_j = 0 adds an exact 0.
 * A sum over d: a lane adds its values d % 4 = x in ascending order for x = 0 .. 3, the four as (s0 + s1) + (s2 + s3), the
 * lanes by the butterfly 32, 16, 8, 4, 2, 1.  A column that is no donor adds an exact +0 everywhere, so appending such columns
 * changes no bit.  share [R][H], chunks [R][H] float, ll [R] double, n_donors [R] int32; row i belongs to rec[i].  No output
 * may overlap an input.  A recipient with D = 0 gets rows of zeros, ll = 0, n_donors = 0 and runs no recursion.
 * a-hat is checkpointed every `block` sites by a forward pass (which also gives ll); the backward pass recomputes one block
 * at a time into scratch by the same operations in the same order: no result depends on `block`, bit for bit.  block 0 =
 * ceil(sqrt(K)); a block above K counts as K.  One wave a recipient; no atomics; every scratch byte read was written by this
 * launch; the same arguments give the same bits.
 * work: loc_paint_work_bytes(H, K, R, block) bytes (-1 on bad sizes), 16-byte aligned.
 * R = 0 or K = 0 launches nothing; K = 0 sets share, chunks, ll and n_donors to zeros (no recursion ran). */
int64_t loc_paint_work_bytes(int H, int64_t K, int R, int block);
int loc_paint_copy(const int8_t* h, int H, int64_t K, int64_t pitch, const uint8_t* donor, const int32_t* owner,
                   const int32_t* rec, int R, const float* rho, float theta, int block,
                   float* share, float* chunks, double* ll, int32_t* n_donors,
                   void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
