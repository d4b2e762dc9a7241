/* Entry point of liblocator_hip.so behind `python -m locator_amd.ancestry` (locator_amd/csrc/local_kernels.hip): the copying
 * posterior of locator_hip_paint.h summed per window of sites and contracted with attributes of the donors.  The spelling rules
 * of locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (OPEN["local"], and the LOC_LOCAL_* constants).  As in locator_hip.h: device pointers
 * unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing launched.  The
 * NumPy definition is locator_amd/ancestry.py: local_host. */
#ifndef LOCATOR_HIP_LOCAL_H
#define LOCATOR_HIP_LOCAL_H
#include "locator_hip_paint.h"

#define LOC_LOCAL_MAX_CHANNELS 64   /* most channels C: lane c keeps channel c of a window until the wave stores the window */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- window sums of the posterior of R recipients, contracted with C attributes of the donors ----
 * h, H, K, pitch, donor, owner, rec, R, rho, theta, block, ll, n_donors, work and stream are loc_paint_copy's, with its sizes,
 * alignments, refusals and the read-back of rec; the donors of a recipient, u, e_j, the forward pass, ll, t, T, g, G, gamma
 * (1 / G read as 0 where G < FLT_MIN) and b_(j-1) are its too, in fp32 by the same operations in the same order: ll and n_donors
 * are the same bits as loc_paint_copy's for the same arguments.
 * v [C][vpitch] float, channel-major: v[c][d] = attribute c of column d; 1 <= C <= LOC_LOCAL_MAX_CHANNELS, vpitch >= H and a
 * multiple of 4, v 16-byte aligned.  The values at donor columns must be finite (not checked); a column that is no donor of the
 * recipient is skipped by the donor mask and its value is never interpreted, NaN included.
 * win [W][2] int32: the windows [v0, v1) of sites, W >= 1, 0 <= v0 < v1 <= K, ascending and disjoint (v1 of a window <= v0 of
 * the next); gaps are allowed.  The launcher reads win back with rec, in the same synchronisation, and refuses a bad window by
 * its index.  K = 0 admits no window and is refused.  The refusals of the sizes (loc_paint_copy's, then C, W, vpitch, K = 0)
 * come before R = 0 returns 0.
 * In the backward walk, S_w(d) = the fp32 sum of gamma_j(d) for j = v1 - 1 down to v0 from +0; a site in no window adds nowhere.
 * When the walk arrives at v0: out[i][w][c] = sum over the recipient's donors d of S_w(d) v[c][d]: a lane forms
 * p = fma(S, v, p) from +0 over its donor columns in ascending (sweep, x) order, the lanes add by the butterfly 32 .. 1; then S
 * is cleared.  out is this plain sum: nothing is divided by the window's length.
 * out [R][W][C] float, row i belongs to rec[i]; lane c keeps channel c and the wave writes a window's C values with one store
 * instruction: every element of out is written exactly once and nothing outside it.  A recipient with D = 0 gets zeros, ll = 0,
 * n_donors = 0.
 * No result depends on `block`, on what scratch or the outputs held, on pad columns or vpitch, on appended non-donor columns, on
 * appended recipients or on how rec is split over launches, on which other windows or which other channels are in the call, bit
 * for bit.  One wave a recipient; no atomics.
 * work: loc_paint_work_bytes(H, K, R, block) bytes, 16-byte aligned, laid out as for loc_paint_copy.  R = 0 launches nothing. */
int loc_paint_local(const int8_t* h, int H, int64_t K, int64_t pitch, const uint8_t* donor, const int32_t* owner,
                    const int32_t* rec, int R, const float* rho, float theta, int block,
                    const float* v, int C, int64_t vpitch, const int32_t* win, int W,
                    float* out, double* ll, int32_t* n_donors,
                    void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
