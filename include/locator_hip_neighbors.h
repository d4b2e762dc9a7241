/* Entry points of liblocator_hip.so behind `python -m locator_amd.neighbors` (locator_amd/csrc/ibs_kernels.hip): the pairwise
 * identity-by-state statistics of all sample pairs over all sites on the int8 matrix pipe, and each row's nearest candidates.
 * The spelling rules of locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py
 * derives the ctypes binding from this file with the same reader (EXTENSIONS["neighbor"], and the LOC_IBS_* constants).  As in
 * locator_hip.h: device pointers unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with
 * loc_last_error set and nothing launched. */
#ifndef LOCATOR_HIP_NEIGHBORS_H
#define LOCATOR_HIP_NEIGHBORS_H
#include "locator_hip.h"

#define LOC_IBS_TILE 128   /* rows per side of a tile pair: one workgroup computes a 128 x 128 block of d and n */
#define LOC_IBS_BLOCK 64   /* sites per block staged through LDS */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pair statistics (exact integers) ----
 * c [n_rows][pitch] int8: c[s][v] = allele-1 count of sample s at site v, 0 .. 2, or negative = missing; columns K .. pitch - 1
 * are never interpreted.  pitch >= K, pitch a multiple of 16, c 16-byte aligned.  Over the sites v < K where both c[i][v] >= 0
 * and c[j][v] >= 0:  n[i][j] = their number, d[i][j] = sum |c[i][v] - c[j][v]|; d, n [n_rows][n_rows] int32, both symmetric,
 * d[i][i] = 0.  A count of 3 .. 127 is outside the contract (the planes below read its two low bits); 2 * K must stay below 2^31.
 * With the byte planes m = [c >= 0], t1 = [c >= 1], t2 = [c >= 2], a = t1 + t2:  n = M M',  d = A M' + M A' - 2 (T1 T1' + T2 T2'),
 * int8 products accumulated in int32.  The sites are split over k_groups groups of workgroups, group q owning a contiguous
 * run of LOC_IBS_BLOCK-site blocks (0 = chosen by the launcher from n_rows, K and the number of compute units; groups past
 * the last block are not launched); with more than one group launched the outputs are zeroed on `stream` and the groups add
 * their integer shares with atomics, so the result is the same for every k_groups.  work / work_bytes: scratch of at least loc_ibs_work_bytes(n_rows, K, k_groups) bytes; this version needs none
 * (the function returns 0 and work may be null). */
int64_t loc_ibs_work_bytes(int n_rows, int64_t K, int k_groups);
int loc_ibs_pairs(const int8_t* c, int n_rows, int64_t K, int64_t pitch, int k_groups, int32_t* d, int32_t* n, void* work,
                  int64_t work_bytes, void* stream);

/* ---- nearest candidates of every row ----
 * d, n [n_rows][n_rows] as above; P = 1 or 2.  D[i][j] = (double)d[i][j] / (double)(P * n[i][j]), one correctly rounded
 * division, defined where n[i][j] > 0.  candidate [n_rows] uint8: j may be a neighbour when candidate[j] != 0.  For every
 * row i: nbr[i][r], r = 0 .. kmax - 1, = the candidates j != i with n[i][j] > 0 in ascending (D[i][j], j) order (equal
 * doubles go to the lower j), -1 past the last; nbr_dist[i][r] = that D, NaN past the last.  nbr [n_rows][kmax] int32,
 * nbr_dist [n_rows][kmax] double; 1 <= kmax <= 64.  An answer does not depend on the launch. */
int loc_ibs_knn(const int32_t* d, const int32_t* n, int n_rows, int P, const uint8_t* candidate, int kmax, int32_t* nbr,
                double* nbr_dist, void* stream);

#ifdef __cplusplus
}
#endif
#endif
