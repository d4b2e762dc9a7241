/* Entry points of liblocator_hip.so behind `python -m locator_amd.pca` (locator_amd/csrc/grm_kernels.hip): the genetic
 * relationship matrix G = Z Z' of all sample pairs over all sites on the fp32 matrix pipe, and the site loadings Z' U of kept
 * eigenvectors.  The spelling rules of locator_hip.h hold (one declaration per `;`, comments only as this one), and
 * locator_amd/_abi.py derives the ctypes binding from this file with the same reader (EXTENSIONS["pca"], and the LOC_PCA_*
 * constants).  As in locator_hip.h: device pointers unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments
 * with loc_last_error set and nothing launched. */
#ifndef LOCATOR_HIP_PCA_H
#define LOCATOR_HIP_PCA_H
#include "locator_hip.h"

#define LOC_PCA_TILE 128      /* rows per side of a tile pair: one workgroup computes a 128 x 128 block of G */
#define LOC_PCA_BLOCK 32      /* sites per block staged through LDS */
#define LOC_PCA_MAX_NPC 64    /* most components loc_pca_loadings takes */
#define LOC_PCA_SITES 256     /* sites per workgroup of loc_pca_loadings */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- G = Z Z' ----
 * c [n_rows][pitch] int8 as loc_ibs_pairs takes it: c[s][v] = allele-1 count of sample s at site v, 0 .. 127, or negative =
 * missing; columns K .. pitch - 1 are never interpreted.  pitch >= K, pitch a multiple of 16, c 16-byte aligned.  mean, scale
 * [K] float, 16-byte aligned.  z[s][v] = fl(fl((float)c[s][v] - mean[v]) * scale[v]), two correctly rounded fp32 operations,
 * or 0 where c[s][v] < 0 (mean imputation); rows past n_rows and sites past K contribute 0.  g [n_rows][n_rows] double:
 * g[i][j] = sum over v of z[i][v] z[j][v].  The sites are split over k_groups groups of workgroups, group q owning a contiguous
 * run of LOC_PCA_BLOCK-site blocks (0 = chosen by the launcher from n_rows, K and the number of compute units; groups past
 * the last block are not launched).  Within a group the sum is an fp32 fused multiply-add chain on v_mfma_f32_32x32x2_f32 (Z
 * itself is never written to memory: the operands are formed in registers on the way to LDS); every group writes its fp32
 * 128 x 128 tiles to its own slab of `work`, and a second kernel adds the slabs in group order in double, writes g[i][j] for
 * i <= j and copies it to g[j][i].  So g is exactly symmetric, the same arguments on the same device give the same bits, no
 * floating-point atomic is used and no byte of `work` is read before this launch has written it.  work / work_bytes: scratch
 * of at least loc_grm_work_bytes(n_rows, K, k_groups) bytes, 16-byte aligned; K must stay below 2^31 and n_rows below 2^20. */
int64_t loc_grm_work_bytes(int n_rows, int64_t K, int k_groups);
int loc_grm_pairs(const int8_t* c, int n_rows, int64_t K, int64_t pitch, const float* mean, const float* scale, int k_groups,
                  double* g, void* work, int64_t work_bytes, void* stream);

/* ---- loadings ----
 * c, pitch, mean, scale and z as above (mean and scale need no alignment here); u [n_rows][npc] float, 1 <= npc <=
 * LOC_PCA_MAX_NPC.  t [K][npc] float: t[v][p] = sum over s of z[s][v] u[s][p], an fp32 fused multiply-add chain over the rows
 * in ascending order: one pass over c, the same bits for the same arguments. */
int loc_pca_loadings(const int8_t* c, int n_rows, int64_t K, int64_t pitch, const float* mean, const float* scale,
                     const float* u, int npc, float* t, void* stream);

#ifdef __cplusplus
}
#endif
#endif
