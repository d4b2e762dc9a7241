/* Entry point of liblocator_hip.so behind `python -m locator_amd.localpca` (locator_amd/csrc/grm_kernels.hip): one relationship
 * matrix G_w = Z_w Z_w' per window of sites, all windows in one launch on the fp32 matrix pipe.  The spelling rules of
 * locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (EXTENSIONS["localpca"], and the LOC_LOCALPCA_* constants).  As in locator_hip.h: device
 * pointers unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing
 * launched.  The NumPy definition is locator_amd/localpca.py: windows_host. */
#ifndef LOCATOR_HIP_LOCALPCA_H
#define LOCATOR_HIP_LOCALPCA_H
#include "locator_hip_pca.h"

#define LOC_LOCALPCA_MAX_WINDOWS 65535   /* most windows of one launch: the window is grid.y */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- G_w = Z[:, v0:v1] Z[:, v0:v1]' for every window ----
 * c, n_rows, K, pitch, mean, scale and z exactly as loc_grm_pairs (locator_hip_pca.h) takes them: n_rows < 2^20, K < 2^31,
 * pitch >= K and a multiple of 16, c, mean and scale 16-byte aligned.  win [n_windows][2] int64, 16-byte aligned: window w is
 * the half-open run of sites win[w][0] <= v < win[w][1], 0 <= v0 <= v1 <= K; windows may overlap, repeat or be empty (the
 * kernel clamps v0 to [0, K] and v1 to [v0, K], but callers pass nothing else).  1 <= n_windows <= LOC_LOCALPCA_MAX_WINDOWS.
 * g [n_windows][n_rows][n_rows] float, 4-byte aligned, offsets into it are 64-bit: g[w][i][j] = sum over v0 <= v < v1 of
 * z[i][v] z[j][v].  One workgroup owns a 128 x 128 tile pair (i <= j by tiles) of one window over the window's WHOLE site run:
 * the sum is a single fp32 fused multiply-add chain on v_mfma_f32_32x32x2_f32 in site order, over the absolute
 * LOC_PCA_BLOCK-site blocks v0 / 32 .. (v1 - 1) / 32, a site of those blocks outside [v0, v1) entering with mean = scale = 0,
 * i.e. as an exact +0.  So g[w] has the bits of loc_grm_pairs(k_groups = 1) run with scale zeroed outside the window, rounded
 * to float (that rounding is exact: the sum was fp32).  The workgroup writes g[w][i][j] for i <= j and the same register to
 * g[w][j][i]: g[w] is exactly symmetric.  Every element of g is written by the launch (zeros for an empty window), no scratch
 * and no atomic is used, and the same arguments give the same bits.  n_rows = 0 launches nothing. */
int loc_grm_windows(const int8_t* c, int n_rows, int64_t K, int64_t pitch, const float* mean, const float* scale,
                    const int64_t* win, int n_windows, float* g, void* stream);

#ifdef __cplusplus
}
#endif
#endif
