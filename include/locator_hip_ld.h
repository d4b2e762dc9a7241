/* Entry point of liblocator_hip.so behind `python -m locator_amd.ld` and the --ld_prune option of the neighbors and pca commands
 * (locator_amd/csrc/ld_kernels.hip): the squared correlation r^2 of every site with the sites that follow it inside a window, on
 * the int8 matrix pipe.  The spelling rules of locator_hip.h hold (one declaration per `;`, comments only as this one), and
 * locator_amd/_abi.py derives the ctypes binding from this file with the same reader (EXTENSIONS["ld"], and the LOC_LD_*
 * constants).  As in locator_hip.h: device pointers unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments
 * with loc_last_error set and nothing launched. */
#ifndef LOCATOR_HIP_LD_H
#define LOCATOR_HIP_LD_H
#include "locator_hip.h"

#define LOC_LD_TILE 64          /* sites per side of a tile pair: one workgroup computes a 64 x 64 block of site pairs */
#define LOC_LD_BLOCK 128        /* samples per block staged through LDS */
#define LOC_LD_MAX_WINDOW 1024  /* largest window W, in sites */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- banded pair sums, r^2 and the over-threshold mask ----
 * ct [K][pitch] int8, site-major: ct[v][s] = allele-1 count of sample s at site v, 0 .. 2, or negative = missing; columns
 * n_samples .. pitch - 1 are never interpreted.  pitch >= n_samples, pitch a multiple of 16, ct 16-byte aligned, n_samples < 2^20,
 * K < 2^31.  A count of 3 .. 127 is outside the contract (the planes read its two low bits).
 * Site i is compared with the sites j = i + 1 .. i + reach(i), reach(i) = reach[i] (W where reach is null) clamped to
 * 0 .. min(W, K - 1 - i); 1 <= W <= LOC_LD_MAX_WINDOW.  Slot l = j - i - 1 of row i holds the pair (i, j).
 * Over the samples s where both ct[i][s] >= 0 and ct[j][s] >= 0, with a = the count of i and b = the count of j, six exact int32
 * sums:  n = their number, sa = sum a, sb = sum b, sab = sum a b, saa = sum a a, sbb = sum b b.  From the byte planes m = [c >= 0],
 * a = [c >= 1] + [c >= 2], a2 = [c >= 1] + 3 [c >= 2]:  n = M M', sa = A M', sb = M A', sab = A A', saa = A2 M', sbb = M A2', int8
 * products accumulated in int32; the reduction over samples is not split, so there is no atomic on a sum.
 * In float64:  cov = n sab - sa sb, va = n saa - sa sa, vb = n sbb - sb sb (exact integers below 2^53),
 * r2 = (cov * cov) / (va * vb), two correctly rounded products and one correctly rounded division; NaN where n < 2, va <= 0 or
 * vb <= 0.  The pair is `over` where r2 > thr (never where r2 is NaN); thr must be finite.
 * over [K][(W + 31) / 32] uint32 (mandatory): bit b of word w of row i is set iff l = 32 w + b < reach(i) and the pair is over.
 * sums [K][W][6] int32 in the order n, sa, sb, sab, saa, sbb, and r2 [K][W] double: each may be null.
 * The launch defines every element of every output it is given: slots l >= reach(i) hold bit 0, sums 0 and r2 NaN.  `over` is
 * zeroed on `stream` and the tile pairs OR their bits in, so the result does not depend on the launch.
 * K = 0 or n_samples = 0 is a valid launch (no pair; n = 0, r2 NaN). */
int loc_ld_band(const int8_t* ct, int64_t K, int n_samples, int64_t pitch, int W, const int32_t* reach, double thr,
                uint32_t* over, int32_t* sums, double* r2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
