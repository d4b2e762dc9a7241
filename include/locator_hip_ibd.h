/* Entry points of liblocator_hip.so behind `python -m locator_amd.ibd` (locator_amd/csrc/ibd_kernels.hip): identity-by-descent
 * segments between phased haplotypes, found on bit planes by integer code alone.  The spelling rules of locator_hip.h hold (one
 * declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding from this file with the
 * same reader (EXTENSIONS["ibd"], and the LOC_IBD_* constants).  As in locator_hip.h: device pointers unless named h_*, `stream` a
 * hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing launched.  The NumPy definitions are
 * locator_amd/ibd.py: pack_host and segments_host; the device gives their answers bit for bit. */
#ifndef LOCATOR_HIP_IBD_H
#define LOCATOR_HIP_IBD_H
#include "locator_hip.h"

#define LOC_IBD_MAX_HAPS 32768    /* most haplotype columns H: a pair keeps O(1) state, the limit only bounds the grid */
#define LOC_IBD_MAX_GAP 8         /* largest gap_sites: discordant sites between two runs that may still be linked */
#define LOC_IBD_PACK_COLS 4       /* consecutive columns a thread of loc_ibd_pack packs: one dword of a site's row */
#define LOC_IBD_BLOCK 256         /* consecutive columns q a workgroup of the scan holds, one lane a pair (p, q) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the two bit planes of a haplotype matrix ----
 * h [K][pitch] int8, site-major: h[j][d] = allele of haplotype column d at site j, 0 or 1, or negative = missing; columns
 * H .. pitch - 1 are never interpreted.  pitch >= H, pitch a multiple of 16, h 16-byte aligned, 1 <= H <= LOC_IBD_MAX_HAPS,
 * 0 <= K < 2^31.  bits [2][W][wpitch] uint64, W = ceil(K / 64), wpitch >= H and a multiple of 8, bits 8-byte aligned: plane 0
 * has bit j % 64 of word [j / 64][d] set where h[j][d] > 0, plane 1 where h[j][d] >= 0.  The bits of sites >= K and the words
 * of the columns H .. wpitch - 1 are zero; every word of both planes is written.  K = 0 writes nothing. */
int loc_ibd_pack(const int8_t* h, int H, int64_t K, int64_t pitch, uint64_t* bits, int64_t wpitch, void* stream);

/* ---- segments of the rows p0 .. p0 + R - 1 against every column ----
 * bits, wpitch, H, K as loc_ibd_pack wrote them.  owner [H] int32 (the individual of a column), first_bits [W] uint64 (bit
 * j % 64 of word j / 64 set where site j is the first of a chromosome; site 0 counts as set either way; bits of sites >= K
 * zero), x [K] int64 (the coordinate of a site, non-decreasing inside a chromosome: not checked here).  0 <= p0, 0 <= R,
 * p0 + R <= H.  seed_sites >= 1, seed_len >= 0, 1 <= extend_sites <= seed_sites, 0 <= gap_sites <= LOC_IBD_MAX_GAP,
 * gap_len >= 0, min_len >= 0.  For p = p0 + i and every q: nothing where q <= p or owner[q] == owner[p]; else, with site j
 * agreeing where an allele is missing or the two are equal:
 *   a run [a, b] is a maximal interval of agreeing sites that holds no first site except as its a;
 *   consecutive runs [a1, b1], [a2, b2] are linked where both have extend_sites sites at least, 1 <= a2 - b1 - 1 <= gap_sites,
 *   no site of b1 + 1 .. a2 is a first site, and x[a2] - x[b1] <= gap_len;
 *   a maximal chain of linked runs from a to b is a segment where one of its runs has seed_sites sites at least and
 *   x-length >= seed_len, and x[b] - x[a] >= min_len.
 * count [R][H] int32 = the segments of the pair, length [R][H] int64 = the sum of their x[b] - x[a], longest [R][H] int64 =
 * the largest of them; zeros where there is nothing.  Every element of the three is written.  Integer code, one lane a
 * pair, no atomics: the answer does not depend on p0 / R, on what the outputs held or on the pad words.
 * R = 0 launches nothing; K = 0 sets the outputs to zeros. */
int loc_ibd_scan(const uint64_t* bits, int64_t wpitch, int H, int64_t K, const int32_t* owner, const uint64_t* first_bits,
                 const int64_t* x, int p0, int R, int64_t seed_sites, int64_t seed_len, int64_t extend_sites, int64_t gap_sites,
                 int64_t gap_len, int64_t min_len, int32_t* count, int64_t* length, int64_t* longest, void* stream);

/* ---- the segments themselves ----
 * The same scan by the same device function; segment number n (ascending in a) of the pair (p0 + i, q) is stored as
 * seg_a[offsets[i][q] + n], seg_b[...] (int32 sites a and b) where that index is in 0 .. capacity - 1, and is dropped
 * otherwise: no store goes outside the capacity elements whatever offsets holds.  offsets [R][H] int64: the driver's exclusive
 * prefix sum of loc_ibd_scan's count in row-major order.  capacity >= 0.  R = 0, K = 0 or capacity = 0 launch nothing. */
int loc_ibd_fill(const uint64_t* bits, int64_t wpitch, int H, int64_t K, const int32_t* owner, const uint64_t* first_bits,
                 const int64_t* x, int p0, int R, int64_t seed_sites, int64_t seed_len, int64_t extend_sites, int64_t gap_sites,
                 int64_t gap_len, int64_t min_len, const int64_t* offsets, int64_t capacity, int32_t* seg_a, int32_t* seg_b,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
