/* Entry points of liblocator_hip.so behind `python -m locator_amd.regions` (locator_amd/csrc/region_kernels.hip): which map
 * region holds each predicted point, and the nearest outline vertex of a point that no region holds.  The spelling rules of
 * locator_hip.h hold (one declaration per `;`, comments only as this one), and locator_amd/_abi.py derives the ctypes binding
 * from this file with the same reader (EXTENSIONS["region"], and the LOC_REGION_* constants).  As in locator_hip.h: device
 * pointers unless named h_*, `stream` a hipStream_t, 0 = success, -1 = bad arguments with loc_last_error set and nothing
 * launched. */
#ifndef LOCATOR_HIP_REGIONS_H
#define LOCATOR_HIP_REGIONS_H
#include "locator_hip.h"

#define LOC_REGION_TILE 256    /* points per workgroup, one per thread */
#define LOC_REGION_STAGE 2048  /* vertices per LDS stage, of both kernels */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- point in region (even-odd crossing number, float64, planar) ----
 * pts [n][2] = (x, y); verts [nv][2]; ring r holds vertices ring_off[r] .. ring_off[r + 1] (ring_off [n_rings + 1], must not
 * decrease) and belongs to region ring_region[r] in 0 .. n_regions - 1 (ring_region [n_rings], must not decrease: a region's
 * rings are adjacent).  A ring is closed by the edge from its last vertex to its first; a ring of fewer than 3 vertices adds
 * nothing.  For every edge (xi, yi) -> (xj, yj) of a ring with (yi > py) != (yj > py), t = (xj - xi) * (py - yi) / (yj - yi) + xi,
 * each operation rounded once to float64 in that order (no fused multiply-add), and px < t toggles the ring's region.  A
 * point is in a region when the toggles over all of that region's rings are odd.
 * region[i] = the lowest region that holds point i, -1 when none does, -2 when a coordinate of the point is not finite;
 * n_inside[i] = how many regions hold it.
 * ring_bbox [n_rings][4] = xmin, xmax, ymin, ymax is what the kernel culls by: ring r is not visited for a point with
 * px < xmin, px > xmax, py < ymin or py > ymax.  The caller owns the claim that no such point can change parity: the y bounds
 * may be the exact extremes (equality is kept), the x bounds must leave room for the rounding of t
 * (locator_amd.regions.ring_boxes pads them).  An answer does not depend on the tile, the launch or the order of the points. */
int loc_region_assign(const double* pts, int64_t n, const double* verts, const int64_t* ring_off, const int32_t* ring_region,
                      const double* ring_bbox, int n_rings, int n_regions, int32_t* region, int32_t* n_inside, void* stream);

/* ---- nearest vertex ----
 * pts3 [m][3], verts3 [nv][3]: nearest[i] = the first vertex v, in index order, with the smallest
 * d2 = ((dx * dx + dy * dy) + dz * dz), d = verts3[v] - pts3[i], each operation rounded once to float64 (no fused
 * multiply-add; strict <, so the lowest index wins a tie), and dist2[i] = that d2.  A point for which no d2 is below
 * +infinity (a NaN coordinate) gets nearest -1 and dist2 +infinity.  m == 0 returns 0; nv == 0 with m > 0 is -1. */
int loc_region_nearest(const double* pts3, int64_t m, const double* verts3, int64_t nv, int64_t* nearest, double* dist2,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
