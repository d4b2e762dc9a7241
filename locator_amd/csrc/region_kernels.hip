// Map regions of the regions command (locator_amd/regions.py): which region's outline holds each predicted point, and the
// nearest outline vertex of a point that no region holds.  The definitions are in include/locator_hip_regions.h; the NumPy
// forms (regions.assign_host, regions.nearest_host) are what tests/test_gpu_regions.py holds both kernels to, bit for bit.
//
// Arithmetic: every float64 operation is rounded once, in the order the header gives - contraction is off for this file, and
// the division is the correctly rounded one (no fast-math flag anywhere in the build).
//
// loc_region_assign, work split: one point per thread, LOC_REGION_TILE points per workgroup.  The workgroup reduces the
// bounding box of its finite points, then walks the rings in order.  A ring whose box misses the tile's box is passed over
// on the scalar side: its box, offsets and region are scalar loads, the test is a scalar branch, no vertex is read and no
// barrier is met.  A surviving ring streams through LDS, LOC_REGION_STAGE vertices at a time plus the one vertex that ends
// the stage's last edge (the next stage's first vertex, or vertex 0 for the closing edge); every thread reads the same LDS
// address, a broadcast.  A thread whose own point lies outside the ring's box sits the ring out.  The parity of the current
// region is one register bit, flushed when ring_region changes (a region's rings are adjacent), so the lowest region that
// holds a point is the first flush that finds the bit set.  No atomics; a point's answer is a function of the point and the
// rings alone.
//
// loc_region_nearest: one point per thread, the vertices through LDS in stages, a running (minimum, index) in index order.
#include "common.h"

#include "../../include/locator_hip_regions.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

constexpr int RG_TILE = LOC_REGION_TILE;
constexpr int RG_STAGE = LOC_REGION_STAGE;
constexpr int RG_WAVES = RG_TILE / 64;

// a value that is the same in every lane of the workgroup, moved to scalar registers: what is branched on stays a scalar branch
__device__ __forceinline__ double rg_uniform(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(RG_TILE) void region_assign_kernel(const double* __restrict__ pts, int64_t n,
                                                                const double* __restrict__ verts,
                                                                const int64_t* __restrict__ ring_off,
                                                                const int32_t* __restrict__ ring_region,
                                                                const double* __restrict__ ring_bbox, int n_rings,
                                                                int32_t* __restrict__ region, int32_t* __restrict__ n_inside) {
    __shared__ double s_x[RG_STAGE + 1], s_y[RG_STAGE + 1];
    __shared__ double s_box[4][RG_WAVES];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * RG_TILE + t;
    double px = NAN, py = NAN;
    if (i < n) {
        px = pts[2 * i];
        py = pts[2 * i + 1];
    }
    const bool finite = isfinite(px) && isfinite(py);
    // the tile's box over its finite points; a tile without one keeps (+inf, -inf) and every ring misses it
    double bx0 = finite ? px : INFINITY, bx1 = finite ? px : -INFINITY;
    double by0 = finite ? py : INFINITY, by1 = finite ? py : -INFINITY;
    for (int d = 32; d >= 1; d >>= 1) {
        bx0 = fmin(bx0, __shfl_xor(bx0, d));
        bx1 = fmax(bx1, __shfl_xor(bx1, d));
        by0 = fmin(by0, __shfl_xor(by0, d));
        by1 = fmax(by1, __shfl_xor(by1, d));
    }
    if ((t & 63) == 0) {
        s_box[0][t >> 6] = bx0;
        s_box[1][t >> 6] = bx1;
        s_box[2][t >> 6] = by0;
        s_box[3][t >> 6] = by1;
    }
    __syncthreads();
    bx0 = s_box[0][0]; bx1 = s_box[1][0]; by0 = s_box[2][0]; by1 = s_box[3][0];
    for (int w = 1; w < RG_WAVES; ++w) {
        bx0 = fmin(bx0, s_box[0][w]);
        bx1 = fmax(bx1, s_box[1][w]);
        by0 = fmin(by0, s_box[2][w]);
        by1 = fmax(by1, s_box[3][w]);
    }
    const double tx0 = rg_uniform(bx0), tx1 = rg_uniform(bx1), ty0 = rg_uniform(by0), ty1 = rg_uniform(by1);

    int cur = -1, first = -1, count = 0;
    bool odd = false;
    for (int r = 0; r < n_rings; ++r) {
        const int reg = ring_region[r];
        if (reg != cur) {                             // uniform: the previous region is complete
            if (odd) {
                if (first < 0) first = cur;
                ++count;
            }
            odd = false;
            cur = reg;
        }
        const double rx0 = ring_bbox[4 * (int64_t)r], rx1 = ring_bbox[4 * (int64_t)r + 1];
        const double ry0 = ring_bbox[4 * (int64_t)r + 2], ry1 = ring_bbox[4 * (int64_t)r + 3];
        if (rx1 < tx0 || rx0 > tx1 || ry1 < ty0 || ry0 > ty1) continue;      // uniform: the ring's box misses the tile's
        const int64_t o0 = ring_off[r], m = ring_off[r + 1] - o0;
        if (m < 3) continue;                          // uniform
        const bool mine = finite && !(px < rx0 || px > rx1 || py < ry0 || py > ry1);
        for (int64_t c0 = 0; c0 < m; c0 += RG_STAGE) {
            const int cnt = (int)min((int64_t)RG_STAGE, m - c0);
            __syncthreads();                          // the previous stage (or ring) is consumed
            for (int k = t; k <= cnt; k += RG_TILE) { // cnt vertices and the end of the last edge
                const int64_t v = c0 + k < m ? c0 + k : 0;
                s_x[k] = verts[2 * (o0 + v)];
                s_y[k] = verts[2 * (o0 + v) + 1];
            }
            __syncthreads();
            if (mine) {
                double xi = s_x[0], yi = s_y[0];
                for (int k = 1; k <= cnt; ++k) {
                    const double xj = s_x[k], yj = s_y[k];
                    if ((yi > py) != (yj > py)) {
                        const double tt = (xj - xi) * (py - yi) / (yj - yi) + xi;
                        odd ^= px < tt;
                    }
                    xi = xj;
                    yi = yj;
                }
            }
        }
    }
    if (odd) {
        if (first < 0) first = cur;
        ++count;
    }
    if (i < n) {
        region[i] = finite ? first : -2;
        n_inside[i] = finite ? count : 0;
    }
}

__global__ __launch_bounds__(RG_TILE) void region_nearest_kernel(const double* __restrict__ pts3, int64_t m,
                                                                 const double* __restrict__ verts3, int64_t nv,
                                                                 int64_t* __restrict__ nearest, double* __restrict__ dist2) {
    __shared__ double s_v[3 * RG_STAGE];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * RG_TILE + t;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (i < m) {
        px = pts3[3 * i];
        py = pts3[3 * i + 1];
        pz = pts3[3 * i + 2];
    }
    double best = INFINITY;
    int64_t arg = -1;
    for (int64_t c0 = 0; c0 < nv; c0 += RG_STAGE) {
        const int cnt = (int)min((int64_t)RG_STAGE, nv - c0);
        __syncthreads();                              // the previous stage is consumed
        for (int k = t; k < 3 * cnt; k += RG_TILE) s_v[k] = verts3[3 * c0 + k];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const double dx = s_v[3 * k] - px, dy = s_v[3 * k + 1] - py, dz = s_v[3 * k + 2] - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) {
                best = d2;
                arg = c0 + k;
            }
        }
    }
    if (i < m) {
        nearest[i] = arg;
        dist2[i] = best;
    }
}

extern "C" int loc_region_assign(const double* pts, int64_t n, const double* verts, const int64_t* ring_off,
                                 const int32_t* ring_region, const double* ring_bbox, int n_rings, int n_regions,
                                 int32_t* region, int32_t* n_inside, void* stream) {
    if (n < 0 || n_rings < 0 || n_regions < 0) {
        loc_set_error("loc_region_assign: n=%lld n_rings=%d n_regions=%d (none may be negative)", (long long)n, n_rings,
                      n_regions);
        return -1;
    }
    if (n == 0) return 0;
    if (!pts || !region || !n_inside || (n_rings > 0 && (!verts || !ring_off || !ring_region || !ring_bbox))) {
        loc_set_error("loc_region_assign: null buffer");
        return -1;
    }
    const int64_t tiles = (n + RG_TILE - 1) / RG_TILE;
    if (tiles > 0x7fffffff) {
        loc_set_error("loc_region_assign: %lld points exceed one launch", (long long)n);
        return -1;
    }
    if (n_rings > 0) {
        // The ring sizes and regions live in device arrays: read them back to check every ring before anything is launched.
        std::vector<int64_t> off((size_t)n_rings + 1);
        std::vector<int32_t> reg((size_t)n_rings);
        hipError_t e = hipMemcpyAsync(off.data(), ring_off, off.size() * sizeof(int64_t), hipMemcpyDefault, (hipStream_t)stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(reg.data(), ring_region, reg.size() * sizeof(int32_t), hipMemcpyDefault, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) {
            loc_set_error("loc_region_assign: reading the ring offsets: %s", hipGetErrorString(e));
            return (int)e;
        }
        if (off[0] < 0) {
            loc_set_error("loc_region_assign: negative first offset");
            return -1;
        }
        for (int r = 0; r < n_rings; ++r) {
            if (off[r + 1] < off[r]) {
                loc_set_error("loc_region_assign: ring_off decreases at ring %d (%lld -> %lld)", r, (long long)off[r],
                              (long long)off[r + 1]);
                return -1;
            }
            if (reg[r] < 0 || reg[r] >= n_regions) {
                loc_set_error("loc_region_assign: ring %d names region %d, outside 0..%d", r, reg[r], n_regions - 1);
                return -1;
            }
            if (r > 0 && reg[r] < reg[r - 1]) {
                loc_set_error("loc_region_assign: ring_region decreases at ring %d (%d -> %d): a region's rings must be adjacent",
                              r, reg[r - 1], reg[r]);
                return -1;
            }
        }
    }
    hipLaunchKernelGGL(region_assign_kernel, dim3((unsigned)tiles), dim3(RG_TILE), 0, (hipStream_t)stream, pts, n, verts,
                       ring_off, ring_region, ring_bbox, n_rings, region, n_inside);
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_region_nearest(const double* pts3, int64_t m, const double* verts3, int64_t nv, int64_t* nearest,
                                  double* dist2, void* stream) {
    if (m < 0 || nv < 0) {
        loc_set_error("loc_region_nearest: m=%lld nv=%lld (neither may be negative)", (long long)m, (long long)nv);
        return -1;
    }
    if (m == 0) return 0;
    if (nv == 0) {
        loc_set_error("loc_region_nearest: %lld points and no vertex", (long long)m);
        return -1;
    }
    if (!pts3 || !verts3 || !nearest || !dist2) {
        loc_set_error("loc_region_nearest: null buffer");
        return -1;
    }
    const int64_t tiles = (m + RG_TILE - 1) / RG_TILE;
    if (tiles > 0x7fffffff) {
        loc_set_error("loc_region_nearest: %lld points exceed one launch", (long long)m);
        return -1;
    }
    hipLaunchKernelGGL(region_nearest_kernel, dim3((unsigned)tiles), dim3(RG_TILE), 0, (hipStream_t)stream, pts3, m, verts3,
                       nv, nearest, dist2);
    LOC_CHECK_LAUNCH();
    return 0;
}
