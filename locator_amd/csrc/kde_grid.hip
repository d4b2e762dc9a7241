// Density grids of the plot command (locator_amd/plot.py): a haversine Gaussian kernel density of each panel's replicate
// predictions, evaluated at every point of that panel's latitude x longitude grid.  One launch covers every panel.
//
// Work split: the panels' grids are laid end to end in z (z_off), and each workgroup takes one tile of KG_TILE
// consecutive grid points of that flat range, one grid point per thread.  Tiles are the same size whatever the panel,
// so large and small grids share the launch evenly.  A tile that straddles panels visits each of them in turn.
//
// Per pair the haversine term needs sin(dlat/2) and sin(dlon/2).  Both come from half-angle sines and cosines
// (sin(a - b) = sin a cos b - cos a sin b): the grid point's are computed once per thread, the points' once per LDS stage.
// That identity loses nothing that matters here: its absolute error is a few ulp of 1, so the exponent d^2 / (2h^2) moves
// by about 1e-13 at the distances where a term is not negligible, far below the 1e-9 relative tolerance of the tests.
//
// Each grid point sums its panel's points in index order (no skipping), so a value does not depend on the tile, the
// launch or the other panels.  Points are staged KG_STAGE at a time; a panel of any size streams through in order.
#include "common.h"

#include <cmath>
#include <vector>

constexpr int KG_TILE = 256;       // grid points per workgroup (one per thread)
constexpr int KG_STAGE = 1024;     // points per LDS stage: 5 doubles each = 40 KB

__global__ __launch_bounds__(KG_TILE) void kde_grid_kernel(const double* __restrict__ pts, const int64_t* __restrict__ pt_off,
                                                           const double* __restrict__ lat_axis, const int64_t* __restrict__ lat_off,
                                                           const double* __restrict__ lon_axis, const int64_t* __restrict__ lon_off,
                                                           int n_panels, double inv_2h2, double norm_2pih2,
                                                           double* __restrict__ z, const int64_t* __restrict__ z_off) {
    __shared__ double s_slat[KG_STAGE], s_clat[KG_STAGE], s_cos[KG_STAGE], s_slon[KG_STAGE], s_clon[KG_STAGE];
    const int t = threadIdx.x;
    const int64_t z0 = z_off[0], z_end = z_off[n_panels];
    const int64_t g0 = z0 + (int64_t)blockIdx.x * KG_TILE, g1 = min(g0 + (int64_t)KG_TILE, z_end);
    const int64_t g = g0 + t;
    // first panel whose grid holds g0: the largest s with z_off[s] <= g0 (empty grids skipped by the <= search)
    int lo = 0, hi = n_panels - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (z_off[mid] <= g0) lo = mid; else hi = mid - 1;
    }
    for (int s = lo; s < n_panels && z_off[s] < g1; ++s) {
        const int64_t zs = z_off[s], ze = z_off[s + 1];
        if (ze <= g0) continue;                       // an empty grid at this offset
        const bool mine = g >= zs && g < ze;
        const int64_t nx = lon_off[s + 1] - lon_off[s];
        const int64_t p0 = pt_off[s], n = pt_off[s + 1] - p0;
        double sla = 0.0, cla = 0.0, cg = 0.0, slo = 0.0, clo = 0.0;
        if (mine) {
            const int64_t k = g - zs, iy = k / nx, ix = k - iy * nx;
            const double lat = lat_axis[lat_off[s] + iy], lon = lon_axis[lon_off[s] + ix];
            sincos(0.5 * lat, &sla, &cla);
            sincos(0.5 * lon, &slo, &clo);
            cg = cos(lat);
        }
        double acc = 0.0;
        int bad = 0;
        for (int64_t c0 = 0; c0 < n; c0 += KG_STAGE) {
            const int cnt = (int)min((int64_t)KG_STAGE, n - c0);
            __syncthreads();                          // the previous stage (or panel) is consumed
            for (int i = t; i < cnt; i += KG_TILE) {
                const double plat = pts[2 * (p0 + c0 + i)], plon = pts[2 * (p0 + c0 + i) + 1];
                bad |= !(isfinite(plat) && isfinite(plon));
                double a, b;
                sincos(0.5 * plat, &a, &b);
                s_slat[i] = a; s_clat[i] = b;
                sincos(0.5 * plon, &a, &b);
                s_slon[i] = a; s_clon[i] = b;
                s_cos[i] = cos(plat);
            }
            __syncthreads();
            if (mine) {
                for (int i = 0; i < cnt; ++i) {
                    const double dla = sla * s_clat[i] - cla * s_slat[i];     // sin((lat_g - lat_p) / 2)
                    const double dlo = slo * s_clon[i] - clo * s_slon[i];     // sin((lon_g - lon_p) / 2)
                    const double hav = fmin(fma(cg * s_cos[i], dlo * dlo, dla * dla), 1.0);
                    const double d = 2.0 * asin(sqrt(hav));
                    acc += exp(-(d * d) * inv_2h2);
                }
            }
        }
        bad = __syncthreads_or(bad);
        if (mine) z[g] = (n == 0 || bad) ? NAN : acc / ((double)n * norm_2pih2);
    }
}

extern "C" int loc_kde_grid_batch(const double* pts, const int64_t* pt_off, const double* lat_axis, const int64_t* lat_off,
                                  const double* lon_axis, const int64_t* lon_off, int n_panels, double bandwidth, double* z,
                                  const int64_t* z_off, void* stream) {
    if (n_panels < 0 || !(bandwidth > 0.0) || !std::isfinite(bandwidth)) {
        loc_set_error("loc_kde_grid_batch: n_panels=%d bandwidth=%g (needs n_panels >= 0 and a finite bandwidth > 0)",
                      n_panels, bandwidth);
        return -1;
    }
    if (n_panels == 0) return 0;
    if (!pts || !pt_off || !lat_axis || !lat_off || !lon_axis || !lon_off || !z || !z_off) {
        loc_set_error("loc_kde_grid_batch: null buffer");
        return -1;
    }
    // The sizes live in the offset arrays: read them back to check every panel before anything is launched.
    const size_t nb = (size_t)(n_panels + 1) * sizeof(int64_t);
    std::vector<int64_t> po(n_panels + 1), ya(n_panels + 1), xa(n_panels + 1), zo(n_panels + 1);
    const int64_t* src[4] = {pt_off, lat_off, lon_off, z_off};
    int64_t* dst[4] = {po.data(), ya.data(), xa.data(), zo.data()};
    for (int k = 0; k < 4; ++k) {
        hipError_t e = hipMemcpyAsync(dst[k], src[k], nb, hipMemcpyDefault, (hipStream_t)stream);
        if (e != hipSuccess) {
            loc_set_error("loc_kde_grid_batch: reading the offsets: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) {
        loc_set_error("loc_kde_grid_batch: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (po[0] < 0 || ya[0] < 0 || xa[0] < 0 || zo[0] < 0) {
        loc_set_error("loc_kde_grid_batch: negative first offset");
        return -1;
    }
    for (int s = 0; s < n_panels; ++s) {
        const int64_t n = po[s + 1] - po[s], ny = ya[s + 1] - ya[s], nx = xa[s + 1] - xa[s], nz = zo[s + 1] - zo[s];
        if (n < 0 || ny < 0 || nx < 0 || nz < 0 || (ny > 0 && nx > INT64_MAX / ny) || nz != ny * nx) {
            loc_set_error("loc_kde_grid_batch: panel %d has %lld points, a %lld x %lld grid and %lld z values "
                          "(offsets must not decrease and z must hold ny * nx values)",
                          s, (long long)n, (long long)ny, (long long)nx, (long long)nz);
            return -1;
        }
    }
    const int64_t tiles = (zo[n_panels] - zo[0] + KG_TILE - 1) / KG_TILE;
    if (tiles == 0) return 0;
    if (tiles > 0x7fffffff) {
        loc_set_error("loc_kde_grid_batch: %lld grid points exceed one launch", (long long)(zo[n_panels] - zo[0]));
        return -1;
    }
    hipLaunchKernelGGL(kde_grid_kernel, dim3((unsigned)tiles), dim3(KG_TILE), 0, (hipStream_t)stream, pts, pt_off,
                       lat_axis, lat_off, lon_axis, lon_off, n_panels, 1.0 / (2.0 * bandwidth * bandwidth),
                       2.0 * M_PI * bandwidth * bandwidth, z, z_off);
    LOC_CHECK_LAUNCH();
    return 0;
}
