// The genetic relationship matrix of the pca command (locator_amd/pca.py) on the fp32 matrix pipe, and the site loadings of
// kept eigenvectors.  The definitions are in include/locator_hip_pca.h; the NumPy forms (pca.grm_host, pca.loadings_host) are
// what tests/test_gpu_pca.py holds both kernels to: element for element where every product and partial sum is an fp32
// integer, and within the derived fp32 bound otherwise.
//
// Arithmetic.  z[s][v] = fl(fl((float)c[s][v] - mean[v]) * scale[v]), 0 for a missing call; G = Z Z'.  Every site carries its
// own non-integer weight, so unlike the IBS product (ibs_kernels.hip) this one cannot run on the int8 pipe: it runs on
// v_mfma_f32_32x32x2_f32, whose result is an fp32 fused multiply-add chain in site order.
//
// grm_pairs_kernel is the tile-pair skeleton of pair_tiles.h (work split, loading, staging, lanes) with blocks of
// LOC_PCA_BLOCK = 32 sites and 64 accumulator registers a thread.  Its own:
// Operands: Z is never written to memory.  A thread loads one 16-byte piece of raw counts per side and block, and the 16
// means and scales of its sites, and forms the 16 operand values in registers (four operations a value, beside the 64 MFMAs
// a wave issues per block); a pre-pass would write and re-read 4 N K bytes where this launch reads N K per tile row.
// LDS: [side][row][32 floats], the eight 16-byte pieces of a row XOR-placed by (row >> 1) & 7.  A [row][site] image read one
// dword per lane would put the 32 rows of an operand on one bank; here a lane reads 16 bytes = four consecutive sites of its
// row with one ds_read_b128 and feeds four successive MFMAs from them, and the 16 lanes of a ds_read_b128 group (16 rows, one
// piece each: rows r and r + 1 share a 256-byte bank row, (row >> 1) & 7 takes eight values over the group) cover all 64
// banks once.
// Operand lanes: an MFMA takes two sites, lane l supplying row l & 31 at the site of its half l >> 5.  In the step over sites
// 8 s .. 8 s + 7 of a block, half h reads sites 8 s + 4 h .. + 3 and MFMA q of the step uses element q: the site pair
// (8 s + q, 8 s + 4 + q), the SAME pair for the A and the B fragment, so every site of the block enters every sum once.
// Epilogue: the group's fp32 tile goes to its own slab of `work`, all 128 x 128 of it.  grm_reduce_kernel then adds the
// slabs of an element in group order in double and writes g[i][j] (i <= j) and its copy g[j][i], inside a diagonal tile too:
// no floating-point atomics, the same bits on every launch, G exactly symmetric.
//
// grm_windows_kernel (the localpca command, include/locator_hip_localpca.h) is the same block loop with a window of sites on
// grid.y in place of the site group and an epilogue of its own: its text stands before it.
//
// pca_loadings_kernel: t[v][p] = sum_s z[s][v] u[s][p].  Memory-bound (one pass over c), so vector-ALU: a workgroup owns
// LOC_PCA_SITES = 256 sites, lane l four consecutive ones (one dword of c per row), wave w the components 16 w .. 16 w + 15,
// 64 accumulators a thread; u is staged through LDS 64 rows at a time, zero-padded to 64 columns, and read as broadcasts.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_pca.h"
#include "../../include/locator_hip_localpca.h"

#include <cstdint>

#pragma clang fp contract(off)

constexpr int GR_T = LOC_PCA_TILE;
constexpr int GR_B = LOC_PCA_BLOCK;
constexpr int GR_NT = PT_NT;
constexpr int GR_SIDE = GR_T * GR_B;              // floats of one side's image
static_assert(GR_T == PT_T && GR_B == 32 && GR_T * GR_B / 16 == GR_NT, "one 16-site piece per thread and side; 128 x 32");

// the operand value of one count
__device__ __forceinline__ float gr_z(int cv, float mean, float scale) {
    const float z = ((float)cv - mean) * scale;   // two roundings: contraction is off
    return cv < 0 ? 0.f : z;
}
__device__ __forceinline__ int gr_byte(uint32_t w, int e) { return (int)(w << (24 - 8 * e)) >> 24; }

// 16 floats of a per-site array from site k on, 0 past K (a is 16-byte aligned, k a multiple of 16)
__device__ __forceinline__ void gr_load_sites(const float* __restrict__ a, int64_t k, int64_t K, f32x4 (&v)[4]) {
    if (k + 16 <= K) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = *reinterpret_cast<const f32x4*>(a + k + 4 * e);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int x = 0; x < 4; ++x) v[e][x] = k + 4 * e + x < K ? a[k + 4 * e + x] : 0.f;
    }
}

__device__ __forceinline__ int gr_at(int row, int piece) { return row * GR_B + ((piece ^ ((row >> 1) & 7)) << 2); }

__device__ __forceinline__ void gr_store_piece(float* side, int row, int chunk, uint4 raw, const f32x4 (&mean)[4],
                                               const f32x4 (&scale)[4]) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f32x4 z;
#pragma unroll
        for (int x = 0; x < 4; ++x) z[x] = gr_z(gr_byte(w[e], x), mean[e][x], scale[e][x]);
        *reinterpret_cast<f32x4*>(side + gr_at(row, 4 * chunk + e)) = z;
    }
}

__global__ __launch_bounds__(GR_NT) void grm_pairs_kernel(const int8_t* __restrict__ c, int n_rows, int64_t K, int64_t pitch,
                                                          const float* __restrict__ mean, const float* __restrict__ scale,
                                                          int tiles, int64_t blocks_per_group, float* __restrict__ slabs) {
    __shared__ __attribute__((aligned(16))) float lds[2 * GR_SIDE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int I, J;
    pt_pair((int)blockIdx.x, tiles, I, J);
    const bool diag = I == J;
    const int64_t nblocks = (K + GR_B - 1) / GR_B;
    const int64_t b0 = (int64_t)blockIdx.y * blocks_per_group;
    const int64_t b1 = min(nblocks, b0 + blocks_per_group);      // the launcher starts no group past the last block: b0 < b1

    float* const side_i = lds;
    float* const side_j = diag ? lds : lds + GR_SIDE;
    const int64_t row_i0 = (int64_t)I * GR_T, row_j0 = (int64_t)J * GR_T;
    const int srow = t >> 1, schunk = t & 1;      // the piece this thread stages: row srow, sites 16 schunk .. + 15 of the block

    uint4 raw_i, raw_j = make_uint4(~0u, ~0u, ~0u, ~0u);
    f32x4 mv[4], sv[4];
    auto request = [&](int64_t b) {
        const int64_t k = b * GR_B + 16 * schunk;
        raw_i = pt_load_piece(c, row_i0 + srow, n_rows, k, K, pitch);
        if (!diag) raw_j = pt_load_piece(c, row_j0 + srow, n_rows, k, K, pitch);
        gr_load_sites(mean, k, K, mv);
        gr_load_sites(scale, k, K, sv);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int arow = pt_arow(w, lane), brow = pt_brow(w, lane), half = pt_half(lane);
    request(b0);
    for (int64_t b = b0; b < b1; ++b) {
        gr_store_piece(side_i, srow, schunk, raw_i, mv, sv);
        if (!diag) gr_store_piece(side_j, srow, schunk, raw_j, mv, sv);
        __syncthreads();
        if (b + 1 < b1) request(b + 1);
#pragma unroll
        for (int s = 0; s < GR_B / 8; ++s) {
            const int piece = 2 * s + half;
            f32x4 a[2], bb[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                a[tt] = *reinterpret_cast<const f32x4*>(side_i + gr_at(arow + 32 * tt, piece));
                bb[tt] = *reinterpret_cast<const f32x4*>(side_j + gr_at(brow + 32 * tt, piece));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = mfma32(a[tm][q], bb[tn][q], acc[tm][tn]);
        }
        __syncthreads();                          // the block is consumed: the next one may overwrite it
    }

    float* const slab = slabs + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (int64_t)(GR_T * GR_T);
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int jl = 64 * (w & 1) + 32 * tn + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int il = 64 * (w >> 1) + 32 * tm + rowmap(r, half);
                slab[il * GR_T + jl] = acc[tm][tn][r];
            }
        }
}

// grid.x = the tile pairs, grid.y * 256 threads = the 128 x 128 elements of a tile
__global__ __launch_bounds__(256) void grm_reduce_kernel(const float* __restrict__ slabs, int groups, int n_rows, int tiles,
                                                         double* __restrict__ g) {
    int I, J;
    pt_pair((int)blockIdx.x, tiles, I, J);
    const int e = (int)blockIdx.y * 256 + (int)threadIdx.x;
    const int64_t i = (int64_t)I * GR_T + (e >> 7), j = (int64_t)J * GR_T + (e & 127);
    if (i >= n_rows || j >= n_rows || i > j) return;
    double s = 0.0;
    for (int q = 0; q < groups; ++q)
        s += (double)slabs[((int64_t)q * gridDim.x + blockIdx.x) * (int64_t)(GR_T * GR_T) + e];
    g[i * n_rows + j] = s;
    g[j * n_rows + i] = s;
}

// mean or scale of 16 sites, 0 for a site outside the window: the window holds the sites lo <= e < hi of the 16
__device__ __forceinline__ void gw_mask_sites(f32x4 (&v)[4], int lo, int hi) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int x = 0; x < 4; ++x) v[e][x] = (4 * e + x >= lo && 4 * e + x < hi) ? v[e][x] : 0.f;
}

// grm_windows_kernel (include/locator_hip_localpca.h): grm_pairs_kernel's block loop with the window on grid.y in place of
// the site group.  The workgroup walks the absolute blocks v0 / 32 .. (v1 - 1) / 32 of its window, so every piece it reads is
// an aligned 16-byte piece wherever the window starts; in the first and the last block the sites outside [v0, v1) get
// mean = scale = 0 in registers: z = fl(fl((float)c - 0) * 0) = +0 for a call, 0 for a missing one.
// Epilogue: one workgroup holds the window's whole sum, so the tile goes straight to g[w] as fp32 - no slab, no reduce pass.
// An element with i <= j is stored from its register, lanes 0 .. 31 of a store covering 128 consecutive bytes of row i.  Its
// copy g[w][j][i] would leave the registers as 32 rows x 4 bytes per store, so each wave turns its 32 x 32 tiles through its
// own quarter of the operand LDS (free after the loop; rows of 33 floats: no bank is hit twice by a half wave) and stores the
// copy along row j, 128 consecutive bytes a half wave again.  -DGW_MIRROR_STRIDED (measurement builds only: `make variant`)
// stores the copy from the registers instead.  A diagonal tile pair takes the same path, i < j selecting the copy: no element
// is stored from two different registers.
constexpr int GW_TR = 33;                         // floats of a row of a wave's transposition image
static_assert(32 * GW_TR <= 2 * GR_SIDE / (GR_NT / 64), "a wave's 32 x 33 image fits its quarter of the operand LDS");

__global__ __launch_bounds__(GR_NT) void grm_windows_kernel(const int8_t* __restrict__ c, int n_rows, int64_t K, int64_t pitch,
                                                            const float* __restrict__ mean, const float* __restrict__ scale,
                                                            int tiles, const int64_t* __restrict__ win, float* __restrict__ g) {
    __shared__ __attribute__((aligned(16))) float lds[2 * GR_SIDE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int I, J;
    pt_pair((int)blockIdx.x, tiles, I, J);
    const bool diag = I == J;
    const int64_t v0 = min(max(win[2 * (int64_t)blockIdx.y], (int64_t)0), K);
    const int64_t v1 = min(max(win[2 * (int64_t)blockIdx.y + 1], v0), K);
    const int64_t b0 = v0 / GR_B;
    const int64_t b1 = v1 > v0 ? (v1 - 1) / GR_B + 1 : b0;       // an empty window walks no block

    float* const side_i = lds;
    float* const side_j = diag ? lds : lds + GR_SIDE;
    const int64_t row_i0 = (int64_t)I * GR_T, row_j0 = (int64_t)J * GR_T;
    const int srow = t >> 1, schunk = t & 1;

    uint4 raw_i = make_uint4(~0u, ~0u, ~0u, ~0u), raw_j = make_uint4(~0u, ~0u, ~0u, ~0u);
    f32x4 mv[4], sv[4];
    auto request = [&](int64_t b) {
        const int64_t k = b * GR_B + 16 * schunk;
        raw_i = pt_load_piece(c, row_i0 + srow, n_rows, k, K, pitch);
        if (!diag) raw_j = pt_load_piece(c, row_j0 + srow, n_rows, k, K, pitch);
        gr_load_sites(mean, k, K, mv);
        gr_load_sites(scale, k, K, sv);
        if (k < v0 || k + 16 > v1) {              // the window's first or last block only
            const int lo = (int)min(max(v0 - k, (int64_t)0), (int64_t)16), hi = (int)min(max(v1 - k, (int64_t)0), (int64_t)16);
            gw_mask_sites(mv, lo, hi);
            gw_mask_sites(sv, lo, hi);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int arow = pt_arow(w, lane), brow = pt_brow(w, lane), half = pt_half(lane);
    if (b0 < b1) request(b0);
    for (int64_t b = b0; b < b1; ++b) {
        gr_store_piece(side_i, srow, schunk, raw_i, mv, sv);
        if (!diag) gr_store_piece(side_j, srow, schunk, raw_j, mv, sv);
        __syncthreads();
        if (b + 1 < b1) request(b + 1);
#pragma unroll
        for (int s = 0; s < GR_B / 8; ++s) {
            const int piece = 2 * s + half;
            f32x4 a[2], bb[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                a[tt] = *reinterpret_cast<const f32x4*>(side_i + gr_at(arow + 32 * tt, piece));
                bb[tt] = *reinterpret_cast<const f32x4*>(side_j + gr_at(brow + 32 * tt, piece));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = mfma32(a[tm][q], bb[tn][q], acc[tm][tn]);
        }
        __syncthreads();                          // the block is consumed: the next one, or the epilogue, may overwrite it
    }

    float* const gw = g + (int64_t)blockIdx.y * n_rows * (int64_t)n_rows;
    float* const tr = lds + w * (2 * GR_SIDE / (GR_NT / 64));
    const int64_t ld = n_rows;                    // wave-uniform: the row offsets below are scalar
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int64_t i00 = row_i0 + 64 * (w >> 1) + 32 * tm, j00 = row_j0 + 64 * (w & 1) + 32 * tn;
            // element r of the tile: row i0 + rowmap(r, 0), column j
            const int64_t i0 = i00 + 4 * half, j = j00 + (lane & 31);
            const int64_t room = j < n_rows ? j - i0 : -1;                            // rows 0 .. room of this lane have i <= j
            float* const direct = gw + i0 * ld + j;
#ifdef GW_MIRROR_STRIDED
            float* const copy = gw + j * ld + i0;
#endif
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (rowmap(r, 0) <= room) direct[rowmap(r, 0) * ld] = acc[tm][tn][r];  // i <= j < n_rows
#ifdef GW_MIRROR_STRIDED
                if (rowmap(r, 0) < room) copy[rowmap(r, 0)] = acc[tm][tn][r];
#else
                tr[(lane & 31) * GW_TR + rowmap(r, half)] = acc[tm][tn][r];           // [column of the tile][row of the tile]
#endif
            }
#ifndef GW_MIRROR_STRIDED
            __syncthreads();
            // element rr of the turned tile: row j00 + half + 2 rr of g, column im
            const int64_t im = i00 + (lane & 31), jm0 = j00 + half;
            const int64_t rows = min((int64_t)n_rows, jm0 + 32) - jm0;                // rows jm0 + 2 rr below n_rows: 2 rr < rows
            const int64_t first = im - jm0;                                           // ... and past im: 2 rr > first
            float* const copy = gw + jm0 * ld + im;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float v = tr[(2 * rr + half) * GW_TR + (lane & 31)];
                if (2 * rr < rows && 2 * rr > first) copy[2 * rr * ld] = v;           // im < jm < n_rows
            }
            __syncthreads();                      // the image is read: the next tile may overwrite it
#endif
        }
}

constexpr int PL_NT = 256;
constexpr int PL_ROWS = 64;                       // rows of u per stage
constexpr int PL_PW = 16;                         // components per wave
static_assert(LOC_PCA_SITES == 4 * 64 && LOC_PCA_MAX_NPC == PL_PW * (PL_NT / 64), "4 sites a lane, 16 components a wave");

__global__ __launch_bounds__(PL_NT) void pca_loadings_kernel(const int8_t* __restrict__ c, int n_rows, int64_t K, int64_t pitch,
                                                             const float* __restrict__ mean, const float* __restrict__ scale,
                                                             const float* __restrict__ u, int npc, float* __restrict__ t) {
    __shared__ __attribute__((aligned(16))) float us[PL_ROWS][LOC_PCA_MAX_NPC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t k = (int64_t)blockIdx.x * LOC_PCA_SITES + 4 * lane;
    const bool live = k < K;                      // pitch is a multiple of 4 and >= K: a dword that starts below K ends within the row
    const bool active = PL_PW * w < npc;          // wave-uniform: this wave has components
    float mv[4], sv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mv[e] = k + e < K ? mean[k + e] : 0.f;
        sv[e] = k + e < K ? scale[k + e] : 0.f;   // a pad byte behind K times 0: never stored either
    }
    float acc[4][PL_PW];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int p = 0; p < PL_PW; ++p) acc[e][p] = 0.f;

    for (int i0 = 0; i0 < n_rows; i0 += PL_ROWS) {
        if (i0) __syncthreads();                  // the previous rows are consumed
#pragma unroll
        for (int x = 0; x < PL_ROWS * LOC_PCA_MAX_NPC / PL_NT; ++x) {
            const int idx = tid + PL_NT * x, r = idx >> 6, p = idx & 63;
            us[r][p] = (i0 + r < n_rows && p < npc) ? u[(int64_t)(i0 + r) * npc + p] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        const int nr = min(PL_ROWS, n_rows - i0);
#pragma unroll 4
        for (int r = 0; r < nr; ++r) {
            const uint32_t wd = live ? *reinterpret_cast<const uint32_t*>(c + (int64_t)(i0 + r) * pitch + k) : ~0u;
            float z[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) z[e] = gr_z(gr_byte(wd, e), mv[e], sv[e]);
#pragma unroll
            for (int p = 0; p < PL_PW; ++p) {
                const float uu = us[r][PL_PW * w + p];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e][p] = __builtin_fmaf(z[e], uu, acc[e][p]);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < K)
#pragma unroll
            for (int p = 0; p < PL_PW; ++p)
                if (PL_PW * w + p < npc) t[(k + e) * npc + PL_PW * w + p] = acc[e][p];
}

// the site groups of a launch (pair_tiles.h); none when there is no site or no row
static pt_groups gr_split(int n_rows, int64_t K, int k_groups) {
    // more pairs than workgroup slots: about eight rounds of shorter workgroups (measured at 528 pairs on 256 units: 4 groups
    // 15.4 ms, 8 groups 14.4 ms, 12 groups 14.2 ms for half as much scratch again).  A group keeps at least 16 blocks (512
    // sites): its 64 KiB slab - written once, read once - stays a small share of its work
    return pt_site_groups((K + GR_B - 1) / GR_B, pt_pairs(pt_tiles(n_rows)), k_groups, sr_compute_units(), 8, 16);
}

static bool gr_sizes_ok(const char* who, int n_rows, int64_t K, int k_groups) {
    if (n_rows < 0 || K < 0 || k_groups < 0 || n_rows >= (1 << 20) || K >= ((int64_t)1 << 31)) {
        loc_set_error("%s: n_rows=%d K=%lld k_groups=%d (none may be negative; n_rows must stay below 2^20 and K below 2^31)", who,
                      n_rows, (long long)K, k_groups);
        return false;
    }
    return true;
}

extern "C" int64_t loc_grm_work_bytes(int n_rows, int64_t K, int k_groups) {
    if (!gr_sizes_ok("loc_grm_work_bytes", n_rows, K, k_groups)) return -1;
    return gr_split(n_rows, K, k_groups).groups * pt_pairs(pt_tiles(n_rows)) * (int64_t)(GR_T * GR_T * sizeof(float));
}

extern "C" int loc_grm_pairs(const int8_t* c, int n_rows, int64_t K, int64_t pitch, const float* mean, const float* scale,
                             int k_groups, double* g, void* work, int64_t work_bytes, void* stream) {
    if (!gr_sizes_ok("loc_grm_pairs", n_rows, K, k_groups) || !pt_sizes_ok("loc_grm_pairs", n_rows, K, pitch, k_groups, work_bytes))
        return -1;
    if (n_rows == 0) return 0;
    if (!g || (K > 0 && (!c || !mean || !scale))) {
        loc_set_error("loc_grm_pairs: null buffer");
        return -1;
    }
    if (K > 0 && !pt_rows_aligned("loc_grm_pairs", c, pitch)) return -1;
    if ((uintptr_t)g % 8 != 0 || (K > 0 && ((uintptr_t)mean % 16 != 0 || (uintptr_t)scale % 16 != 0))) {
        loc_set_error("loc_grm_pairs: mean and scale must be multiples of 16 bytes (site constants are read 16 bytes at a time), "
                      "g of 8");
        return -1;
    }
    const pt_groups split = gr_split(n_rows, K, k_groups);
    const int64_t groups = split.groups, tiles = pt_tiles(n_rows), pairs = pt_pairs(tiles);
    const int64_t need = groups * pairs * (int64_t)(GR_T * GR_T * sizeof(float));
    if (!pt_work_ok("loc_grm_pairs", "loc_grm_work_bytes", work, work_bytes, need)) return -1;
    if (groups > 0) {
        hipLaunchKernelGGL(grm_pairs_kernel, dim3((unsigned)pairs, (unsigned)groups), dim3(GR_NT), 0, (hipStream_t)stream, c,
                           n_rows, K, pitch, mean, scale, (int)tiles, split.per, (float*)work);
        LOC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(grm_reduce_kernel, dim3((unsigned)pairs, GR_T * GR_T / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float*)work, (int)groups, n_rows, (int)tiles, g);     // no group: every sum is 0
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_grm_windows(const int8_t* c, int n_rows, int64_t K, int64_t pitch, const float* mean, const float* scale,
                               const int64_t* win, int n_windows, float* g, void* stream) {
    if (!gr_sizes_ok("loc_grm_windows", n_rows, K, 0) || !pt_sizes_ok("loc_grm_windows", n_rows, K, pitch, 0, 0)) return -1;
    if (n_windows < 1 || n_windows > LOC_LOCALPCA_MAX_WINDOWS) {
        loc_set_error("loc_grm_windows: n_windows=%d (1..%d: the caller batches above that)", n_windows, LOC_LOCALPCA_MAX_WINDOWS);
        return -1;
    }
    if (!g || !win || (K > 0 && (!c || !mean || !scale))) {
        loc_set_error("loc_grm_windows: null buffer");
        return -1;
    }
    if (K > 0 && !pt_rows_aligned("loc_grm_windows", c, pitch)) return -1;
    if ((uintptr_t)g % 4 != 0 || (uintptr_t)win % 16 != 0 || (K > 0 && ((uintptr_t)mean % 16 != 0 || (uintptr_t)scale % 16 != 0))) {
        loc_set_error("loc_grm_windows: mean, scale and win must be multiples of 16 bytes (site constants and window bounds are "
                      "read 16 bytes at a time), g of 4");
        return -1;
    }
    if (n_rows == 0) return 0;
    const int64_t tiles = pt_tiles(n_rows), pairs = pt_pairs(tiles);
    hipLaunchKernelGGL(grm_windows_kernel, dim3((unsigned)pairs, (unsigned)n_windows), dim3(GR_NT), 0, (hipStream_t)stream, c,
                       n_rows, K, pitch, mean, scale, (int)tiles, win, g);
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_pca_loadings(const int8_t* c, int n_rows, int64_t K, int64_t pitch, const float* mean, const float* scale,
                                const float* u, int npc, float* t, void* stream) {
    if (!gr_sizes_ok("loc_pca_loadings", n_rows, K, 0)) return -1;
    if (pitch < K || npc < 1 || npc > LOC_PCA_MAX_NPC) {
        loc_set_error("loc_pca_loadings: K=%lld pitch=%lld npc=%d (pitch >= K, npc 1..%d)", (long long)K, (long long)pitch, npc,
                      LOC_PCA_MAX_NPC);
        return -1;
    }
    if (K == 0) return 0;
    if (!t || !mean || !scale || (n_rows > 0 && (!c || !u))) {
        loc_set_error("loc_pca_loadings: null buffer");
        return -1;
    }
    if (pitch % 16 != 0 || (uintptr_t)c % 16 != 0 || (uintptr_t)mean % 4 != 0 || (uintptr_t)scale % 4 != 0 ||
        (uintptr_t)u % 4 != 0 || (uintptr_t)t % 4 != 0) {
        loc_set_error("loc_pca_loadings: pitch=%lld and c must be multiples of 16 bytes, the float arrays of 4", (long long)pitch);
        return -1;
    }
    const int64_t blocks = (K + LOC_PCA_SITES - 1) / LOC_PCA_SITES;
    hipLaunchKernelGGL(pca_loadings_kernel, dim3((unsigned)blocks), dim3(PL_NT), 0, (hipStream_t)stream, c, n_rows, K, pitch,
                       mean, scale, u, npc, t);
    LOC_CHECK_LAUNCH();
    return 0;
}
