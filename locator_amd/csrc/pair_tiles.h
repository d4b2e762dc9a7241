// The tile-pair skeleton of the two all-pairs kernels, ibs_pairs_kernel (ibs_kernels.hip, int8 matrix pipe) and
// grm_pairs_kernel (grm_kernels.hip, fp32 matrix pipe; grm_windows_kernel beside it puts a window of sites on grid.y where
// the site group is); arithmetic, LDS image, operand lanes and epilogue stay in their files.
// ld_band_kernel (ld_kernels.hip) takes the loader, the lanes and the band's pair map from here; its work split is its own.
// Work split.  The result [n_rows][n_rows] is symmetric, so only the tile pairs (I, J), J >= I, of PT_T = 128 rows a side are
// computed: grid.x = the pair index, row I of the upper triangle holding tiles - I pairs.  grid.y = the site groups, group g
// owning the contiguous run of blocks [g per, min(nblocks, (g + 1) per)) of the kernel's site-block width; a group that would
// own no block is not launched, so every workgroup has b0 < b1 (pt_site_groups).  A workgroup is PT_NT = 256 threads = 4 waves;
// wave w owns the 64 x 64 quadrant (w >> 1, w & 1) of the 128 x 128 result as 2 x 2 tiles (tm, tn) of 32 x 32.
// Loading.  Raw int8 counts travel 16 bytes = 16 sites at a time (pt_load_piece); a row past n_rows and a site past K read as
// 0xff = missing, so pad rows and pad columns are never interpreted.  Each kernel forms its operands from the raw bytes IN
// REGISTERS on the way to LDS, requests the next block's pieces before the MFMAs of the current one, and stages the rows of a
// diagonal pair (I == J) once, both sides reading the same image.
// Lanes.  For either 32 x 32 MFMA shape, lane l supplies row l & 31 of its operand tile at the sites of its half l >> 5 (each
// kernel says which); the result tile comes back as column = lane & 31, row = rowmap(reg, half) (common.h).
#pragma once
#include <stdint.h>
#include <algorithm>

constexpr int PT_T = 128;                         // rows per side of a tile pair
constexpr int PT_NT = 256;                        // threads of a workgroup: 4 waves

#ifdef __HIPCC__
#include "common.h"

// one 16-byte piece of raw counts: row `row` of c, sites k .. k + 15; 0xff (missing) for a row past n_rows or a site past K
__device__ __forceinline__ uint4 pt_load_piece(const int8_t* __restrict__ c, int64_t row, int n_rows, int64_t k, int64_t K,
                                               int64_t pitch) {
    uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (row < n_rows && k < K) {                  // pitch is a multiple of 16 and >= K: a piece that starts below K ends within the row
        v = *reinterpret_cast<const uint4*>(c + row * pitch + k);
        const int64_t rem = K - k;
        if (rem < 16) {
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = (int)rem - 4 * e;
                if (r <= 0) w[e] = ~0u;
                else if (r < 4) w[e] |= ~0u << (8 * r);
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    return v;
}

// tile pair index -> (I, J): row I of the upper triangle holds tiles - I pairs
__device__ __forceinline__ void pt_pair(int pair, int tiles, int& I, int& J) {
    I = 0;
    while (pair >= tiles - I) {
        pair -= tiles - I;
        ++I;
    }
    J = I + pair;
}

// tile pair index -> (I, J) of a band (ld_kernels.hip): every row tile I meets the `per_row` column tiles J = I .. I + per_row - 1
__device__ __forceinline__ void pt_band_pair(int64_t pair, int per_row, int64_t& I, int64_t& J) {
    I = pair / per_row;
    J = I + pair % per_row;
}

// operand rows within the 128 rows of a side, of wave w's tile tm = 0 / tn = 0 (+ 32 for tile 1), and the lane's half
__device__ __forceinline__ int pt_arow(int w, int lane) { return 64 * (w >> 1) + (lane & 31); }
__device__ __forceinline__ int pt_brow(int w, int lane) { return 64 * (w & 1) + (lane & 31); }
__device__ __forceinline__ int pt_half(int lane) { return lane >> 5; }
// Accumulator r of tile (tm, tn) belongs at row 64 (w >> 1) + 32 tm + rowmap(r, half), column 64 (w & 1) + 32 tn + (lane & 31).
// The epilogues spell these sums out: behind a function (for the 64-bit rows of ibs_kernels.hip, rowmap itself) the compiler
// folds them before it meets the unrolled constants and schedules the block loops differently.
#endif

// ---- host: launch geometry and the launchers' common refusals.  Plain C++, no HIP call.
void loc_set_error(const char* fmt, ...);         // api.hip

inline int64_t pt_tiles(int n_rows) { return ((int64_t)n_rows + PT_T - 1) / PT_T; }
inline int64_t pt_pairs(int64_t tiles) { return tiles * (tiles + 1) / 2; }
// column tiles a row tile of `tile` rows meets in a band of W following rows: its own .. the one holding its last row + W
inline int64_t pt_band_tiles(int tile, int W) { return ((int64_t)tile - 1 + W) / tile + 1; }

// The site groups of a launch over `nblocks` site blocks and `pairs` tile pairs: how many are launched and the blocks each
// owns (0 when there is no block or no pair).  k_groups = 0 chooses from the device: two workgroups fit a compute unit.  Few
// pairs get as many groups as fill those 2 `units` slots once, and no more (one workgroup past a full round costs a whole
// round); more pairs than slots about `rounds` rounds of shorter workgroups, so that the last, partly filled round is a small
// share.  A group keeps at least `min_blocks` blocks: its epilogue stays a small share of its work (the callers say why their
// numbers are what they are).  Groups past the last block are not launched; grid.y holds 65535 at most.
struct pt_groups { int64_t groups, per; };
inline pt_groups pt_site_groups(int64_t nblocks, int64_t pairs, int k_groups, int units, int rounds, int min_blocks) {
    pt_groups s = {0, 0};
    if (nblocks <= 0 || pairs <= 0) return s;
    int64_t want = k_groups;
    if (want == 0) {
        const int64_t slots = 2 * (int64_t)units;
        want = pairs <= slots ? slots / pairs : (rounds * slots + pairs - 1) / pairs;
        want = std::max<int64_t>(1, std::min<int64_t>(want, nblocks / min_blocks));
    }
    want = std::min<int64_t>(std::min<int64_t>(want, nblocks), 65535);
    s.per = (nblocks + want - 1) / want;
    s.groups = (nblocks + s.per - 1) / s.per;
    return s;
}

// false, with loc_set_error naming `who`, for a negative size or a pitch below K
inline bool pt_sizes_ok(const char* who, int n_rows, int64_t K, int64_t pitch, int k_groups, int64_t work_bytes) {
    if (n_rows >= 0 && K >= 0 && pitch >= K && k_groups >= 0 && work_bytes >= 0) return true;
    loc_set_error("%s: n_rows=%d K=%lld pitch=%lld k_groups=%d work_bytes=%lld (none may be negative, pitch >= K)", who, n_rows,
                  (long long)K, (long long)pitch, k_groups, (long long)work_bytes);
    return false;
}
// ... and for rows that pt_load_piece could not read 16 bytes at a time
inline bool pt_rows_aligned(const char* who, const void* c, int64_t pitch) {
    if (pitch % 16 == 0 && (uintptr_t)c % 16 == 0) return true;
    loc_set_error("%s: pitch=%lld and c must be multiples of 16 bytes (rows are read 16 bytes at a time)", who, (long long)pitch);
    return false;
}
// ... and for scratch that is missing, misaligned or smaller than the `need` bytes that the entry point `sizer` asks for
inline bool pt_work_ok(const char* who, const char* sizer, const void* work, int64_t work_bytes, int64_t need) {
    if (need <= 0 || (work && work_bytes >= need && (uintptr_t)work % 16 == 0)) return true;
    loc_set_error("%s: work of %lld bytes at %p: needs %lld bytes, 16-byte aligned (%s)", who, (long long)work_bytes, work,
                  (long long)need, sizer);
    return false;
}
