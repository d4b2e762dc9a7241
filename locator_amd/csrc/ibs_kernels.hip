// Pairwise identity-by-state statistics of the neighbors command (locator_amd/neighbors.py) on the int8 matrix pipe, and each
// row's nearest candidates.  The definitions are in include/locator_hip_neighbors.h; the NumPy forms (neighbors.pairs_host,
// neighbors.knn_host) are what tests/test_gpu_neighbors.py holds both kernels to, element for element.
//
// Arithmetic.  For allele counts a, b in {0, 1, 2}: |a - b| = a + b - 2 min(a, b) and min(a, b) = [a>=1][b>=1] + [a>=2][b>=2].
// With the byte planes m = [c >= 0], t1 = [c >= 1], t2 = [c >= 2], a = t1 + t2 (all zero where the call is missing):
//     n = M M'          d = A M' + M A' - 2 (T1 T1' + T2 T2')
// five int8 products per 32-site step and 32 x 32 tile on v_mfma_i32_32x32x32_i8, accumulated in i32: exact.
//
// ibs_pairs_kernel is the tile-pair skeleton of pair_tiles.h (work split, loading, staging, lanes) with blocks of
// LOC_IBS_BLOCK = 64 sites and, for n and for d, 128 accumulator registers a thread.  Its own:
// Operands: a thread loads two 16-byte pieces of raw counts per side and block, and eight bit operations per 4 sites turn
// them into the four planes (a pre-pass would write and re-read 4 N K bytes of plane images for every launch; here the raw
// bytes are read once per tile pair and the vector-ALU work, about 150 operations per thread and block, hides under the 40
// MFMAs a wave issues per block).  The -2 of the T products is applied to the A-side fragments after the LDS read (bytes 0 / 1
// times 0xfe = 0 / -2), so both sides of a tile pair share one LDS image format.
// LDS: [side][plane][row][64 B], the four 16-byte pieces of a row XOR-placed by (row >> 2) & 3: the 16 lanes of a
// ds_read_b128 group (rows r .. r + 15, one piece each) then cover all 64 banks once.
// Operand lanes: lane l holds 16 consecutive sites of row l & 31, the same 16 for the A and the B fragment of a step (half h
// the sites 32 ks + 16 h .. + 15), so the sum over sites is complete whatever order the pipe assigns to the 32 sites of a step.
// Epilogue: the tile and, off the diagonal, its mirror; plain stores with one group, integer atomics into zeroed outputs
// otherwise (any order of integer additions gives the same sums).
//
// ibs_knn_kernel: one wave per row; kmax rounds, each the minimum of (D, j) above the previous round's pick.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_neighbors.h"

#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

typedef int32_t ib_i32x16 __attribute__((ext_vector_type(16)));
typedef int32_t ib_i32x4 __attribute__((ext_vector_type(4)));

constexpr int IB_T = LOC_IBS_TILE;
constexpr int IB_B = LOC_IBS_BLOCK;
constexpr int IB_NT = PT_NT;
constexpr int IB_PLANE = IB_T * IB_B;             // bytes of one plane of one side
constexpr int IB_PIECES = IB_T * IB_B / 16 / IB_NT;   // 16-byte pieces per thread, side and block: 2
static_assert(IB_T == PT_T && IB_B == 64 && IB_PIECES == 2, "the wave / quadrant split below is written for 128 x 64");

enum { IB_M = 0, IB_A = 1, IB_T1 = 2, IB_T2 = 3 };

// four raw counts -> the four plane words
__device__ __forceinline__ void ib_planes(uint32_t w, uint32_t& m, uint32_t& a, uint32_t& t1, uint32_t& t2) {
    m = (~w >> 7) & 0x01010101u;
    const uint32_t v = w & (m * 0xffu) & 0x03030303u;
    t2 = (v >> 1) & 0x01010101u;
    t1 = (v | (v >> 1)) & 0x01010101u;
    a = t1 + t2;
}

__device__ __forceinline__ void ib_store_piece(uint8_t* side, int row, int chunk, uint4 raw) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t p[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ib_planes(w[e], p[IB_M][e], p[IB_A][e], p[IB_T1][e], p[IB_T2][e]);
    const int off = row * IB_B + ((chunk ^ ((row >> 2) & 3)) << 4);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<uint4*>(side + q * IB_PLANE + off) = make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
}

__device__ __forceinline__ ib_i32x4 ib_frag(const uint8_t* side, int plane, int row, int chunk) {
    return *reinterpret_cast<const ib_i32x4*>(side + plane * IB_PLANE + row * IB_B + ((chunk ^ ((row >> 2) & 3)) << 4));
}

template <bool ATOMIC>
__device__ __forceinline__ void ib_put(int32_t* __restrict__ out, int64_t at, int32_t v) {
    if (ATOMIC) atomicAdd(out + at, v);
    else out[at] = v;
}

template <bool ATOMIC>
__global__ __launch_bounds__(IB_NT) void ibs_pairs_kernel(const int8_t* __restrict__ c, int n_rows, int64_t K, int64_t pitch,
                                                          int tiles, int64_t blocks_per_group, int32_t* __restrict__ d,
                                                          int32_t* __restrict__ n) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 4 * IB_PLANE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int I, J;
    pt_pair((int)blockIdx.x, tiles, I, J);
    const bool diag = I == J;
    const int64_t nblocks = (K + IB_B - 1) / IB_B;
    const int64_t b0 = (int64_t)blockIdx.y * blocks_per_group;
    const int64_t b1 = min(nblocks, b0 + blocks_per_group);      // the launcher starts no group past the last block: b0 < b1

    uint8_t* const side_i = lds;
    uint8_t* const side_j = diag ? lds : lds + 4 * IB_PLANE;
    const int64_t row_i0 = (int64_t)I * IB_T, row_j0 = (int64_t)J * IB_T;

    uint4 raw_i[IB_PIECES], raw_j[IB_PIECES];
    auto request = [&](int64_t b) {
#pragma unroll
        for (int e = 0; e < IB_PIECES; ++e) {
            const int q = t + IB_NT * e, row = q >> 2, chunk = q & 3;
            const int64_t k = b * IB_B + 16 * chunk;
            raw_i[e] = pt_load_piece(c, row_i0 + row, n_rows, k, K, pitch);
            if (!diag) raw_j[e] = pt_load_piece(c, row_j0 + row, n_rows, k, K, pitch);
        }
    };

    ib_i32x16 acc_n[2][2], acc_d[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc_n[tm][tn][r] = 0;
                acc_d[tm][tn][r] = 0;
            }

    const int arow = pt_arow(w, lane), brow = pt_brow(w, lane), half = pt_half(lane);
    request(b0);
    for (int64_t b = b0; b < b1; ++b) {
#pragma unroll
        for (int e = 0; e < IB_PIECES; ++e) {
            const int q = t + IB_NT * e, row = q >> 2, chunk = q & 3;
            ib_store_piece(side_i, row, chunk, raw_i[e]);
            if (!diag) ib_store_piece(side_j, row, chunk, raw_j[e]);
        }
        __syncthreads();
        if (b + 1 < b1) request(b + 1);
#pragma unroll
        for (int ks = 0; ks < IB_B / 32; ++ks) {
            const int chunk = 2 * ks + half;
            ib_i32x4 am[2], aa[2], at1[2], at2[2], bm[2], ba[2], bt1[2], bt2[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                am[tt] = ib_frag(side_i, IB_M, arow + 32 * tt, chunk);
                aa[tt] = ib_frag(side_i, IB_A, arow + 32 * tt, chunk);
                at1[tt] = ib_frag(side_i, IB_T1, arow + 32 * tt, chunk) * (int32_t)0xfe;   // bytes 0 / 1 -> 0 / -2
                at2[tt] = ib_frag(side_i, IB_T2, arow + 32 * tt, chunk) * (int32_t)0xfe;
                bm[tt] = ib_frag(side_j, IB_M, brow + 32 * tt, chunk);
                ba[tt] = ib_frag(side_j, IB_A, brow + 32 * tt, chunk);
                bt1[tt] = ib_frag(side_j, IB_T1, brow + 32 * tt, chunk);
                bt2[tt] = ib_frag(side_j, IB_T2, brow + 32 * tt, chunk);
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    acc_n[tm][tn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(am[tm], bm[tn], acc_n[tm][tn], 0, 0, 0);
                    ib_i32x16 x = acc_d[tm][tn];
                    x = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa[tm], bm[tn], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_i32_32x32x32_i8(am[tm], ba[tn], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_i32_32x32x32_i8(at1[tm], bt1[tn], x, 0, 0, 0);
                    x = __builtin_amdgcn_mfma_i32_32x32x32_i8(at2[tm], bt2[tn], x, 0, 0, 0);
                    acc_d[tm][tn] = x;
                }
        }
        __syncthreads();                          // the block is consumed: the next one may overwrite it
    }

#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int64_t j = row_j0 + 64 * (w & 1) + 32 * tn + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // (r & 3) + ... is rowmap(r, half) of common.h, spelled out: see the note on the epilogues in pair_tiles.h
                const int64_t i = row_i0 + 64 * (w >> 1) + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (i < n_rows && j < n_rows) {
                    ib_put<ATOMIC>(n, i * n_rows + j, acc_n[tm][tn][r]);
                    ib_put<ATOMIC>(d, i * n_rows + j, acc_d[tm][tn][r]);
                    if (!diag) {
                        ib_put<ATOMIC>(n, j * n_rows + i, acc_n[tm][tn][r]);
                        ib_put<ATOMIC>(d, j * n_rows + i, acc_d[tm][tn][r]);
                    }
                }
            }
        }
}

__global__ __launch_bounds__(64) void ibs_knn_kernel(const int32_t* __restrict__ d, const int32_t* __restrict__ n, int n_rows,
                                                     int P, const uint8_t* __restrict__ candidate, int kmax,
                                                     int32_t* __restrict__ nbr, double* __restrict__ nbr_dist) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int32_t* drow = d + (int64_t)i * n_rows;
    const int32_t* nrow = n + (int64_t)i * n_rows;
    double prev_d = -1.0;                         // every D is >= 0: the first round takes any candidate
    int prev_j = -1;
    int r = 0;
    for (; r < kmax; ++r) {
        double best_d = INFINITY;
        int best_j = INT_MAX;
        for (int j = lane; j < n_rows; j += 64) {
            if (j == i || !candidate[j]) continue;
            const int32_t nn = nrow[j];
            if (nn <= 0) continue;                // D is NaN: no shared site
            const double D = (double)drow[j] / (double)(P * nn);
            if (!(D > prev_d || (D == prev_d && j > prev_j))) continue;     // picked in an earlier round
            if (D < best_d || (D == best_d && j < best_j)) {
                best_d = D;
                best_j = j;
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const double od = __shfl_xor(best_d, s);
            const int oj = __shfl_xor(best_j, s);
            if (od < best_d || (od == best_d && oj < best_j)) {
                best_d = od;
                best_j = oj;
            }
        }
        if (best_j == INT_MAX) break;             // uniform: no candidate is left
        if (lane == 0) {
            nbr[(int64_t)i * kmax + r] = best_j;
            nbr_dist[(int64_t)i * kmax + r] = best_d;
        }
        prev_d = best_d;
        prev_j = best_j;
    }
    for (int q = r + lane; q < kmax; q += 64) {
        nbr[(int64_t)i * kmax + q] = -1;
        nbr_dist[(int64_t)i * kmax + q] = NAN;
    }
}

extern "C" int64_t loc_ibs_work_bytes(int n_rows, int64_t K, int k_groups) {
    (void)n_rows;
    (void)K;
    (void)k_groups;
    return 0;                                     // the groups meet in the outputs themselves (integer atomics)
}

extern "C" int loc_ibs_pairs(const int8_t* c, int n_rows, int64_t K, int64_t pitch, int k_groups, int32_t* d, int32_t* n,
                             void* work, int64_t work_bytes, void* stream) {
    (void)work;
    if (!pt_sizes_ok("loc_ibs_pairs", n_rows, K, pitch, k_groups, work_bytes)) return -1;
    if (2 * K >= ((int64_t)1 << 31)) {
        loc_set_error("loc_ibs_pairs: K=%lld: a distance sum could leave int32 (2 K must stay below 2^31)", (long long)K);
        return -1;
    }
    if (n_rows == 0) return 0;
    if (!d || !n || (K > 0 && !c)) {
        loc_set_error("loc_ibs_pairs: null buffer");
        return -1;
    }
    if (K > 0 && !pt_rows_aligned("loc_ibs_pairs", c, pitch)) return -1;
    const int64_t tiles = pt_tiles(n_rows), pairs = pt_pairs(tiles);
    if (pairs > 0x7fffffff) {
        loc_set_error("loc_ibs_pairs: %d rows exceed one launch", n_rows);
        return -1;
    }
    // more pairs than workgroup slots: about four rounds of shorter workgroups, so that the last, partly filled round is a
    // small share.  A group keeps at least 8 blocks: its epilogue stays a small share
    const pt_groups split = pt_site_groups((K + IB_B - 1) / IB_B, pairs, k_groups, sr_compute_units(), 4, 8);
    const size_t out_bytes = (size_t)n_rows * (size_t)n_rows * sizeof(int32_t);
    if (split.groups != 1) {                      // no site: the sums are 0; several groups: they meet in zeroed outputs
        hipError_t e = hipMemsetAsync(d, 0, out_bytes, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(n, 0, out_bytes, (hipStream_t)stream);
        if (e != hipSuccess) {
            loc_set_error("loc_ibs_pairs: zeroing the outputs: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    if (split.groups == 0) return 0;
    const dim3 grid((unsigned)pairs, (unsigned)split.groups);
    if (split.groups > 1)
        hipLaunchKernelGGL(ibs_pairs_kernel<true>, grid, dim3(IB_NT), 0, (hipStream_t)stream, c, n_rows, K, pitch, (int)tiles,
                           split.per, d, n);
    else
        hipLaunchKernelGGL(ibs_pairs_kernel<false>, grid, dim3(IB_NT), 0, (hipStream_t)stream, c, n_rows, K, pitch, (int)tiles,
                           split.per, d, n);
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_ibs_knn(const int32_t* d, const int32_t* n, int n_rows, int P, const uint8_t* candidate, int kmax,
                           int32_t* nbr, double* nbr_dist, void* stream) {
    if (n_rows < 0 || (P != 1 && P != 2) || kmax < 1 || kmax > 64) {
        loc_set_error("loc_ibs_knn: n_rows=%d P=%d kmax=%d (n_rows >= 0, P 1 or 2, kmax 1..64)", n_rows, P, kmax);
        return -1;
    }
    if (n_rows == 0) return 0;
    if (!d || !n || !candidate || !nbr || !nbr_dist) {
        loc_set_error("loc_ibs_knn: null buffer");
        return -1;
    }
    hipLaunchKernelGGL(ibs_knn_kernel, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, d, n, n_rows, P, candidate, kmax,
                       nbr, nbr_dist);
    LOC_CHECK_LAUNCH();
    return 0;
}
