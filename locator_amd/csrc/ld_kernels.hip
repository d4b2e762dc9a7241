// Banded linkage disequilibrium of the ld command (locator_amd/ld.py) on the int8 matrix pipe: for every site the six pair sums,
// r^2 and the over-threshold bit against the sites that follow it inside a window.  The definitions are in
// include/locator_hip_ld.h; the NumPy forms (ld.sums_host, ld.r2_host, ld.over_host) are what tests/test_gpu_ld.py holds the
// kernel to: sums element for element, r^2 bit for bit, the mask word for word.
//
// ld_band_kernel is a sibling of ibs_pairs_kernel (ibs_kernels.hip) with the roles swapped: the rows of the product are SITES,
// the reduction runs over SAMPLES.  From the tile-pair skeleton of pair_tiles.h it keeps the loading (pt_load_piece: raw 16-byte
// pieces, 0xff = missing for a site past K and a sample past n_samples), operands formed in registers on the way to LDS, the
// next block requested before the MFMAs of the current one, the LDS image and the operand lanes.  Its own:
// Work split: a band, not a triangle.  Tiles are LD_T = 64 sites a side; row tile I meets the column tiles J = I .. the one
// holding site 64 I + 63 + W (pt_band_pair), grid.x = tiles x tiles per row.  The reduction is not split: the samples are the
// short dimension and the band supplies the workgroups, so the sums need no atomics and no zeroing.
// Arithmetic: the planes m = [c >= 0], a = t1 + t2, a2 = t1 + 3 t2 = a a (bytes 0, 1, 4), and per 32-sample step and 32 x 32 tile
// the six products (m,m) (a,m) (m,a) (a,a) (a2,m) (m,a2) on v_mfma_i32_32x32x32_i8 into six i32 accumulators: exact.
// Wave shape: 256 threads = 4 waves, wave w owns ONE 32 x 32 tile, the quadrant (w >> 1, w & 1) of the 64 x 64 pair: six
// accumulators are 96 registers (the skeleton's 2 x 2 tiles a wave would need 384).  A wave whose quadrant holds no pair with
// 1 <= j - i <= W (below the diagonal, past the band, past K) skips its MFMAs; it still meets the barriers.
// Blocks are LD_B = 128 samples: two 16-byte pieces per thread and side in flight while a wave issues the 24 MFMAs of a block.
// LDS: [side][plane][row][128 B] = 48 KB, the eight 16-byte pieces of a row XOR-placed by (row >> 1) & 7: the 16 lanes of a
// ds_read_b128 group (rows r .. r + 15, one piece each; a row is 32 banks) then cover all 64 banks once.
// Epilogue: a lane holds all six sums of its 16 elements (column j = lane & 31, row i = rowmap(r, half)): it forms r^2 in float64
// (contraction off: two products, one division), writes sums and r^2 where asked, and the 32 lanes of a half, which hold 32
// consecutive slots of one row, ballot their bits; one lane of the half ORs the at most two words into the mask the launcher
// zeroed.  Every slot (i, l), l < W, lies in exactly one tile pair of the band, sites past K included: those pairs run no block
// and write the fill (sums 0, r^2 NaN), so the launch defines every element without a fill pass.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_ld.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

typedef int32_t ld_i32x16 __attribute__((ext_vector_type(16)));
typedef int32_t ld_i32x4 __attribute__((ext_vector_type(4)));

constexpr int LD_T = LOC_LD_TILE;
constexpr int LD_B = LOC_LD_BLOCK;
constexpr int LD_NT = PT_NT;
constexpr int LD_PLANE = LD_T * LD_B;             // bytes of one plane of one side
constexpr int LD_CHUNKS = LD_B / 16;              // 16-byte pieces of a row of a block
constexpr int LD_PIECES = LD_T * LD_CHUNKS / LD_NT;   // pieces per thread, side and block: 2
static_assert(LD_T == 64 && LD_B == 128 && LD_PIECES == 2, "2 x 2 waves of one tile; the XOR placement below is written for 128-byte rows");

enum { LD_M = 0, LD_A = 1, LD_A2 = 2, LD_PLANES = 3 };

// four raw counts -> the three plane words (the bit operations of ib_planes; a2 = t1 + 3 t2)
__device__ __forceinline__ void ld_planes(uint32_t w, uint32_t& m, uint32_t& a, uint32_t& a2) {
    m = (~w >> 7) & 0x01010101u;
    const uint32_t v = w & (m * 0xffu) & 0x03030303u;
    const uint32_t t2 = (v >> 1) & 0x01010101u;
    const uint32_t t1 = (v | (v >> 1)) & 0x01010101u;
    a = t1 + t2;
    a2 = t1 + 3u * t2;
}

__device__ __forceinline__ void ld_store_piece(uint8_t* side, int row, int chunk, uint4 raw) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t p[LD_PLANES][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ld_planes(w[e], p[LD_M][e], p[LD_A][e], p[LD_A2][e]);
    const int off = row * LD_B + ((chunk ^ ((row >> 1) & 7)) << 4);
#pragma unroll
    for (int q = 0; q < LD_PLANES; ++q)
        *reinterpret_cast<uint4*>(side + q * LD_PLANE + off) = make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
}

__device__ __forceinline__ ld_i32x4 ld_frag(const uint8_t* side, int plane, int row, int chunk) {
    return *reinterpret_cast<const ld_i32x4*>(side + plane * LD_PLANE + row * LD_B + ((chunk ^ ((row >> 1) & 7)) << 4));
}

__global__ __launch_bounds__(LD_NT, 2) void ld_band_kernel(const int8_t* __restrict__ ct, int64_t K, int n_samples, int64_t pitch,
                                                        int W, int per_row, const int32_t* __restrict__ reach, double thr,
                                                        uint32_t* __restrict__ over, int32_t* __restrict__ sums,
                                                        double* __restrict__ r2) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * LD_PLANES * LD_PLANE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t I, J;
    pt_band_pair((int64_t)blockIdx.x, per_row, I, J);
    const bool diag = I == J;
    const int64_t row_i0 = I * LD_T, row_j0 = J * LD_T;            // row_i0 < K: the launcher starts tiles x per_row pairs
    // a pair whose column tile lies past the last site runs no block: it only writes the fill of its slots
    const int nblocks = row_j0 < K ? (n_samples + LD_B - 1) / LD_B : 0;

    uint8_t* const side_i = lds;
    uint8_t* const side_j = diag ? lds : lds + LD_PLANES * LD_PLANE;
    const int n_rows = (int)K;                                     // K < 2^31 (launcher)

    uint4 raw_i[LD_PIECES], raw_j[LD_PIECES];
    auto request = [&](int b) {
#pragma unroll
        for (int e = 0; e < LD_PIECES; ++e) {
            const int q = t + LD_NT * e, row = q / LD_CHUNKS, chunk = q % LD_CHUNKS;
            const int64_t k = (int64_t)b * LD_B + 16 * chunk;
            raw_i[e] = pt_load_piece(ct, row_i0 + row, n_rows, k, n_samples, pitch);
            if (!diag) raw_j[e] = pt_load_piece(ct, row_j0 + row, n_rows, k, n_samples, pitch);
        }
    };

    ld_i32x16 acc[6];
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0;

    const int wi = 32 * (w >> 1), wj = 32 * (w & 1);               // the wave's quadrant
    const int arow = wi + (lane & 31), brow = wj + (lane & 31), half = pt_half(lane);
    // j - i over the quadrant runs from lo to hi; it holds a pair of the band iff hi >= 1, lo <= W and its first rows exist
    const int64_t gap_lo = (row_j0 + wj) - (row_i0 + wi + 31), gap_hi = (row_j0 + wj + 31) - (row_i0 + wi);
    const bool live = gap_hi >= 1 && gap_lo <= W && row_j0 + wj < K && row_i0 + wi < K;

    if (nblocks > 0) request(0);
    for (int b = 0; b < nblocks; ++b) {
#pragma unroll
        for (int e = 0; e < LD_PIECES; ++e) {
            const int q = t + LD_NT * e, row = q / LD_CHUNKS, chunk = q % LD_CHUNKS;
            ld_store_piece(side_i, row, chunk, raw_i[e]);
            if (!diag) ld_store_piece(side_j, row, chunk, raw_j[e]);
        }
        __syncthreads();
        if (b + 1 < nblocks) request(b + 1);
        if (live) {
#pragma unroll
            for (int ks = 0; ks < LD_B / 32; ++ks) {
                const int chunk = 2 * ks + half;
                const ld_i32x4 am = ld_frag(side_i, LD_M, arow, chunk), aa = ld_frag(side_i, LD_A, arow, chunk),
                               aq = ld_frag(side_i, LD_A2, arow, chunk);
                const ld_i32x4 bm = ld_frag(side_j, LD_M, brow, chunk), ba = ld_frag(side_j, LD_A, brow, chunk),
                               bq = ld_frag(side_j, LD_A2, brow, chunk);
                acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(am, bm, acc[0], 0, 0, 0);      // n
                acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, bm, acc[1], 0, 0, 0);      // sa
                acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(am, ba, acc[2], 0, 0, 0);      // sb
                acc[3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, ba, acc[3], 0, 0, 0);      // sab
                acc[4] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq, bm, acc[4], 0, 0, 0);      // saa
                acc[5] = __builtin_amdgcn_mfma_i32_32x32x32_i8(am, bq, acc[5], 0, 0, 0);      // sbb
            }
        }
        __syncthreads();                          // the block is consumed: the next one may overwrite it
    }

    const int words = (W + 31) / 32;
    const int64_t j = row_j0 + wj + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        // (r & 3) + ... is rowmap(r, half) of common.h, spelled out: see the note on the epilogues in pair_tiles.h
        const int64_t i = row_i0 + wi + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int64_t l = j - i - 1;              // the slot of (i, j) in row i
        const bool slot = i < K && l >= 0 && l < W;
        int64_t rc = 0;
        if (i < K) {
            rc = reach ? (int64_t)reach[i] : (int64_t)W;
            rc = max((int64_t)0, min(rc, min((int64_t)W, K - 1 - i)));
        }
        const bool in = slot && l < rc;
        double v = NAN;
        if (in) {
            const int64_t n = acc[0][r], sa = acc[1][r], sb = acc[2][r], sab = acc[3][r], saa = acc[4][r], sbb = acc[5][r];
            const int64_t cov = n * sab - sa * sb, va = n * saa - sa * sa, vb = n * sbb - sb * sb;   // exact: n < 2^20
            if (n >= 2 && va > 0 && vb > 0) {
                const double c = (double)cov, num = c * c, den = (double)va * (double)vb;
                v = num / den;
            }
        }
        if (slot) {
            const int64_t at = i * W + l;
            if (sums) {
#pragma unroll
                for (int q = 0; q < 6; ++q) sums[at * 6 + q] = in ? acc[q][r] : 0;
            }
            if (r2) r2[at] = v;
        }
        // the 32 lanes of a half hold the slots l0 .. l0 + 31 of row i, l0 = the slot of the half's first lane (possibly < 0)
        const unsigned long long votes = __ballot(in && v > thr);
        uint64_t mine = half ? votes >> 32 : votes & 0xffffffffull;
        if ((lane & 31) == 0 && mine != 0) {      // a set bit means i < K and 0 <= l < reach(i) <= W for that lane
            int64_t l0 = l;
            if (l0 < 0) {
                mine >>= (int)min((int64_t)63, -l0);
                l0 = 0;
            }
            mine <<= (int)(l0 & 31);
            uint32_t* const word = over + i * words + (l0 >> 5);
            if ((uint32_t)mine) atomicOr(word, (uint32_t)mine);
            if (mine >> 32) atomicOr(word + 1, (uint32_t)(mine >> 32));
        }
    }
}

extern "C" int loc_ld_band(const int8_t* ct, int64_t K, int n_samples, int64_t pitch, int W, const int32_t* reach, double thr,
                           uint32_t* over, int32_t* sums, double* r2, void* stream) {
    if (K < 0 || n_samples < 0 || pitch < n_samples || W < 1 || W > LOC_LD_MAX_WINDOW || n_samples >= (1 << 20) || !std::isfinite(thr)) {
        loc_set_error("loc_ld_band: K=%lld n_samples=%d pitch=%lld W=%d thr=%g (sizes may not be negative, pitch >= n_samples, "
                      "W 1 .. %d, n_samples < 2^20, thr finite)", (long long)K, n_samples, (long long)pitch, W, thr, LOC_LD_MAX_WINDOW);
        return -1;
    }
    if (!ct || !over) {
        loc_set_error("loc_ld_band: null buffer (ct and over are mandatory)");
        return -1;
    }
    if (!pt_rows_aligned("loc_ld_band", ct, pitch)) return -1;
    const int64_t tiles = (K + LD_T - 1) / LD_T, per_row = pt_band_tiles(LD_T, W), pairs = tiles * per_row;
    if (K > 0x7fffffff || pairs > 0x7fffffff) {
        loc_set_error("loc_ld_band: K=%lld sites with W=%d exceed one launch", (long long)K, W);
        return -1;
    }
    if (K == 0) return 0;
    const hipError_t e = hipMemsetAsync(over, 0, (size_t)K * (size_t)((W + 31) / 32) * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        loc_set_error("loc_ld_band: zeroing the mask: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(ld_band_kernel, dim3((unsigned)pairs), dim3(LD_NT), 0, (hipStream_t)stream, ct, K, n_samples, pitch, W,
                       (int)per_row, reach, thr, over, sums, r2);
    LOC_CHECK_LAUNCH();
    return 0;
}
