// A kept model applied to a new genotype file (python -m locator_amd.predict): the query's calls -> the model's sample-major
// uint8 rows, one column per model SNP in the model's order.  The host has matched every model column k
// to a query variant col_variant[k] (or -1: absent) and to the allele col_allele[k] of that variant whose copies the column
// counts (1 normally, 0 when the query swaps REF and ALT, 2.. for a multi-allelic record; locator_amd/query.py).
//   X[r][k] = sum_p (gt[col_variant[k]][sample_order[r]][p] == col_allele[k])
// Missing alleles (negative) count nothing, as to_allele_counts does in training; an absent column is 0.  Laid out like
// snp_rows_kernel (filter_kernels.hip): a workgroup owns QT consecutive model columns, reads each gathered variant's N * P
// contiguous bytes with wide loads, counts into an LDS tile [column][sample], then writes every output row's run of the
// tile contiguously (lane = column).  Results: tests/test_gpu_query.py against the NumPy form in tests/test_query.py.
#include "common.h"
#include "../../include/locator_hip_query.h"

#define QT 64
#define QS 960
#define QPAD 4      /* row pitch QS + 4 bytes = 241 words (odd): the 64 lanes reading one sample of the tile hit distinct banks */
#define QU 8        /* wide loads in flight per thread */

template <int VB> struct QVec;
template <> struct QVec<16> { typedef uint4 T; };
template <> struct QVec<8> { typedef uint2 T; };
template <> struct QVec<4> { typedef uint32_t T; };

// VB > 0: every thread loads VB bytes = VB / P samples of one column at a time (the host picks VB so that every row and every
// chunk start is VB-aligned).  VB == 0: any ploidy, one sample per thread and step.
template <int VB, int P>
__global__ __launch_bounds__(256) void query_rows_kernel(const int8_t* __restrict__ gt, int64_t n_variants, int n_samples,
                                                         int ploidy, const int32_t* __restrict__ col_variant,
                                                         const int8_t* __restrict__ col_allele, int K,
                                                         const int32_t* __restrict__ sample_order, int n_out,
                                                         uint8_t* __restrict__ X, int64_t x_pitch) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[QT][QS + QPAD];
    __shared__ int32_t var[QT];
    __shared__ int32_t alle[QT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t k0 = (int64_t)blockIdx.x * QT;
    const int nk = K - k0 < QT ? (int)(K - k0) : QT;
    if (t < QT) {
        int v = -1, a = -1;
        if (t < nk) {
            v = col_variant[k0 + t];
            a = col_allele[k0 + t];
            if (v < 0 || v >= n_variants || a < 0) v = -1;      // absent (or out of range: never read)
        }
        var[t] = v;
        alle[t] = a;
    }
    const int64_t row_bytes = (int64_t)n_samples * ploidy;
    for (int s0 = 0; s0 < n_samples; s0 += QS) {
        const int ns = n_samples - s0 < QS ? n_samples - s0 : QS;
        __syncthreads();                            // var / alle written; the previous chunk's tile fully read
        if constexpr (VB > 0) {
            typedef typename QVec<VB>::T V;
            constexpr int SPT = VB / P;             // samples per load
            const int wpc = ns / SPT;               // loads per column in this chunk (ns * P is a multiple of VB)
            const int total = nk * wpc;
            for (int i0 = t; i0 < total; i0 += 256 * QU) {
                union { V v; uint8_t b[VB]; } buf[QU];
#pragma unroll
                for (int u = 0; u < QU; ++u) {
                    const int i = i0 + u * 256;
                    buf[u].v = V{};
                    if (i < total) {
                        const int j = i / wpc, wi = i - j * wpc, v = var[j];
                        if (v >= 0) buf[u].v = *(const V*)(gt + (int64_t)v * row_bytes + (int64_t)s0 * P + (int64_t)wi * VB);
                    }
                }
#pragma unroll
                for (int u = 0; u < QU; ++u) {
                    const int i = i0 + u * 256;
                    if (i >= total) break;
                    const int j = i / wpc, wi = i - j * wpc;
                    const int a = var[j] >= 0 ? alle[j] : -1;       // absent: a = -1 never equals a byte read as 0 .. 255 below
                    uint8_t c[SPT];
#pragma unroll
                    for (int q = 0; q < SPT; ++q) {
                        int n = 0;
#pragma unroll
                        for (int p = 0; p < P; ++p) n += (int)(int8_t)buf[u].b[q * P + p] == a && a >= 0 ? 1 : 0;
                        c[q] = (uint8_t)n;
                    }
                    if constexpr (SPT % 4 == 0) {
#pragma unroll
                        for (int q = 0; q < SPT; q += 4)
                            *(uint32_t*)&tile[j][wi * SPT + q] = (uint32_t)c[q] | ((uint32_t)c[q + 1] << 8) |
                                                                 ((uint32_t)c[q + 2] << 16) | ((uint32_t)c[q + 3] << 24);
                    } else {
#pragma unroll
                        for (int q = 0; q < SPT; ++q) tile[j][wi * SPT + q] = c[q];
                    }
                }
            }
        } else {
            const int total = nk * ns;
            for (int i = t; i < total; i += 256) {
                const int j = i / ns, s = i - j * ns, v = var[j];
                int n = 0;
                if (v >= 0) {
                    const int8_t* g = gt + (int64_t)v * row_bytes + (int64_t)(s0 + s) * ploidy;
                    const int a = alle[j];
                    for (int p = 0; p < ploidy; ++p) n += g[p] == a ? 1 : 0;
                }
                tile[j][s] = (uint8_t)n;
            }
        }
        __syncthreads();
        // output rows whose sample lies in this chunk: wave w looks at rows w * 64 .. + 63, then + 256, ...; one coalesced
        // read of their sample indices, then one 64-byte store (lane = column) per row found
        for (int rb = w * 64; rb < n_out; rb += 256) {
            const int r = rb + lane;
            const int so = r < n_out ? sample_order[r] - s0 : -1;
            uint64_t m = __ballot(so >= 0 && so < ns);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const int s = __shfl(so, b);
                if (lane < nk) X[(int64_t)(rb + b) * x_pitch + k0 + lane] = tile[lane][s];
            }
        }
    }
}

template <int VB, int P>
static void launch_query(unsigned grid, hipStream_t st, const int8_t* gt, int64_t n_variants, int n_samples, int ploidy,
                         const int32_t* col_variant, const int8_t* col_allele, int K, const int32_t* sample_order, int n_out,
                         uint8_t* X, int64_t x_pitch) {
    hipLaunchKernelGGL((query_rows_kernel<VB, P>), dim3(grid), dim3(256), 0, st, gt, n_variants, n_samples, ploidy, col_variant,
                       col_allele, K, sample_order, n_out, X, x_pitch);
}

extern "C" int loc_query_rows(const int8_t* gt, int64_t n_variants, int n_samples, int ploidy, const int32_t* col_variant,
                              const int8_t* col_allele, int K, const int32_t* sample_order, int n_out, uint8_t* X,
                              int64_t x_pitch, void* stream) {
    if (n_variants < 0 || n_variants > ((int64_t)1 << 31) - 1 || n_samples < 1 || ploidy < 1 || ploidy > 255 ||
        (int64_t)n_samples * ploidy > (1 << 30) || K < 0 || K > (1 << 30) || n_out < 0 || x_pitch < K ||
        (n_variants > 0 && gt == nullptr) || (K > 0 && (col_variant == nullptr || col_allele == nullptr)) ||
        (n_out > 0 && K > 0 && (sample_order == nullptr || X == nullptr))) {
        loc_set_error("loc_query_rows: n_variants=%lld n_samples=%d ploidy=%d K=%d n_out=%d x_pitch=%lld", (long long)n_variants,
                      n_samples, ploidy, K, n_out, (long long)x_pitch);
        return -1;
    }
    if (K == 0 || n_out == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((K + QT - 1) / QT);
    const int64_t row_bytes = (int64_t)n_samples * ploidy;
    const uintptr_t base = (uintptr_t)gt;
    // widest load that keeps every row start (v * row_bytes) and chunk start (s0 * P, s0 a multiple of 960) aligned
    int vb = 0;
    if (ploidy <= 2) {
        for (int c = 16; c >= 4; c >>= 1)
            if (row_bytes % c == 0 && base % c == 0) { vb = c; break; }
    }
    if (vb == 16 && ploidy == 2) launch_query<16, 2>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    else if (vb == 16) launch_query<16, 1>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    else if (vb == 8 && ploidy == 2) launch_query<8, 2>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    else if (vb == 8) launch_query<8, 1>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    else if (vb == 4 && ploidy == 2) launch_query<4, 2>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    else if (vb == 4) launch_query<4, 1>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    else launch_query<0, 0>(grid, st, gt, n_variants, n_samples, ploidy, col_variant, col_allele, K, sample_order, n_out, X, x_pitch);
    LOC_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// --dosage queries (python -m locator_amd.predict / explain --dosage): the same gather for a query that holds expected
// alt-allele dosages, ds float32 [n_variants][n_samples] (NaN = missing), into the q-unit rows a LocatorNet(unit = 63) runs:
//   X[r][k] = q          if col_allele[k] == 1
//           = 126 - q    if col_allele[k] == 0 (the query swaps REF and ALT: the column counts the other allele)
//           = 0          if the column is absent, col_allele[k] is anything else, or the dosage is NaN
// with q = dosage_q_dev(ds[col_variant[k]][sample_order[r]]) (common.h).  The flip comes AFTER the quantisation, so a value
// and its flip always sum to 126.  Same shape as query_rows_kernel: QT columns per workgroup, chunks of QS samples, the
// [column][sample] byte tile, one 64-byte run per output row.  VEC: float4 loads (the host asks for them when n_samples is
// a multiple of 4 and the base is 16-byte aligned: then every row start v * n_samples and every chunk start s0 is too);
// otherwise one float per thread and step.  4 bytes read and 1 written per element; every offset into ds is 64-bit.
template <bool VEC>
__global__ __launch_bounds__(256) void query_rows_dosage_kernel(const float* __restrict__ ds, int64_t n_variants, int n_samples,
                                                                const int32_t* __restrict__ col_variant,
                                                                const int8_t* __restrict__ col_allele, int K,
                                                                const int32_t* __restrict__ sample_order, int n_out,
                                                                uint8_t* __restrict__ X, int64_t x_pitch) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[QT][QS + QPAD];
    __shared__ int32_t var[QT];
    __shared__ int32_t alle[QT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t k0 = (int64_t)blockIdx.x * QT;
    const int nk = K - k0 < QT ? (int)(K - k0) : QT;
    if (t < QT) {
        int v = -1, a = -1;
        if (t < nk) {
            v = col_variant[k0 + t];
            a = col_allele[k0 + t];
            if (v < 0 || v >= n_variants || (a != 0 && a != 1)) v = -1;     // absent (or out of range: never read)
        }
        var[t] = v;
        alle[t] = a;
    }
    constexpr int QMAX = 2 * LOC_DOSAGE_UNIT;
    for (int s0 = 0; s0 < n_samples; s0 += QS) {
        const int ns = n_samples - s0 < QS ? n_samples - s0 : QS;
        __syncthreads();                            // var / alle written; the previous chunk's tile fully read
        if constexpr (VEC) {
            const int wpc = ns / 4;                 // loads per column in this chunk (ns is a multiple of 4)
            const int total = nk * wpc;
            for (int i0 = t; i0 < total; i0 += 256 * QU) {
                float4 buf[QU];
#pragma unroll
                for (int u = 0; u < QU; ++u) {
                    const int i = i0 + u * 256;
                    buf[u] = float4{0.f, 0.f, 0.f, 0.f};
                    if (i < total) {
                        const int j = i / wpc, wi = i - j * wpc, v = var[j];
                        if (v >= 0) buf[u] = *(const float4*)(ds + (int64_t)v * n_samples + s0 + (int64_t)wi * 4);
                    }
                }
#pragma unroll
                for (int u = 0; u < QU; ++u) {
                    const int i = i0 + u * 256;
                    if (i >= total) break;
                    const int j = i / wpc, wi = i - j * wpc;
                    uint32_t word = 0;
                    if (var[j] >= 0) {
                        const bool flip = alle[j] == 0;
                        const float d[4] = {buf[u].x, buf[u].y, buf[u].z, buf[u].w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int q = dosage_q_dev(d[c]);
                            word |= (uint32_t)(q < 0 ? 0 : flip ? QMAX - q : q) << (8 * c);
                        }
                    }
                    *(uint32_t*)&tile[j][wi * 4] = word;
                }
            }
        } else {
            const int total = nk * ns;
            for (int i = t; i < total; i += 256) {
                const int j = i / ns, s = i - j * ns, v = var[j];
                int x = 0;
                if (v >= 0) {
                    const int q = dosage_q_dev(ds[(int64_t)v * n_samples + s0 + s]);
                    x = q < 0 ? 0 : alle[j] == 0 ? QMAX - q : q;
                }
                tile[j][s] = (uint8_t)x;
            }
        }
        __syncthreads();
        // as query_rows_kernel: the output rows whose sample lies in this chunk, one 64-byte store (lane = column) per row
        for (int rb = w * 64; rb < n_out; rb += 256) {
            const int r = rb + lane;
            const int so = r < n_out ? sample_order[r] - s0 : -1;
            uint64_t m = __ballot(so >= 0 && so < ns);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const int s = __shfl(so, b);
                if (lane < nk) X[(int64_t)(rb + b) * x_pitch + k0 + lane] = tile[lane][s];
            }
        }
    }
}

extern "C" int loc_query_rows_dosage(const float* ds, int64_t n_variants, int n_samples, const int32_t* col_variant,
                                     const int8_t* col_allele, int K, const int32_t* sample_order, int n_out, uint8_t* X,
                                     int64_t x_pitch, void* stream) {
    if (n_variants < 0 || n_variants > ((int64_t)1 << 31) - 1 || n_samples < 1 || n_samples > (1 << 30) || K < 0 ||
        K > (1 << 30) || n_out < 0 || x_pitch < K || (n_variants > 0 && ds == nullptr) ||
        (K > 0 && (col_variant == nullptr || col_allele == nullptr)) ||
        (n_out > 0 && K > 0 && (sample_order == nullptr || X == nullptr))) {
        loc_set_error("loc_query_rows_dosage: n_variants=%lld n_samples=%d K=%d n_out=%d x_pitch=%lld", (long long)n_variants,
                      n_samples, K, n_out, (long long)x_pitch);
        return -1;
    }
    if (K == 0 || n_out == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((K + QT - 1) / QT);
    if (n_samples % 4 == 0 && (uintptr_t)ds % 16 == 0)
        hipLaunchKernelGGL(query_rows_dosage_kernel<true>, dim3(grid), dim3(256), 0, st, ds, n_variants, n_samples, col_variant,
                           col_allele, K, sample_order, n_out, X, x_pitch);
    else
        hipLaunchKernelGGL(query_rows_dosage_kernel<false>, dim3(grid), dim3(256), 0, st, ds, n_variants, n_samples, col_variant,
                           col_allele, K, sample_order, n_out, X, x_pitch);
    LOC_CHECK_LAUNCH();
    return 0;
}
