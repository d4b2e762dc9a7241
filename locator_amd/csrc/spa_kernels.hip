// The two kernels of the spa command (locator_amd/spa.py): a logistic allele-frequency surface per site, fitted by Newton steps
// (spa_fit_kernel), and the genotype log-likelihood of every sample at every node of a grid on the fp32 matrix pipe
// (spa_grid_kernel + spa_reduce_kernel).  The definitions are in include/locator_hip_spa.h; the NumPy forms (spa.fit_host,
// spa.grid_host) are what tests/test_gpu_spa.py holds both to.
//
// spa_grid_kernel is a rectangular sibling of grm_pairs_kernel (grm_kernels.hip): from the skeleton of pair_tiles.h it keeps
// the 16-byte loader (a row past Q and a site past K read as missing), operands formed in registers on the way to LDS, the next
// block requested with plain loads before the MFMAs of the current one, the split of the site blocks over groups, the LDS
// placement and the operand lanes of grm_pairs_kernel.  Its own:
// Work split: a plain 2-D tile index, blockIdx.x = the node tile, blockIdx.y = the sample tile, blockIdx.z = the site group.
// A tile is 256 samples x 128 nodes and a workgroup 512 threads = 8 waves, wave w the 64 x 64 block (w >> 1, w & 1): the
// (site, node) operands cost about 140 vector instructions a value (log1pf is a double-float routine), as much vector time as
// the MFMAs take matrix time at 128 samples a tile (measured: 0.47 of the matrix peak); twice the samples share them.
// Operands: images of [rows][32 sites] floats.  Sample side (256 rows): a = max(c, 0) and m = -P [c >= 0].  Node side (128
// rows): t and softplus(t), formed per (site, node) from theta in registers; the K x G surface is never written to memory.
// A thread owns ONE node for the whole launch (its gx, gy stay in registers) and 8 sites of every block; the block's 32
// thetas (ax, ay, b, used) are double-buffered in LDS and run two blocks ahead of the counts (see the loop).  An unused site
// has t = 0 by selection and softplus times used = 0.
// Two accumulators a tile, acc_t += a t and acc_s += m sp, 128 registers a thread: one shared accumulator would put 2 B terms
// in a chain and double the rounding bound (B + 8) 2^-24 sum |terms| the tests hold the launch to.  They are added once, in
// fp32, on the way to the group's slab.
// Reduction: spa_reduce_kernel adds the slabs of an element in group order in double: no floating-point atomics, the same
// bits on every launch, no scratch byte read that this launch did not write.
//
// spa_fit_kernel: one wave per site, LOC_SPA_FIT_SITES sites per workgroup, everything fp32 and uncontracted.  Per Newton step
// the workgroup walks the samples LOC_SPA_FIT_CHUNK at a time: xy and w are staged in LDS (placed i + (i >> 4): a lane's 16
// consecutive samples start 17 dwords apart), lane l loads the 16 counts of samples 16 l .. 16 l + 15 of the chunk with one
// 16-byte load (pt_load_piece: pad bytes never interpreted) and adds their terms to nine running sums in ascending order; the 64
// lanes are added by an xor butterfly, after which every lane holds the same bits and solves the 3 x 3 system on its own.
// It runs K N iters operations against the grid's 2 Q K G and is kept plain.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_spa.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

constexpr int SP_TQ = LOC_SPA_TILE_SAMPLES;       // samples of a tile
constexpr int SP_T = LOC_SPA_TILE;                // nodes of a tile
constexpr int SP_B = LOC_SPA_BLOCK;
constexpr int SP_NT = 512;                        // 8 waves: wave w owns the 64 x 64 block (w >> 1, w & 1) of the 256 x 128 tile
constexpr int SP_SIDE_Q = SP_TQ * SP_B;           // floats of one sample image
constexpr int SP_SIDE_G = SP_T * SP_B;            // floats of one node image
static_assert(SP_T == PT_T && SP_B == 32 && SP_TQ * SP_B / 16 == SP_NT && SP_T * SP_B / 8 == SP_NT,
              "a 16-site piece of counts and 8 (site, node) values per thread and block");

__device__ __forceinline__ int sp_byte(uint32_t w, int e) { return (int)(w << (24 - 8 * e)) >> 24; }
__device__ __forceinline__ int sp_at(int row, int piece) { return row * SP_B + ((piece ^ ((row >> 1) & 7)) << 2); }

__device__ __forceinline__ float sp_softplus(float t) { return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t))); }

// the sample side: a = max(c, 0), m = -P [c >= 0]
__device__ __forceinline__ void sp_store_samples(float* img_a, float* img_m, int row, int chunk, uint4 raw, float negP) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f32x4 a, m;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int cv = sp_byte(w[e], x);
            a[x] = cv > 0 ? (float)cv : 0.f;
            m[x] = cv >= 0 ? negP : 0.f;
        }
        *reinterpret_cast<f32x4*>(img_a + sp_at(row, 4 * chunk + e)) = a;
        *reinterpret_cast<f32x4*>(img_m + sp_at(row, 4 * chunk + e)) = m;
    }
}

// the node side: t and softplus(t) of one node at two sites (elements x0, x0 + 1 of piece e of `chunk`), from the block's thetas
__device__ __forceinline__ void sp_form_nodes(f32x4& tv, f32x4& sv, int chunk, int e, int x0, const f32x4* th, float gx, float gy) {
#pragma unroll
    for (int x = x0; x < x0 + 2; ++x) {
        const f32x4 p = th[16 * chunk + 4 * e + x];                    // ax, ay, b, used: the same address over the half-wave
        const float lin = p[0] * gx + p[1] * gy;                       // three roundings: contraction is off
        const bool on = p[3] != 0.f;
        const float t = on ? lin + p[2] : 0.f;                         // selected first: an unused site has t = 0 whatever
        tv[x] = t;                                                     // theta holds, softplus(0) = log 2 is finite, and
        sv[x] = sp_softplus(t) * p[3];                                 // times used = 0 / 1 it is exact.  A product, not a
    }                                                                  // select: the compiler guards a select's softplus by
                                                                       // a branch, and no MFMA can be placed across one
}

__global__ __launch_bounds__(SP_NT, 2) void spa_grid_kernel(const int8_t* __restrict__ c, int Q, int64_t K, int64_t pitch, float negP,
                                                         const float* __restrict__ theta, const uint8_t* __restrict__ used,
                                                         const float* __restrict__ gx, const float* __restrict__ gy, int G,
                                                         int64_t blocks_per_group, float* __restrict__ slabs) {
    __shared__ __attribute__((aligned(16))) float lds[2 * SP_SIDE_Q + 2 * SP_SIDE_G];
    __shared__ __attribute__((aligned(16))) f32x4 th[2][SP_B];
    float* const img_a = lds;
    float* const img_m = lds + SP_SIDE_Q;
    float* const img_t = lds + 2 * SP_SIDE_Q;
    float* const img_s = lds + 2 * SP_SIDE_Q + SP_SIDE_G;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t nblocks = (K + SP_B - 1) / SP_B;
    const int64_t b0 = (int64_t)blockIdx.z * blocks_per_group;
    const int64_t b1 = min(nblocks, b0 + blocks_per_group);        // the launcher starts no group past the last block: b0 < b1
    const int64_t row0 = (int64_t)blockIdx.y * SP_TQ;
    const int srow = t >> 1, schunk = t & 1;      // the piece of counts this thread stages: row srow, sites 16 schunk .. + 15
    // ... and its (site, node) values: node nrow at the 8 sites 16 nchunk + 8 nhalf .. + 7, the pieces 2 nhalf, 2 nhalf + 1
    const int nrow = t >> 2, nchunk = (t >> 1) & 1, nhalf = t & 1;
    const int node = (int)blockIdx.x * SP_T + nrow;
    const float my_gx = node < G ? gx[node] : 0.f, my_gy = node < G ? gy[node] : 0.f;

    uint4 raw;
    f32x4 par = {0.f, 0.f, 0.f, 0.f};
    auto request_counts = [&](int64_t b) { raw = pt_load_piece(c, row0 + srow, Q, b * SP_B + 16 * schunk, K, pitch); };
    auto request_thetas = [&](int64_t b) {
        if (t < SP_B) {
            const int64_t k = b * SP_B + t;
            par = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < K) {
                par = *reinterpret_cast<const f32x4*>(theta + 4 * k);
                par[3] = used[k] ? 1.f : 0.f;
            }
        }
    };

    f32x16 acc_t[2][2], acc_s[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_t[tm][tn][r] = acc_s[tm][tn][r] = 0.f;

    const int arow = pt_arow(w, lane), brow = pt_brow(w, lane), half = pt_half(lane);
    // The node operands of block b + 1 are formed in registers BETWEEN the MFMAs of block b (two sites per step of eight):
    // the vector ALU works on softplus while the matrix pipe runs.  So the thetas run two blocks ahead of the counts: those of
    // block b + 1 are stored in front of block b's first barrier, those of block b + 2 requested behind it.
    f32x4 nt[2], ns[2];
    request_counts(b0);
    request_thetas(b0);
    if (t < SP_B) th[b0 & 1][t] = par;
    if (b0 + 1 < b1) request_thetas(b0 + 1);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) sp_form_nodes(nt[s >> 1], ns[s >> 1], nchunk, 2 * nhalf + (s >> 1), 2 * (s & 1), th[b0 & 1], my_gx, my_gy);
    for (int64_t b = b0; b < b1; ++b) {
        sp_store_samples(img_a, img_m, srow, schunk, raw, negP);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<f32x4*>(img_t + sp_at(nrow, 4 * nchunk + 2 * nhalf + j)) = nt[j];
            *reinterpret_cast<f32x4*>(img_s + sp_at(nrow, 4 * nchunk + 2 * nhalf + j)) = ns[j];
        }
        if (b + 1 < b1 && t < SP_B) th[(b + 1) & 1][t] = par;          // its last readers formed block b - 1 behind b - 2's barrier
        __syncthreads();
        if (b + 1 < b1) request_counts(b + 1);
        if (b + 2 < b1) request_thetas(b + 2);
        const f32x4* const next = th[(b + 1) & 1];                     // behind the last block: stale values, formed and dropped
#pragma unroll
        for (int s = 0; s < SP_B / 8; ++s) {
            const int piece = 2 * s + half;
            f32x4 a[2], m[2], tt[2], ss[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const f32x4*>(img_a + sp_at(arow + 32 * i, piece));
                m[i] = *reinterpret_cast<const f32x4*>(img_m + sp_at(arow + 32 * i, piece));
                tt[i] = *reinterpret_cast<const f32x4*>(img_t + sp_at(brow + 32 * i, piece));
                ss[i] = *reinterpret_cast<const f32x4*>(img_s + sp_at(brow + 32 * i, piece));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) {
                        acc_t[tm][tn] = mfma32(a[tm][q], tt[tn][q], acc_t[tm][tn]);
                        acc_s[tm][tn] = mfma32(m[tm][q], ss[tn][q], acc_s[tm][tn]);
                    }
            sp_form_nodes(nt[s >> 1], ns[s >> 1], nchunk, 2 * nhalf + (s >> 1), 2 * (s & 1), next, my_gx, my_gy);
            // the wave issues in order: without this the 32 MFMAs of the step go out in one burst and the softplus code
            // waits behind them.  One MFMA (16 passes of the matrix pipe), then the vector instructions that fit under it.
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
            }
        }
        __syncthreads();                          // the block is consumed: the next one may overwrite it
    }

    const int64_t tile = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    float* const slab = slabs + tile * (int64_t)(SP_TQ * SP_T);
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int jl = 64 * (w & 1) + 32 * tn + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int il = 64 * (w >> 1) + 32 * tm + rowmap(r, half);
                slab[il * SP_T + jl] = acc_t[tm][tn][r] + acc_s[tm][tn][r];
            }
        }
}

// grid.x = the node tiles, grid.y = the sample tiles, grid.z * 256 threads = the 256 x 128 elements of a tile
__global__ __launch_bounds__(256) void spa_reduce_kernel(const float* __restrict__ slabs, int groups, int Q, int G,
                                                         double* __restrict__ ll) {
    const int e = (int)blockIdx.z * 256 + (int)threadIdx.x;
    const int64_t q = (int64_t)blockIdx.y * SP_TQ + (e >> 7);
    const int g = (int)blockIdx.x * SP_T + (e & 127);
    if (q >= Q || g >= G) return;
    const int64_t tiles = (int64_t)gridDim.x * gridDim.y, tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    double s = 0.0;
    for (int z = 0; z < groups; ++z) s += (double)slabs[(z * tiles + tile) * (int64_t)(SP_TQ * SP_T) + e];
    ll[q * G + g] = s;
}

// ---------------------------------------------------------------------------------------------------------------- the fit
constexpr int SF_NT = 64 * LOC_SPA_FIT_SITES;
constexpr int SF_CHUNK = LOC_SPA_FIT_CHUNK;
constexpr int SF_PER = SF_CHUNK / SF_NT;          // samples a thread stages per chunk
static_assert(SF_CHUNK == 16 * 64 && SF_CHUNK % SF_NT == 0, "a lane takes 16 samples of a chunk: one 16-byte piece");
constexpr float SF_TINY = 1e-30f;

__device__ __forceinline__ int sf_at(int i) { return i + (i >> 4); }

__device__ __forceinline__ float sf_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int sf_wave_sum_i(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float sf_clamp(float v) {
    return fminf(fmaxf(v, -(float)LOC_SPA_MAX_STEP), (float)LOC_SPA_MAX_STEP);
}

__global__ __launch_bounds__(SF_NT) void spa_fit_kernel(const int8_t* __restrict__ ct, int64_t K, int N, int64_t pitch, int P,
                                                        const float* __restrict__ xy, const uint8_t* __restrict__ w, float ridge,
                                                        int iters, float* __restrict__ theta, uint8_t* __restrict__ used) {
    __shared__ float xs[SF_CHUNK + SF_CHUNK / 16], ys[SF_CHUNK + SF_CHUNK / 16];
    __shared__ uint8_t ws[SF_CHUNK + SF_CHUNK / 16];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t k = (int64_t)blockIdx.x * LOC_SPA_FIT_SITES + (t >> 6);          // rows past K read as missing: never stored
    const int nchunks = (N + SF_CHUNK - 1) / SF_CHUNK;
    const float fP = (float)P;

    // stage the chunk's xy and w; a sample past N or outside w is off, its xy is not read
    auto stage = [&](int ch) {
        __syncthreads();                          // the previous chunk is consumed
#pragma unroll
        for (int x = 0; x < SF_PER; ++x) {
            const int i = t + SF_NT * x;
            const int64_t s = (int64_t)ch * SF_CHUNK + i;
            const bool on = s < N && w[s] == 1;
            ws[sf_at(i)] = on ? 1 : 0;
            xs[sf_at(i)] = on ? xy[2 * s] : 0.f;
            ys[sf_at(i)] = on ? xy[2 * s + 1] : 0.f;
        }
        __syncthreads();
    };
    auto piece = [&](int ch) { return pt_load_piece(ct, k, (int)min(K, (int64_t)0x7fffffff), (int64_t)ch * SF_CHUNK + 16 * lane, N, pitch); };

    // n and s over the samples of w with a call
    int n = 0, sum = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        stage(ch);
        const uint4 raw = piece(ch);
        const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int cv = sp_byte(wd[e >> 2], e & 3);
            const bool on = cv >= 0 && ws[sf_at(16 * lane + e)];
            n += on ? 1 : 0;
            sum += on ? cv : 0;
        }
    }
    n = sf_wave_sum_i(n);
    sum = sf_wave_sum_i(sum);
    const bool fit = n > 0 && sum > 0 && sum < P * n;                             // wave-uniform
    float ax = 0.f, ay = 0.f, b = fit ? logf((float)sum) - logf((float)(P * n - sum)) : 0.f, last = 0.f;

    for (int it = 0; it < iters; ++it) {
        float g1 = 0.f, g2 = 0.f, g3 = 0.f, h11 = 0.f, h12 = 0.f, h13 = 0.f, h22 = 0.f, h23 = 0.f, h33 = 0.f;
        for (int ch = 0; ch < nchunks; ++ch) {
            stage(ch);
            const uint4 raw = piece(ch);
            const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int cv = sp_byte(wd[e >> 2], e & 3);
                const int at = sf_at(16 * lane + e);
                const bool on = cv >= 0 && ws[at];
                const float x = on ? xs[at] : 0.f, y = on ? ys[at] : 0.f;     // a sample without a call: its xy is not interpreted
                const float tt = (ax * x + ay * y) + b;
                const float f = 1.f / (1.f + expf(-tt));
                const float r = on ? (float)cv - fP * f : 0.f;
                const float v = on ? (fP * f) * (1.f - f) : 0.f;
                const float vx = v * x, vy = v * y;
                g1 = g1 + r * x;
                g2 = g2 + r * y;
                g3 = g3 + r;
                h11 = h11 + vx * x;
                h12 = h12 + vx * y;
                h13 = h13 + vx;
                h22 = h22 + vy * y;
                h23 = h23 + vy;
                h33 = h33 + v;
            }
        }
        g1 = sf_wave_sum(g1) - ridge * ax;
        g2 = sf_wave_sum(g2) - ridge * ay;
        g3 = sf_wave_sum(g3);
        h11 = sf_wave_sum(h11) + ridge;
        h12 = sf_wave_sum(h12);
        h13 = sf_wave_sum(h13);
        h22 = sf_wave_sum(h22) + ridge;
        h23 = sf_wave_sum(h23);
        h33 = sf_wave_sum(h33);
        // L D L' without pivoting, pivots floored
        const float d1 = fmaxf(h11, SF_TINY);
        const float l21 = h12 / d1, l31 = h13 / d1;
        const float d2 = fmaxf(h22 - l21 * h12, SF_TINY);
        const float l32 = (h23 - l31 * h12) / d2;
        const float d3 = fmaxf((h33 - l31 * h13) - l32 * (l32 * d2), SF_TINY);
        const float z1 = g1, z2 = g2 - l21 * z1, z3 = (g3 - l31 * z1) - l32 * z2;
        float s3 = z3 / d3;
        float s2 = z2 / d2 - l32 * s3;
        float s1 = (z1 / d1 - l21 * s2) - l31 * s3;
        s1 = sf_clamp(s1);
        s2 = sf_clamp(s2);
        s3 = sf_clamp(s3);
        ax = ax + s1;
        ay = ay + s2;
        b = b + s3;
        last = fmaxf(fmaxf(fabsf(s1), fabsf(s2)), fabsf(s3));
    }
    if (lane == 0 && k < K) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (fit) o = f32x4{ax, ay, b, last};
        *reinterpret_cast<f32x4*>(theta + 4 * k) = o;
        used[k] = fit ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
static bool sp_common_ok(const char* who, int rows, int64_t K, int P) {
    if (rows < 0 || K < 0 || rows >= (1 << 20) || K >= ((int64_t)1 << 31) || P < 1 || P > 2) {
        loc_set_error("%s: rows=%d K=%lld P=%d (sizes may not be negative; rows must stay below 2^20, K below 2^31, P 1 or 2)", who,
                      rows, (long long)K, P);
        return false;
    }
    return true;
}

extern "C" int loc_spa_fit(const int8_t* ct, int64_t K, int N, int64_t pitch, int P, const float* xy, const uint8_t* w, float ridge,
                           int iters, float* theta, uint8_t* used, void* stream) {
    if (!sp_common_ok("loc_spa_fit", N, K, P)) return -1;
    if (pitch < N || iters < 1 || iters > LOC_SPA_MAX_ITERS || !std::isfinite(ridge) || ridge < 0.f) {
        loc_set_error("loc_spa_fit: N=%d pitch=%lld iters=%d ridge=%g (pitch >= N, iters 1 .. %d, ridge finite and >= 0)", N,
                      (long long)pitch, iters, (double)ridge, LOC_SPA_MAX_ITERS);
        return -1;
    }
    if (K == 0) return 0;
    if (!theta || !used || (N > 0 && (!ct || !xy || !w))) {
        loc_set_error("loc_spa_fit: null buffer");
        return -1;
    }
    if (N > 0 && !pt_rows_aligned("loc_spa_fit", ct, pitch)) return -1;
    if ((uintptr_t)theta % 16 != 0 || (uintptr_t)xy % 8 != 0) {
        loc_set_error("loc_spa_fit: theta must be a multiple of 16 bytes, xy of 8");
        return -1;
    }
    const int64_t groups = (K + LOC_SPA_FIT_SITES - 1) / LOC_SPA_FIT_SITES;
    hipLaunchKernelGGL(spa_fit_kernel, dim3((unsigned)groups), dim3(SF_NT), 0, (hipStream_t)stream, ct, K, N, pitch, P, xy, w, ridge,
                       iters, theta, used);
    LOC_CHECK_LAUNCH();
    return 0;
}

static int64_t sp_tiles(int n, int side) { return ((int64_t)n + side - 1) / side; }

// the site groups of a launch (pair_tiles.h): as gr_split of grm_kernels.hip, over the rectangle's tiles
static pt_groups sp_split(int Q, int64_t K, int G, int k_groups) {
    // pt_site_groups counts two workgroup slots a compute unit; 99 KiB of LDS and 8 waves of 244 registers leave this kernel one
    return pt_site_groups((K + SP_B - 1) / SP_B, sp_tiles(Q, SP_TQ) * sp_tiles(G, SP_T), k_groups,
                          std::max(1, sr_compute_units() / 2), 8, 16);
}

static bool sp_grid_sizes_ok(const char* who, int Q, int64_t K, int G, int k_groups) {
    if (Q < 0 || K < 0 || Q >= (1 << 20) || K >= ((int64_t)1 << 31) || G < 1 || G > LOC_SPA_MAX_NODES || k_groups < 0) {
        loc_set_error("%s: Q=%d K=%lld G=%d k_groups=%d (none may be negative; Q below 2^20, K below 2^31, G 1 .. %d)", who, Q,
                      (long long)K, G, k_groups, LOC_SPA_MAX_NODES);
        return false;
    }
    return true;
}

extern "C" int64_t loc_spa_grid_work_bytes(int Q, int64_t K, int G, int k_groups) {
    if (!sp_grid_sizes_ok("loc_spa_grid_work_bytes", Q, K, G, k_groups)) return -1;
    return sp_split(Q, K, G, k_groups).groups * sp_tiles(Q, SP_TQ) * sp_tiles(G, SP_T) * (int64_t)(SP_TQ * SP_T * sizeof(float));
}

extern "C" int loc_spa_grid(const int8_t* c, int Q, int64_t K, int64_t pitch, int P, const float* theta, const uint8_t* used,
                            const float* gx, const float* gy, int G, int k_groups, double* ll, void* work, int64_t work_bytes,
                            void* stream) {
    if (!sp_grid_sizes_ok("loc_spa_grid", Q, K, G, k_groups) || !sp_common_ok("loc_spa_grid", Q, K, P) ||
        !pt_sizes_ok("loc_spa_grid", Q, K, pitch, k_groups, work_bytes))
        return -1;
    if (Q == 0) return 0;
    if (!ll || !gx || !gy || (K > 0 && (!c || !theta || !used))) {
        loc_set_error("loc_spa_grid: null buffer");
        return -1;
    }
    if (K > 0 && !pt_rows_aligned("loc_spa_grid", c, pitch)) return -1;
    if ((uintptr_t)ll % 8 != 0 || (uintptr_t)gx % 4 != 0 || (uintptr_t)gy % 4 != 0 || (K > 0 && (uintptr_t)theta % 16 != 0)) {
        loc_set_error("loc_spa_grid: theta must be a multiple of 16 bytes, ll of 8, gx and gy of 4");
        return -1;
    }
    const pt_groups split = sp_split(Q, K, G, k_groups);
    const int64_t tq = sp_tiles(Q, SP_TQ), tg = sp_tiles(G, SP_T);
    const int64_t need = split.groups * tq * tg * (int64_t)(SP_TQ * SP_T * sizeof(float));
    if (tq * tg * std::max<int64_t>(split.groups, 1) > ((int64_t)1 << 16)) {       // 2^16 slabs are 8 GiB of scratch
        loc_set_error("loc_spa_grid: Q=%d G=%d in %lld site groups exceed one launch", Q, G, (long long)split.groups);
        return -1;
    }
    if (!pt_work_ok("loc_spa_grid", "loc_spa_grid_work_bytes", work, work_bytes, need)) return -1;
    if (split.groups > 0) {
        hipLaunchKernelGGL(spa_grid_kernel, dim3((unsigned)tg, (unsigned)tq, (unsigned)split.groups), dim3(SP_NT), 0,
                           (hipStream_t)stream, c, Q, K, pitch, -(float)P, theta, used, gx, gy, G, split.per, (float*)work);
        LOC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(spa_reduce_kernel, dim3((unsigned)tg, (unsigned)tq, SP_TQ * SP_T / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float*)work, (int)split.groups, Q, G, ll);                // no group: every sum is 0
    LOC_CHECK_LAUNCH();
    return 0;
}
