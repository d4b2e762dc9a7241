// The haplotype copying model of the paint command (locator_amd/paint.py): loc_paint_copy, defined in
// include/locator_hip_paint.h; the NumPy form paint.copy_host is what tests/test_gpu_paint.py holds it to.  Plain vector code,
// every operation fp32 and uncontracted except the fused multiply-adds that are written out.
//
// One wave (a workgroup of its own) runs one recipient: K dependent site steps, each an elementwise pass over the H columns and
// one or two sums over them.  The state lives in registers: lane l holds the columns 4 l + 256 i + x (i < NR, x < 4), so that a
// lane reads the alleles of four of its columns as one dword of the site's row and a-hat as one float4.  NR = 1, 2, 4, 8 or 16
// by H; the columns past H up to 256 NR are never donors and add exact zeros.
// paint_kernel, in order:
//   the donor mask (one bit a value of the lane) and D;
//   the forward pass over all sites: ll, and a-hat after every `block`-th site into the recipient's checkpoints;
//   for the blocks from the last to the first: a-hat of the block's sites recomputed from its checkpoint into the recipient's
//   scratch rows by the same pk_forward, then the backward walk over the block, which reads a row back (each lane the floats it
//   wrote itself, c_j from a slot of its own behind the row: no lane reads what another wrote).
// The next site's alleles (forward) and the previous site's a-hat row (backward) are requested before the current site's
// arithmetic, so that the wave does not stand still for the whole latency of a load at every one of its K steps.
// The pk_* functions and the launcher's layout and refusals are in paint_core.h, which impute_kernels.hip shares.
#include "paint_core.h"

template <int NR>
__global__ __launch_bounds__(64) void paint_kernel(const int8_t* __restrict__ h, int H, int64_t K, int64_t pitch,
                                                   const uint8_t* __restrict__ donor, const int32_t* __restrict__ owner,
                                                   const int32_t* __restrict__ rec, const float* __restrict__ rho, float theta, int64_t B,
                                                   float* __restrict__ share, float* __restrict__ chunks, double* __restrict__ ll,
                                                   int32_t* __restrict__ n_donors, float* __restrict__ work, int64_t per_rec) {
    constexpr int64_t HP = (int64_t)PK_SWEEP * NR, STRIDE = HP + PK_CS;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const int rc = rec[r];
    if (rc < 0 || rc >= H) return;                          // the launcher has refused it
    const int own = owner[rc];
    uint64_t mask = 0;
    int D = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) {
            const int d = PK_X * lane + PK_SWEEP * i + x;
            if (d < H && donor[d] != 0 && owner[d] != own) {
                mask |= (uint64_t)1 << (PK_X * i + x);
                ++D;
            }
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) D += __shfl_xor(D, d, 64);
    float* const sh = share + r * H;
    float* const ch = chunks + r * H;
    if (lane == 0) n_donors[r] = D;
    if (D == 0) {
        for (int d = lane; d < H; d += 64) {
            sh[d] = 0.0f;
            ch[d] = 0.0f;
        }
        if (lane == 0) ll[r] = 0.0;
        return;
    }
    const float u = 1.0f / (float)D, th = theta, omt = 1.0f - theta;
    const int64_t nb = (K + B - 1) / B;
    float* const ck = work + r * per_rec;                    // nb - 1 checkpoints of HP floats
    float* const sc = ck + (nb - 1) * HP;                    // B rows of STRIDE floats

    float ah[NR][PK_X];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) ah[i][x] = 0.0f;
    const double L = pk_run<NR, true>(h, pitch, rc, lane, rho, 0, K, K, B, ah, mask, u, th, omt, ck, HP);
    if (lane == 0) ll[r] = L;

    float b[NR][PK_X], sa[NR][PK_X], ca[NR][PK_X], nx[NR][PK_X];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) {
            b[i][x] = u;
            sa[i][x] = 0.0f;
            ca[i][x] = 0.0f;
        }
    for (int64_t k = nb - 1; k >= 0; --k) {
        const int64_t lo = k * B, hi = lo + B < K ? lo + B : K;
        if (k == 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int x = 0; x < PK_X; ++x) ah[i][x] = 0.0f;
        } else {
            pk_load_row<NR>(ck + (k - 1) * HP, lane, ah);
        }
        pk_run<NR, false>(h, pitch, rc, lane, rho, lo, hi, K, B, ah, mask, u, th, omt, sc, STRIDE);

        uint32_t w[NR], wn[NR];
        int ar, arn;
        float cj, cn;
        pk_load_alleles<NR>(h, hi - 1, pitch, rc, lane, wn, arn);
        pk_load_row<NR>(sc + (hi - 1 - lo) * STRIDE, lane, nx);
        cn = sc[(hi - 1 - lo) * STRIDE + HP + lane];
        for (int64_t j = hi - 1; j >= lo; --j) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                w[i] = wn[i];
#pragma unroll
                for (int x = 0; x < PK_X; ++x) ah[i][x] = nx[i][x];
            }
            ar = arn;
            cj = cn;
            const int64_t jp = j > lo ? j - 1 : j;
            pk_load_alleles<NR>(h, jp, pitch, rc, lane, wn, arn);
            pk_load_row<NR>(sc + (jp - lo) * STRIDE, lane, nx);
            cn = sc[(jp - lo) * STRIDE + HP + lane];

            // first sweep: b <- t = e b, ah <- g = a-hat b, and their sums
            float sT[PK_X] = {0.0f, 0.0f, 0.0f, 0.0f}, sG[PK_X] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                float e[PK_X];
                pk_emit(w[i], ar, (uint32_t)(mask >> (PK_X * i)) & 15u, th, omt, e);
#pragma unroll
                for (int x = 0; x < PK_X; ++x) {
                    const float g = ah[i][x] * b[i][x], t = e[x] * b[i][x];
                    ah[i][x] = g;
                    b[i][x] = t;
                    sG[x] = sG[x] + g;
                    sT[x] = sT[x] + t;
                }
            }
            float T = pk_lane4(sT), G = pk_lane4(sG);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                if (PK_ABLATE & 1) break;
                T = T + __shfl_xor(T, d, 64);
                G = G + __shfl_xor(G, d, 64);
            }
            const float invG = G >= FLT_MIN ? 1.0f / G : 0.0f;
            const float rj = j == 0 ? 1.0f : rho[j];
            const float ru = rj * u;
            const float coef = (ru * invG) * (1.0f / cj);    // in this order no factor leaves fp32: rho u / G <= c / T
            const float kb = (1.0f - rj) * (1.0f / T);
            const bool first = j == 0;
            // second sweep: the posterior into the two sums, and b_(j-1)
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int x = 0; x < PK_X; ++x) {
                    const float gam = ah[i][x] * invG;
                    sa[i][x] = sa[i][x] + gam;
                    ca[i][x] = ca[i][x] + (first ? gam : b[i][x] * coef);
                    b[i][x] = __builtin_fmaf(kb, b[i][x], ru);
                }
        }
    }
    const float fK = (float)K;
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) {
            const int d = PK_X * lane + PK_SWEEP * i + x;
            if (d < H) {
                sh[d] = sa[i][x] / fK;
                ch[d] = ca[i][x];
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------- launcher
extern "C" int64_t loc_paint_work_bytes(int H, int64_t K, int R, int block) {
    if (!pk_sizes_ok("loc_paint_work_bytes", H, K, R, block)) return -1;
    return pk_work(H, K, R, block).bytes;
}

extern "C" int loc_paint_copy(const int8_t* h, int H, int64_t K, int64_t pitch, const uint8_t* donor, const int32_t* owner,
                              const int32_t* rec, int R, const float* rho, float theta, int block, float* share, float* chunks,
                              double* ll, int32_t* n_donors, void* work, int64_t work_bytes, void* stream) {
    const pk_call c = {h, H, K, pitch, donor, owner, rec, R, rho, theta, block, ll, n_donors, work, work_bytes, (hipStream_t)stream};
    const size_t rows = (size_t)(R > 0 ? R : 0) * (size_t)H * sizeof(float);
    const pk_out outs[] = {{"share", share, rows}, {"chunks", chunks, rows}};
    pk_layout L;
    int rc;
    if (!pk_enter("loc_paint_copy", c, outs, 2, L, rc)) return rc;
    pk_dispatch(H, [&](auto nr) {
        hipLaunchKernelGGL(paint_kernel<decltype(nr)::value>, dim3((unsigned)R), dim3(64), 0, c.stream, h, H, K, pitch, donor, owner, rec,
                           rho, theta, L.B, share, chunks, ll, n_donors, (float*)work, L.per_rec);
    });
    return pk_launched("pk_launch");                          // the name this message has carried since the first launcher
}
