// The allele dosages of the impute command (locator_amd/impute.py): loc_impute_dose, defined in include/locator_hip_impute.h;
// the NumPy form impute.dose_host is what tests/test_gpu_impute.py holds it to.  The copying model is paint_kernels.hip's, by the
// same pk_* functions (paint_core.h): one wave a recipient, the state in registers, the forward pass with checkpoints (ll), then
// block by block from the last the recomputation of a-hat into scratch and the backward walk with its prefetch of the previous
// row.  The walk differs: it forms no G, no share and no chunks, so it holds a-hat, b and the prefetched row and no accumulator a
// column; instead the posterior weight g = a-hat b is summed over the columns that hold allele 1 and over those that hold
// allele 0, two lane sums that ride in the butterfly of T, and the site's dose is A1 / (A0 + A1).
// Output: the walk descends over all sites K - 1 .. 0, across the blocks.  Lane j % 64 keeps the dose of site j, and when the
// walk reaches a site that is a multiple of 64 the wave writes the sites j .. min(j + 63, K - 1) with one store instruction, each
// lane its own: every element of the recipient's row exactly once, 256 contiguous bytes a store.
#include "paint_core.h"

#include "../../include/locator_hip_impute.h"

constexpr int IK_RUN = LOC_IMPUTE_STORE_RUN;
static_assert(IK_RUN == 64, "a site a lane");

template <int NR>
__global__ __launch_bounds__(64) void impute_kernel(const int8_t* __restrict__ h, int H, int64_t K, int64_t pitch,
                                                    const uint8_t* __restrict__ donor, const int32_t* __restrict__ owner,
                                                    const int32_t* __restrict__ rec, const float* __restrict__ rho, float theta, int64_t B,
                                                    float* __restrict__ dose, double* __restrict__ ll, int32_t* __restrict__ n_donors,
                                                    float* __restrict__ work, int64_t per_rec) {
    constexpr int64_t HP = (int64_t)PK_SWEEP * NR, STRIDE = HP + PK_CS;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const int rc = rec[r];
    if (rc < 0 || rc >= H) return;                          // the launcher has refused it
    int D;
    const uint64_t mask = pk_donor_mask<NR>(donor, owner, H, owner[rc], lane, D);
    float* const out = dose + r * K;
    const float nan = __builtin_nanf("");
    if (lane == 0) n_donors[r] = D;
    if (D == 0) {
        for (int64_t j = lane; j < K; j += 64) out[j] = nan;
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

    float b[NR][PK_X], nx[NR][PK_X];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) b[i][x] = u;
    float keep = nan;                                        // the dose of the site j with j % 64 == lane, until its run is stored
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
        pk_load_alleles<NR>(h, hi - 1, pitch, rc, lane, wn, arn);
        pk_load_row<NR>(sc + (hi - 1 - lo) * STRIDE, lane, nx);
        for (int64_t j = hi - 1; j >= lo; --j) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                w[i] = wn[i];
#pragma unroll
                for (int x = 0; x < PK_X; ++x) ah[i][x] = nx[i][x];
            }
            ar = arn;
            const int64_t jp = j > lo ? j - 1 : j;
            pk_load_alleles<NR>(h, jp, pitch, rc, lane, wn, arn);
            pk_load_row<NR>(sc + (jp - lo) * STRIDE, lane, nx);

            // b <- t = e b; g = a-hat b into the sum of its column's allele
            float sT[PK_X] = {0.0f, 0.0f, 0.0f, 0.0f}, s0[PK_X] = {0.0f, 0.0f, 0.0f, 0.0f}, s1[PK_X] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                float e[PK_X];
                pk_emit(w[i], ar, (uint32_t)(mask >> (PK_X * i)) & 15u, th, omt, e);
#pragma unroll
                for (int x = 0; x < PK_X; ++x) {
                    const int a = (int)(w[i] << (24 - 8 * x)) >> 24;
                    const float g = ah[i][x] * b[i][x], t = e[x] * b[i][x];
                    b[i][x] = t;
                    sT[x] = sT[x] + t;
                    s0[x] = s0[x] + ((PK_ABLATE & 16) || a == 0 ? g : 0.0f);
                    s1[x] = s1[x] + ((PK_ABLATE & 16) || a == 1 ? g : 0.0f);
                }
            }
            float T = pk_lane4(sT), A0 = pk_lane4(s0), A1 = pk_lane4(s1);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                if (PK_ABLATE & 1) break;
                T = T + __shfl_xor(T, d, 64);
                A0 = A0 + __shfl_xor(A0, d, 64);
                A1 = A1 + __shfl_xor(A1, d, 64);
            }
            const float S = A0 + A1;
            const float q = A1 * (1.0f / S);
            const float ds = S >= FLT_MIN ? (q < 1.0f ? q : 1.0f) : nan;
            if (lane == (int)(j % IK_RUN)) keep = ds;
            // the sites j .. j + 63 below K: all walked.  (The ablation keeps the dose alive behind a condition that never holds.)
            if (j % IK_RUN == 0 && j + lane < K && (!(PK_ABLATE & 8) || theta > 2.0f)) out[j + lane] = keep;
            const float rj = j == 0 ? 1.0f : rho[j];
            const float ru = rj * u;
            const float kb = (1.0f - rj) * (1.0f / T);
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int x = 0; x < PK_X; ++x) b[i][x] = __builtin_fmaf(kb, b[i][x], ru);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- launcher
extern "C" int loc_impute_dose(const int8_t* h, int H, int64_t K, int64_t pitch, const uint8_t* donor, const int32_t* owner,
                               const int32_t* rec, int R, const float* rho, float theta, int block, float* dose, double* ll,
                               int32_t* n_donors, void* work, int64_t work_bytes, void* stream) {
    const pk_call c = {h, H, K, pitch, donor, owner, rec, R, rho, theta, block, ll, n_donors, work, work_bytes, (hipStream_t)stream};
    const pk_out outs[] = {{"dose", dose, 0}};
    pk_layout L;
    int rc;
    if (!pk_enter("loc_impute_dose", c, outs, 1, L, rc)) return rc;
    pk_dispatch(H, [&](auto nr) {
        hipLaunchKernelGGL(impute_kernel<decltype(nr)::value>, dim3((unsigned)R), dim3(64), 0, c.stream, h, H, K, pitch, donor, owner, rec,
                           rho, theta, L.B, dose, ll, n_donors, (float*)work, L.per_rec);
    });
    return pk_launched("ik_launch");                          // the name this message has carried since the first launcher
}
