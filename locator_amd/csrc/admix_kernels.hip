// The EM step of the admix command (locator_amd/admix.py): loc_admix_step, defined in include/locator_hip_admix.h; the NumPy
// form admix.step_host is what tests/test_gpu_admix.py holds it to.  Plain vector code, every operation fp32 and uncontracted.
//
// The step needs two reductions of the same (sample, site) terms a = g / h, b = r / hb: over the samples for F', over the
// sites for Q'.  Each gets a pass of its own that recomputes h and hb (4 C flops) instead of exchanging them:
// admix_f_kernel: a workgroup owns LOC_ADMIX_BLOCK = 64 sites, one a lane, F[k][:] and the sums A, B [C] in registers.  Its
//   LOC_ADMIX_SPLIT = 4 waves walk the samples w, w + 4, ...: a wave reads 64 consecutive bytes of a row of c, and the row of
//   Q is wave-uniform (scalar loads).  The four partial A, B meet in LDS in wave order; wave 0 finishes F' and the block's
//   share of ll, which no other workgroup touches.  ll: a lane keeps an fp32 run of LOC_ADMIX_LL_RUN / 2 samples (two terms
//   each) and continues in double; lanes by a butterfly, waves in order, all double.
// admix_q_kernel: a wave owns LOC_ADMIX_TILE = 64 samples, one a lane, and a group of site blocks; Q[i][:] and S [C] in
//   registers.  A lane reads its row 16 sites at a time (pt_load_piece: a row past N and a site past K read as missing, pad
//   bytes are never interpreted), the row of F is wave-uniform.  S and the integer n go to the group's slab of `work`.
// admix_finish_kernel: a thread per (sample, cluster) adds the element's slabs in group order and finishes Q'; its last
//   workgroup adds the blocks' ll.
// No tile of c is transposed: each pass reads the one layout along the axis it does not reduce over.
// Clusters are padded to CP = 4, 8 or 16 with Q = F = Fb = 0: a padded cluster adds +0 to h and hb.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_admix.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

constexpr int AD_T = LOC_ADMIX_TILE;
constexpr int AD_B = LOC_ADMIX_BLOCK;
constexpr int AD_W = LOC_ADMIX_SPLIT;
constexpr int AD_RUN = LOC_ADMIX_LL_RUN / 2;      // samples of a lane's fp32 run of ll: two terms each
constexpr float AD_EPS = 1e-5f;
static_assert(AD_T == 64 && AD_B == 64 && AD_B % 16 == 0, "one sample / one site a lane; a block is whole 16-byte pieces");

__device__ __forceinline__ int ad_byte(uint32_t w, int e) { return (int)(w << (24 - 8 * e)) >> 24; }

// (h, hb) = sum_c q (f, fb), clusters in ascending order, the two sums side by side as one packed multiply and one packed add a
// cluster (v_pk_mul_f32, v_pk_add_f32: two IEEE operations an instruction, the same bits as two scalar ones).  Both passes form
// them by these lines, so they hold the same bits.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int CP>
__device__ __forceinline__ f32x2 ad_mix(const float (&q)[CP], const f32x2 (&ff)[CP]) {
    f32x2 hh = {0.f, 0.f};
#pragma unroll
    for (int x = 0; x < CP; ++x) hh = hh + q[x] * ff[x];
    return hh;
}

// a = g / h and b = r / hb in the reciprocal form, exactly 0 for a missing call (cv < 0) whatever h and hb hold
__device__ __forceinline__ void ad_ratios(int cv, float fP, float h, float hb, float& g, float& r, float& a, float& b) {
    const bool on = cv >= 0;
    g = on ? (float)cv : 0.f;
    r = on ? fP - g : 0.f;
    a = on ? g * __builtin_amdgcn_rcpf(h) : 0.f;
    b = on ? r * __builtin_amdgcn_rcpf(hb) : 0.f;
}

template <int CP>
__global__ __launch_bounds__(64 * AD_W) void admix_f_kernel(const int8_t* __restrict__ c, int N, int64_t K, int64_t pitch, float fP,
                                                            int C, const float* __restrict__ Q, const float* __restrict__ F,
                                                            float* __restrict__ F_out, double* __restrict__ ll_part) {
    __shared__ float sA[AD_W][CP][64], sB[AD_W][CP][64];
    __shared__ double sl[AD_W];
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t k = (int64_t)blockIdx.x * AD_B + lane;
    const bool live = k < K;
    f32x2 ff[CP], AB[CP];                         // (F, Fb) of the site and its sums (A, B)
#pragma unroll
    for (int x = 0; x < CP; ++x) {
        const bool in = live && x < C;
        const float fv = in ? F[k * C + x] : 0.f;
        ff[x] = f32x2{fv, in ? 1.f - fv : 0.f};
        AB[x] = f32x2{0.f, 0.f};
    }
    double lld = 0.0;
    float llf = 0.f;
    int run = 0;
    for (int i = w; i < N; i += AD_W) {
        const int cv = live ? (int)c[(int64_t)i * pitch + k] : -1;       // a site past K reads as missing
        const float* const qi = Q + (int64_t)i * C;                      // wave-uniform
        float q[CP];
#pragma unroll
        for (int x = 0; x < CP; ++x) q[x] = x < C ? qi[x] : 0.f;
        float g, r, a, b;
        const f32x2 hh = ad_mix<CP>(q, ff);
        const float h = hh[0], hb = hh[1];
        ad_ratios(cv, fP, h, hb, g, r, a, b);
        const f32x2 ab = {a, b};
#pragma unroll
        for (int x = 0; x < CP; ++x) AB[x] = AB[x] + q[x] * ab;
        const float t1 = cv >= 0 ? g * logf(h) : 0.f, t2 = cv >= 0 ? r * logf(hb) : 0.f;
        llf = llf + t1;
        llf = llf + t2;
        if (++run == AD_RUN) {                                           // wave-uniform: every lane has walked the same samples
            lld += (double)llf;
            llf = 0.f;
            run = 0;
        }
    }
    lld += (double)llf;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lld = lld + __shfl_xor(lld, d, 64);
    if (lane == 0) sl[w] = lld;
#pragma unroll
    for (int x = 0; x < CP; ++x) {
        sA[w][x][lane] = AB[x][0];
        sB[w][x][lane] = AB[x][1];
    }
    __syncthreads();
    if (w != 0) return;
    if (lane == 0) {
        double s = sl[0];
#pragma unroll
        for (int v = 1; v < AD_W; ++v) s = s + sl[v];
        ll_part[blockIdx.x] = s;
    }
    if (!live) return;
    const float hi = 1.f - AD_EPS;
#pragma unroll
    for (int x = 0; x < CP; ++x) {
        if (x >= C) break;
        float sa = sA[0][x][lane], sb = sB[0][x][lane];
#pragma unroll
        for (int v = 1; v < AD_W; ++v) {
            sa = sa + sA[v][x][lane];
            sb = sb + sB[v][x][lane];
        }
        const float fa = ff[x][0] * sa, den = fa + ff[x][1] * sb;
        const float nf = den > 0.f ? fa / den : ff[x][0];                   // no called sample: the row stays
        F_out[k * C + x] = fminf(fmaxf(nf, AD_EPS), hi);
    }
}

// grid.x = the sample tiles, grid.y = the site groups; S slab [groups][N][CP] float, n slab [groups][N] int
template <int CP>
__global__ __launch_bounds__(AD_T) void admix_q_kernel(const int8_t* __restrict__ c, int N, int64_t K, int64_t pitch, float fP, int C,
                                                       const float* __restrict__ Q, const float* __restrict__ F,
                                                       int64_t blocks_per_group, float* __restrict__ s_slab, int* __restrict__ n_slab) {
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * AD_T + lane;
    const bool live = i < N;
    const int64_t nblocks = (K + AD_B - 1) / AD_B;
    const int64_t b0 = (int64_t)blockIdx.y * blocks_per_group, b1 = min(nblocks, b0 + blocks_per_group);
    const int64_t kend = min(K, b1 * AD_B);
    float q[CP], S[CP];
#pragma unroll
    for (int x = 0; x < CP; ++x) {
        q[x] = live && x < C ? Q[i * C + x] : 0.f;
        S[x] = 0.f;
    }
    int n = 0;
    for (int64_t k0 = b0 * AD_B; k0 < kend; k0 += 16) {
        const uint4 raw = pt_load_piece(c, i, N, k0, K, pitch);
        const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t k = k0 + e;
            if (k < kend) {                                              // wave-uniform: F past K is not read
                const int cv = ad_byte(wd[e >> 2], e & 3);
                const float* const fk = F + k * C;                       // wave-uniform
                f32x2 ff[CP];
#pragma unroll
                for (int x = 0; x < CP; ++x) {
                    const float fv = x < C ? fk[x] : 0.f;
                    ff[x] = f32x2{fv, x < C ? 1.f - fv : 0.f};
                }
                float g, r, a, b;
                const f32x2 hh = ad_mix<CP>(q, ff);
                ad_ratios(cv, fP, hh[0], hh[1], g, r, a, b);
                const f32x2 ab = {a, b};
#pragma unroll
                for (int x = 0; x < CP; ++x) {
                    const f32x2 p = ff[x] * ab;
                    S[x] = S[x] + (p[0] + p[1]);
                }
                n += cv >= 0 ? 1 : 0;
            }
        }
    }
    if (!live) return;
    const int64_t at = (int64_t)blockIdx.y * N + i;
#pragma unroll
    for (int x = 0; x < CP; x += 4) *reinterpret_cast<f32x4*>(s_slab + at * CP + x) = f32x4{S[x], S[x + 1], S[x + 2], S[x + 3]};
    n_slab[at] = n;
}

// A thread per (sample, cluster), 256 / CP samples a workgroup: the slabs of an element are read in group order, coalesced
// over the workgroup; the sum of a row is taken by every lane of the row's CP lanes from shuffles, clusters in ascending
// order.  The last workgroup adds the blocks' shares of ll instead: lane l of its first wave adds l, l + 64, ..., then a butterfly.
constexpr int AD_FIN_NT = 256;
template <int CP>
__global__ __launch_bounds__(AD_FIN_NT) void admix_finish_kernel(int N, int C, float fP, const float* __restrict__ Q,
                                                                 const float* __restrict__ s_slab, const int* __restrict__ n_slab,
                                                                 int groups, const double* __restrict__ ll_part, int64_t n_parts,
                                                                 float* __restrict__ Q_out, double* __restrict__ ll) {
    const int t = threadIdx.x, lane = t & 63;
    if (blockIdx.x == gridDim.x - 1) {
        if (t >= 64) return;
        double s = 0.0;
        for (int64_t p = lane; p < n_parts; p += 64) s = s + ll_part[p];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d, 64);
        if (lane == 0) *ll = s;
        return;
    }
    const int x = t & (CP - 1);
    const int64_t i = (int64_t)blockIdx.x * (AD_FIN_NT / CP) + t / CP;
    const bool live = i < N, mine = live && x < C;                  // no lane leaves: the row's lanes meet in the shuffles
    float S = 0.f;
    int64_t n = 0;
    if (live)
#pragma unroll 8                                  // eight slabs' loads in flight; the adds keep the group order
        for (int z = 0; z < groups; ++z) {
            const int64_t at = (int64_t)z * N + i;
            S = S + s_slab[at * CP + x];
            n += n_slab[at];
        }
    const float den = fP * (float)n;
    const float qv = mine ? Q[i * C + x] : 0.f;
    const float out = mine ? fmaxf(n > 0 ? qv * S / den : qv, AD_EPS) : 0.f;       // no called site: the row stays
    float sum = 0.f;
#pragma unroll
    for (int y = 0; y < CP; ++y) {
        const float v = __shfl(out, (lane & ~(CP - 1)) + y, 64);
        if (y < C) sum = sum + v;
    }
    if (mine) Q_out[i * C + x] = out / sum;
}

// ---------------------------------------------------------------------------------------------------------------- launcher
static bool ad_sizes_ok(const char* who, int N, int64_t K, int C, int k_groups) {
    if (N < 0 || K < 0 || N >= (1 << 20) || K >= ((int64_t)1 << 31) || C < 2 || C > LOC_ADMIX_MAX_POPS || k_groups < 0) {
        loc_set_error("%s: N=%d K=%lld C=%d k_groups=%d (none may be negative; N below 2^20, K below 2^31, C 2 .. %d)", who, N,
                      (long long)K, C, k_groups, LOC_ADMIX_MAX_POPS);
        return false;
    }
    return true;
}

static int ad_padded(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : 16; }
static int64_t ad_up16(int64_t v) { return (v + 15) / 16 * 16; }

// The site groups of the Q-pass.  A workgroup is one wave and keeps few registers, so a compute unit holds many: the groups
// are chosen to fill 16 waves a compute unit (pt_site_groups counts 2 slots a unit; measured at 1,000 x 100,000 x 8: 8 waves a
// unit left the vector units waiting, 0.40 ms against 0.33 ms of the F-pass for the same arithmetic), and a group keeps at least
// 4 blocks = 256 sites, so that its slab row (C floats a sample) stays a small share of what it reads.
static pt_groups ad_split(int N, int64_t K, int k_groups) {
    return pt_site_groups((K + AD_B - 1) / AD_B, ((int64_t)N + AD_T - 1) / AD_T, k_groups, 8 * sr_compute_units(), 4, 4);
}

struct ad_layout { int64_t parts, groups, per, s_at, n_at, bytes; };
static ad_layout ad_work(int N, int64_t K, int C, int k_groups) {
    ad_layout L = {0, 0, 0, 0, 0, 0};
    if (N == 0 || K == 0) return L;
    const pt_groups split = ad_split(N, K, k_groups);
    L.parts = (K + AD_B - 1) / AD_B;
    L.groups = split.groups;
    L.per = split.per;
    L.s_at = ad_up16(L.parts * (int64_t)sizeof(double));
    L.n_at = L.s_at + L.groups * N * ad_padded(C) * (int64_t)sizeof(float);
    L.bytes = ad_up16(L.n_at + L.groups * N * (int64_t)sizeof(int));
    return L;
}

extern "C" int64_t loc_admix_work_bytes(int N, int64_t K, int C, int k_groups) {
    if (!ad_sizes_ok("loc_admix_work_bytes", N, K, C, k_groups)) return -1;
    return ad_work(N, K, C, k_groups).bytes;
}

static bool ad_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return na > 0 && nb > 0 && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

template <int CP>
static int ad_launch(const int8_t* c, int N, int64_t K, int64_t pitch, int P, int C, const float* Q, const float* F, float* Q_out,
                     float* F_out, double* ll, const ad_layout& L, char* work, hipStream_t stream) {
    double* const ll_part = (double*)work;
    float* const s_slab = (float*)(work + L.s_at);
    int* const n_slab = (int*)(work + L.n_at);
    const unsigned tiles = (unsigned)(((int64_t)N + AD_T - 1) / AD_T);
    hipLaunchKernelGGL(admix_f_kernel<CP>, dim3((unsigned)L.parts), dim3(64 * AD_W), 0, stream, c, N, K, pitch, (float)P, C, Q, F, F_out,
                       ll_part);
    LOC_CHECK_LAUNCH();
    hipLaunchKernelGGL(admix_q_kernel<CP>, dim3(tiles, (unsigned)L.groups), dim3(AD_T), 0, stream, c, N, K, pitch, (float)P, C, Q, F,
                       L.per, s_slab, n_slab);
    LOC_CHECK_LAUNCH();
    const unsigned rows = (unsigned)(((int64_t)N + AD_FIN_NT / CP - 1) / (AD_FIN_NT / CP));
    hipLaunchKernelGGL(admix_finish_kernel<CP>, dim3(rows + 1), dim3(AD_FIN_NT), 0, stream, N, C, (float)P, Q, (const float*)s_slab,
                       (const int*)n_slab, (int)L.groups, (const double*)ll_part, L.parts, Q_out, ll);
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_admix_step(const int8_t* c, int N, int64_t K, int64_t pitch, int P, int C, const float* Q, const float* F,
                              float* Q_out, float* F_out, double* ll, int k_groups, void* work, int64_t work_bytes, void* stream) {
    if (!ad_sizes_ok("loc_admix_step", N, K, C, k_groups) || !pt_sizes_ok("loc_admix_step", N, K, pitch, k_groups, work_bytes)) return -1;
    if (P < 1 || P > 2) {
        loc_set_error("loc_admix_step: P=%d (must be 1 or 2)", P);
        return -1;
    }
    const int64_t qb = (int64_t)N * C * sizeof(float), fb = K * C * (int64_t)sizeof(float);
    if (!ll || (N > 0 && (!Q || !Q_out)) || (K > 0 && (!F || !F_out)) || (N > 0 && K > 0 && !c)) {
        loc_set_error("loc_admix_step: null buffer");
        return -1;
    }
    if ((uintptr_t)Q % 16 != 0 || (uintptr_t)F % 16 != 0 || (uintptr_t)Q_out % 16 != 0 || (uintptr_t)F_out % 16 != 0 ||
        (uintptr_t)ll % 8 != 0) {
        loc_set_error("loc_admix_step: Q, F, Q_out and F_out must be multiples of 16 bytes, ll of 8");
        return -1;
    }
    if (ad_overlap(Q_out, qb, Q, qb) || ad_overlap(Q_out, qb, F, fb) || ad_overlap(F_out, fb, Q, qb) || ad_overlap(F_out, fb, F, fb) ||
        ad_overlap(Q_out, qb, F_out, fb) || ad_overlap(ll, 8, Q_out, qb) || ad_overlap(ll, 8, F_out, fb)) {
        loc_set_error("loc_admix_step: Q_out, F_out and ll may overlap neither an input nor each other");
        return -1;
    }
    if (N > 0 && K > 0 && !pt_rows_aligned("loc_admix_step", c, pitch)) return -1;
    const ad_layout L = ad_work(N, K, C, k_groups);
    if (!pt_work_ok("loc_admix_step", "loc_admix_work_bytes", work, work_bytes, L.bytes)) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0 || K == 0) {                       // no call: no row moves and the likelihood is that of nothing
        hipError_t e = hipMemsetAsync(ll, 0, sizeof(double), s);
        if (e == hipSuccess && N > 0) e = hipMemcpyAsync(Q_out, Q, (size_t)qb, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && K > 0) e = hipMemcpyAsync(F_out, F, (size_t)fb, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) {
            loc_set_error("loc_admix_step: %s", hipGetErrorString(e));
            return (int)e;
        }
        return 0;
    }
    switch (ad_padded(C)) {
        case 4: return ad_launch<4>(c, N, K, pitch, P, C, Q, F, Q_out, F_out, ll, L, (char*)work, s);
        case 8: return ad_launch<8>(c, N, K, pitch, P, C, Q, F, Q_out, F_out, ll, L, (char*)work, s);
        default: return ad_launch<16>(c, N, K, pitch, P, C, Q, F, Q_out, F_out, ll, L, (char*)work, s);
    }
}
