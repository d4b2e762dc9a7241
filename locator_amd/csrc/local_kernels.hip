// The window sums of the ancestry command (locator_amd/ancestry.py): loc_paint_local, defined in include/locator_hip_local.h;
// the NumPy form ancestry.local_host is what tests/test_gpu_ancestry.py holds it to.  The copying model is paint_kernels.hip's, by
// the same pk_* functions (paint_core.h): one wave a recipient, the state in registers, the forward pass with checkpoints (ll),
// then block by block from the last the recomputation of a-hat into scratch and the backward walk with its prefetch of the
// previous row.  The walk forms paint's gamma = g (1 / G) by paint's operations and no chunks: it holds a-hat, b, the prefetched
// row and one accumulator a column, S, the sum of gamma over the sites of the current window.
// Windows: the walk descends over all sites K - 1 .. 0 across the blocks and the windows are ascending and disjoint, so it meets
// them from the last to the first; [v0, v1) of the current one ride in scalars.  A site outside it adds nowhere.  On arrival at
// v0 the wave contracts S with the C attribute rows: a lane reads its four columns of a sweep of row c as one float4 (row c + 1
// is requested before row c is reduced), p = fma(S, v, p) over its donor columns, the butterfly, and lane c keeps channel c; then
// one store instruction writes the window's C values, S is cleared and the window before it becomes the current one.
#include "paint_core.h"

#include "../../include/locator_hip_local.h"

constexpr int LK_C = LOC_LOCAL_MAX_CHANNELS;
static_assert(LK_C == 64, "a channel a lane");

// the lane's columns of the attribute row `row`: columns at or past vpitch read as 0 (they are no donors: never multiplied)
template <int NR>
__device__ __forceinline__ void lk_load_attr(const float* __restrict__ row, int64_t vpitch, int lane, float (&a)[NR][PK_X]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int64_t col = PK_X * lane + PK_SWEEP * i;       // vpitch is a multiple of 4: a float4 that starts inside ends inside
        const float4 q = col < vpitch ? *reinterpret_cast<const float4*>(row + col) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        a[i][0] = q.x; a[i][1] = q.y; a[i][2] = q.z; a[i][3] = q.w;
    }
}

template <int NR>
__global__ __launch_bounds__(64) void local_kernel(const int8_t* __restrict__ h, int H, int64_t K, int64_t pitch,
                                                   const uint8_t* __restrict__ donor, const int32_t* __restrict__ owner,
                                                   const int32_t* __restrict__ rec, const float* __restrict__ rho, float theta, int64_t B,
                                                   const float* __restrict__ v, int C, int64_t vpitch, const int32_t* __restrict__ win,
                                                   int W, float* __restrict__ out, double* __restrict__ ll,
                                                   int32_t* __restrict__ n_donors, float* __restrict__ work, int64_t per_rec) {
    constexpr int64_t HP = (int64_t)PK_SWEEP * NR, STRIDE = HP + PK_CS;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const int rc = rec[r];
    if (rc < 0 || rc >= H) return;                          // the launcher has refused it
    int D;
    const uint64_t mask = pk_donor_mask<NR>(donor, owner, H, owner[rc], lane, D);
    float* const o = out + r * (int64_t)W * C;
    if (lane == 0) n_donors[r] = D;
    if (D == 0) {
        for (int64_t e = lane; e < (int64_t)W * C; e += 64) o[e] = 0.0f;
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

    float b[NR][PK_X], S[NR][PK_X], nx[NR][PK_X];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int x = 0; x < PK_X; ++x) {
            b[i][x] = u;
            S[i][x] = 0.0f;
        }
    int wi = W - 1;                                           // the current window: the last one that the walk has not left
    int64_t v0 = win[2 * wi], v1 = win[2 * wi + 1];
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
            const float kb = (1.0f - rj) * (1.0f / T);
            const bool inside = wi >= 0 && j >= v0 && j < v1;
            // second sweep: the posterior into the window's sum, and b_(j-1)
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int x = 0; x < PK_X; ++x) {
                    if (inside) S[i][x] = S[i][x] + ah[i][x] * invG;
                    b[i][x] = __builtin_fmaf(kb, b[i][x], ru);
                }
            if (!inside || j != v0) continue;

            // the window's end: out[w][c] = sum_d S(d) v[c][d] over the donors, channel c kept by lane c; a-hat's registers are
            // free until the next site takes the prefetched row
            // (The ablation keeps S and gamma alive behind a condition that never holds.)
            float keep = 0.0f;
            if (!(PK_ABLATE & 32) || theta > 2.0f) {
                float a[NR][PK_X], an[NR][PK_X];
                lk_load_attr<NR>(v, vpitch, lane, an);
                for (int c = 0; c < C; ++c) {
#pragma unroll
                    for (int i = 0; i < NR; ++i)
#pragma unroll
                        for (int x = 0; x < PK_X; ++x) a[i][x] = an[i][x];
                    lk_load_attr<NR>(v + (int64_t)(c + 1 < C ? c + 1 : c) * vpitch, vpitch, lane, an);
                    float p = 0.0f;
#pragma unroll
                    for (int i = 0; i < NR; ++i)
#pragma unroll
                        for (int x = 0; x < PK_X; ++x)
                            if ((mask >> (PK_X * i + x)) & 1u) p = __builtin_fmaf(S[i][x], a[i][x], p);
                    p = pk_wave_sum(p);
                    if (lane == c) keep = p;
                }
            }
            if (lane < C) o[(int64_t)wi * C + lane] = keep;
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int x = 0; x < PK_X; ++x) S[i][x] = 0.0f;
            --wi;
            if (wi >= 0) {
                v0 = win[2 * wi];
                v1 = win[2 * wi + 1];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- launcher
extern "C" int loc_paint_local(const int8_t* h, int H, int64_t K, int64_t pitch, const uint8_t* donor, const int32_t* owner,
                               const int32_t* rec, int R, const float* rho, float theta, int block, const float* v, int C,
                               int64_t vpitch, const int32_t* win, int W, float* out, double* ll, int32_t* n_donors, void* work,
                               int64_t work_bytes, void* stream) {
    const char* who = "loc_paint_local";
    const pk_call c = {h, H, K, pitch, donor, owner, rec, R, rho, theta, block, ll, n_donors, work, work_bytes, (hipStream_t)stream};
    if (!pk_args_ok(who, H, K, R, block, pitch, work_bytes, theta)) return -1;
    if (K == 0) {
        loc_set_error("%s: K=0 admits no window", who);
        return -1;
    }
    if (C < 1 || C > LK_C || W < 1 || W > K) {
        loc_set_error("%s: C=%d W=%d (C 1 .. %d: a channel a lane; W 1 .. K = %lld: the windows are disjoint and not empty)", who, C, W,
                      LK_C, (long long)K);
        return -1;
    }
    if (vpitch < H || vpitch % 4 != 0) {
        loc_set_error("%s: vpitch=%lld (vpitch >= H = %d and a multiple of 4)", who, (long long)vpitch, H);
        return -1;
    }
    if (R == 0) return 0;
    if (!v || !win) {
        loc_set_error("%s: null buffer", who);
        return -1;
    }
    if ((uintptr_t)v % 16 != 0 || (uintptr_t)win % 4 != 0) {
        loc_set_error("%s: v must be a multiple of 16 bytes (a row is read 16 bytes at a time), win of 4", who);
        return -1;
    }
    std::vector<int32_t> h_win((size_t)W * 2);
    const pk_also also = {win, h_win.data(), h_win.size() * sizeof(int32_t)};
    const pk_out outs[] = {{"out", out, 0}};
    pk_layout L;
    int rc;
    if (!pk_enter(who, c, outs, 1, L, rc, &also)) return rc;
    for (int w = 0; w < W; ++w) {
        const int64_t a = h_win[(size_t)2 * w], b = h_win[(size_t)2 * w + 1];
        if (a < 0 || a >= b || b > K || (w > 0 && a < h_win[(size_t)2 * w - 1])) {
            loc_set_error("%s: win[%d] = [%lld, %lld) is no window (0 <= v0 < v1 <= K = %lld, ascending and disjoint)", who, w,
                          (long long)a, (long long)b, (long long)K);
            return -1;
        }
    }
    pk_dispatch(H, [&](auto nr) {
        hipLaunchKernelGGL(local_kernel<decltype(nr)::value>, dim3((unsigned)R), dim3(64), 0, c.stream, h, H, K, pitch, donor, owner, rec,
                           rho, theta, L.B, v, C, vpitch, win, W, out, ll, n_donors, (float*)work, L.per_rec);
    });
    return pk_launched("lk_launch");
}
