// Per-SNP attribution of a kept model (python -m locator_amd.explain; DESIGN.md §8, the explain command).  Three entry points after the
// exact layer-1 forward (loc_l1_forward_rows / loc_l1_forward):
//   loc_explain_stack_grad   hidden-stack forward keeping every layer's activations, then the backward pass with the two seeds
//                            of the map-unit outputs: delta1[(n, j)][h] = d(xhat, yhat)_j / d(layer-1 pre-activation)_h.
//                            Plain fp32 64 x 64 tiles on the vector ALU (its FLOPs are a few % of the next step's).
//   loc_explain_sites        D[(n, j)][s] = sum_h delta1[(n, j)][h] U[s][h] on v_mfma_f32_32x32x2_f32, U = the folded first
//                            layer (s_c W1[c][h] summed over the columns of site s), with the per-site epilogue
//                            A = D (x_ns - mov_mean_s) and the four per-site sums of the workgroup's rows -> partial[split][4][Ks].
//   loc_explain_reduce       the splits added in a fixed order (no atomics: bit-identical from run to run) -> means.
// Rows 2n and 2n + 1 of D are sample n's x and y: in the 32 x 32 C/D map (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
// registers 2p and 2p + 1 of a lane then hold D_x and D_y of one sample at one site, so sqrt(A_x^2 + A_y^2) needs no lane
// movement.  Offsets are 64-bit wherever n * pitch or Ks * Hp can pass 2^31.
#include "common.h"

#define EX_MT 128    /* rows of D (64 samples x {x, y}) per M tile                                                   */
#define EX_NT 128    /* sites per workgroup                                                                         */
#define EX_KC 32     /* h per LDS chunk                                                                              */
#define EX_PITCH 36  /* floats per LDS row: ds_read_b128 of 16 consecutive rows start in 16 distinct 4-bank slots  */
#define EX_LDS_FLOATS ((EX_MT + EX_NT) * EX_PITCH)
static_assert(EX_LDS_FLOATS * 4 <= 160 * 1024, "explain_sites LDS exceeds gfx950's 160 KB");
static_assert(4 * 2 * 4 * 64 * 8 <= EX_LDS_FLOATS * 4, "the final cross-wave reduction reuses the operand LDS");

// ------------------------------------------------------------------ hidden stack: forward + backward (fp32 vector ALU)
#define DT 64        /* output tile rows / columns */
#define DK 16        /* k per LDS chunk           */

// MODE 0 (forward):  C[r][c] = ELU(sum_k A[r][k] W[k][c] + bias[c])                 (A = activations [M][Hp])
// MODE 1 (backward): C[r][c] = (sum_k A[r][k] W[c][k]) * elu'(act[r >> 1][c])        (A = gradients [2n][Hp])
template <int MODE>
__global__ __launch_bounds__(256) void ex_dense_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                       const float* __restrict__ bias, const float* __restrict__ act,
                                                       float* __restrict__ C, int M, int Hp) {
    __shared__ float As[DK][DT + 4];
    __shared__ float Bs[DK][DT + 4];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * DT;      // rows on x: 2n / 64 tiles can pass grid.y's 65535
    const int c0 = blockIdx.y * DT;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < Hp; k0 += DK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + 256 * i;
            const int r = idx >> 4, kk = idx & 15;
            As[kk][r] = r0 + r < M ? A[(r0 + r) * Hp + k0 + kk] : 0.f;
            if (MODE == 0) {
                const int kb = idx >> 6, c = idx & 63;
                Bs[kb][c] = c0 + c < Hp ? W[(int64_t)(k0 + kb) * Hp + c0 + c] : 0.f;
            } else {
                const int c = idx >> 4;
                Bs[kk][c] = c0 + c < Hp ? W[(int64_t)(c0 + c) * Hp + k0 + kk] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty * 4 + i]; b[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + ty * 4 + i;
        if (r >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx * 4 + j;
            if (c >= Hp) continue;
            C[r * Hp + c] = MODE == 0 ? elu_f(acc[i][j] + bias[c])
                                      : acc[i][j] * elu_grad_from_act(act[(r >> 1) * Hp + c]);
        }
    }
}

// G[(n, j)][h] = sd_j (Wa Wb[:, j])[h] * elu'(aL[n][h]): the constant head Dense(2) . Dense(2) in map units, into the last layer
__global__ __launch_bounds__(256) void ex_seed_kernel(const float* __restrict__ aL, const float* __restrict__ wa,
                                                      const float* __restrict__ wb, float sd_x, float sd_y,
                                                      float* __restrict__ G, int n, int Hp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * (int64_t)n * Hp) return;
    const int64_t r = i / Hp;
    const int h = (int)(i - r * Hp), j = (int)(r & 1);
    const float c = (j ? sd_y : sd_x) * (wa[2 * h] * wb[j] + wa[2 * h + 1] * wb[2 + j]);
    G[i] = c * elu_grad_from_act(aL[(r >> 1) * Hp + h]);
}

extern "C" int loc_explain_stack_grad(const float* a1, int n, int Hp, int L, const float* wh, const float* bh,
                                      const float* wa, const float* wb, float sd_x, float sd_y, float* acts, float* g,
                                      float* delta1, void* stream) {
    if (n < 1 || n > (1 << 29) || Hp < 32 || Hp > LOC_MAX_WIDTH || Hp % 32 || L < 1) {
        loc_set_error("loc_explain_stack_grad: n=%d Hp=%d L=%d (need 1 <= n <= 2^29, 32 <= Hp <= %d, Hp %% 32 == 0, L >= 1)",
                      n, Hp, L, LOC_MAX_WIDTH);
        return -1;
    }
    if (L >= 2 && (!acts || !g)) { loc_set_error("loc_explain_stack_grad: nlayers %d needs acts and g scratch", L); return -1; }
    const int64_t nH = (int64_t)n * Hp, HH = (int64_t)Hp * Hp;
    auto act = [&](int l) { return l == 1 ? a1 : acts + (int64_t)(l - 2) * nH; };
    const unsigned ct = (Hp + DT - 1) / DT;
    for (int l = 2; l <= L; ++l) {
        hipLaunchKernelGGL(ex_dense_kernel<0>, dim3((n + DT - 1) / DT, ct), dim3(256), 0, (hipStream_t)stream,
                           act(l - 1), wh + (l - 2) * HH, bh + (int64_t)(l - 2) * Hp, nullptr, acts + (int64_t)(l - 2) * nH,
                           n, Hp);
        LOC_CHECK_LAUNCH();
    }
    // L - 1 backward launches ping-pong between g and delta1 so that the last one writes delta1
    float* cur = (L - 1) % 2 == 0 ? delta1 : g;
    const int64_t total = 2 * nH;
    hipLaunchKernelGGL(ex_seed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, act(L), wa,
                       wb, sd_x, sd_y, cur, n, Hp);
    LOC_CHECK_LAUNCH();
    for (int l = L; l >= 2; --l) {
        float* next = cur == delta1 ? g : delta1;
        hipLaunchKernelGGL(ex_dense_kernel<1>, dim3((2 * n + DT - 1) / DT, ct), dim3(256), 0, (hipStream_t)stream,
                           cur, wh + (l - 2) * HH, nullptr, act(l - 1), next, 2 * n, Hp);
        LOC_CHECK_LAUNCH();
        cur = next;
    }
    return 0;
}

// ------------------------------------------------------------------ the site contraction (matrix pipe) + epilogue
// Workgroup = 4 waves over a 128-row x 128-site tile, wave w: rows 64 (w & 1) .., sites 64 (w >> 1) .., 2 x 2 accumulators of
// 32 x 32.  K order inside a 32-chunk: MFMA step s of lane half q contracts h = 16 q + s, for A and B alike, so each lane's 16
// operands of a chunk are 4 consecutive float4 of its LDS row.  The workgroup walks M tiles mt0 .. mt1 of its split and keeps
// its lanes' per-site sums in fp64 registers; one fixed-order cross-lane / cross-wave sum through the LDS at the end.
__global__ __launch_bounds__(256) void ex_sites_kernel(const float* __restrict__ delta1, int n, const float* __restrict__ U,
                                                       int Ks, int Hp, const uint8_t* __restrict__ Xs, int64_t xs_pitch,
                                                       const float* __restrict__ mov_mean, int mt_per_split,
                                                       double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float lds[EX_LDS_FLOATS];
    float* As = lds;
    float* Bs = lds + EX_MT * EX_PITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1, col = lane & 31, q = lane >> 5;
    const int64_t site0 = (int64_t)blockIdx.x * EX_NT;
    const int64_t M = 2 * (int64_t)n;
    const int mt_total = (int)((M + EX_MT - 1) / EX_MT);
    const int mt0 = blockIdx.y * mt_per_split;
    const int mt1 = mt0 + mt_per_split < mt_total ? mt0 + mt_per_split : mt_total;
    double st[2][4] = {};
    float mm[2];
    bool site_ok[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int64_t s = site0 + wn * 64 + ni * 32 + col;
        site_ok[ni] = s < Ks;
        mm[ni] = site_ok[ni] ? mov_mean[s] : 0.f;
    }
    for (int mt = mt0; mt < mt1; ++mt) {
        const int64_t row0 = (int64_t)mt * EX_MT;
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
        for (int h0 = 0; h0 < Hp; h0 += EX_KC) {
            f32x4 ra[4], rb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = t + 256 * i, r = idx >> 3, c4 = idx & 7;
                ra[i] = row0 + r < M ? *(const f32x4*)(delta1 + (row0 + r) * Hp + h0 + 4 * c4) : f32x4{};
                rb[i] = site0 + r < Ks ? *(const f32x4*)(U + (site0 + r) * Hp + h0 + 4 * c4) : f32x4{};
            }
            __syncthreads();                       // the previous chunk's LDS reads are done
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = t + 256 * i, r = idx >> 3, c4 = idx & 7;
                *(f32x4*)(As + r * EX_PITCH + 4 * c4) = ra[i];
                *(f32x4*)(Bs + r * EX_PITCH + 4 * c4) = rb[i];
            }
            __syncthreads();
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                f32x4 a[2], b[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    a[mi] = *(const f32x4*)(As + (wm * 64 + mi * 32 + col) * EX_PITCH + 16 * q + 4 * i4);
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    b[ni] = *(const f32x4*)(Bs + (wn * 64 + ni * 32 + col) * EX_PITCH + 16 * q + 4 * i4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma32(a[mi][e], b[ni][e], acc[mi][ni]);
            }
        }
        // epilogue: register pair (4 g + 2 p, 4 g + 2 p + 1) = rows 8 g + 4 q + 2 p (+1) = D_x, D_y of one sample
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if (!site_ok[ni]) continue;
            const int64_t s = site0 + wn * 64 + ni * 32 + col;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        const int64_t smp = (row0 + wm * 64 + mi * 32 + 8 * g + 4 * q + 2 * p) >> 1;
                        if (smp >= n) continue;
                        const float jx = acc[mi][ni][4 * g + 2 * p], jy = acc[mi][ni][4 * g + 2 * p + 1];
                        const float dx = (float)Xs[smp * xs_pitch + s] - mm[ni];
                        const float ax = jx * dx, ay = jy * dx;
                        st[ni][0] += (double)fabsf(ax);
                        st[ni][1] += (double)fabsf(ay);
                        st[ni][2] += (double)sqrtf(ax * ax + ay * ay);
                        st[ni][3] += (double)(jx * jx + jy * jy);
                    }
        }
    }
    // fixed-order sum over the two lane halves and the two row waves of each site
    __syncthreads();
    double* red = (double*)lds;                    // [wave][ni][stat][lane]
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[((wave * 2 + ni) * 4 + k) * 64 + lane] = st[ni][k];
    __syncthreads();
    if (t < EX_NT) {
        const int tn = t >> 6, tni = (t >> 5) & 1, tc = t & 31;
        const int64_t s = site0 + t;
        if (s < Ks) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double v = 0.0;
                for (int twm = 0; twm < 2; ++twm)
                    for (int tq = 0; tq < 2; ++tq) v += red[(((twm + 2 * tn) * 2 + tni) * 4 + k) * 64 + tc + 32 * tq];
                partial[((int64_t)blockIdx.y * 4 + k) * Ks + s] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void ex_reduce_kernel(const double* __restrict__ partial, int splits, int Ks, int n,
                                                        double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= Ks) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = 0.0;
        for (int sp = 0; sp < splits; ++sp) v += partial[((int64_t)sp * 4 + k) * Ks + s];
        v /= (double)n;
        out[(int64_t)k * Ks + s] = k == 3 ? sqrt(v) : v;
    }
}

extern "C" int loc_explain_splits(int n, int Ks, int compute_units) {
    if (n < 1 || Ks < 1) return 1;
    const int64_t mt = (2 * (int64_t)n + EX_MT - 1) / EX_MT, nt = ((int64_t)Ks + EX_NT - 1) / EX_NT;
    const int64_t want = 4 * (int64_t)(compute_units > 0 ? compute_units : 256);   // workgroups to fill the device
    int64_t s = (want + nt - 1) / nt;
    if (s > mt) s = mt;
    if (s < 1) s = 1;
    // every split gets at least one M tile: ceil(mt / ceil(mt / s)) splits
    const int64_t per = (mt + s - 1) / s;
    return (int)((mt + per - 1) / per);
}

extern "C" int loc_explain_sites(const float* delta1, int n, const float* U, int Ks, int Hp, const uint8_t* Xs,
                                 int64_t xs_pitch, const float* mov_mean, int splits, double* partial, void* stream) {
    if (n < 1 || n > (1 << 29) || Ks < 1 || Hp < 32 || Hp > LOC_MAX_WIDTH || Hp % 32 || xs_pitch < Ks) {
        loc_set_error("loc_explain_sites: n=%d Ks=%d Hp=%d xs_pitch=%lld (need 1 <= n <= 2^29, Ks >= 1, 32 <= Hp <= %d, "
                      "Hp %% 32 == 0, xs_pitch >= Ks)", n, Ks, Hp, (long long)xs_pitch, LOC_MAX_WIDTH);
        return -1;
    }
    const int mt = (int)((2 * (int64_t)n + EX_MT - 1) / EX_MT);
    if (splits < 1 || splits > mt || splits > 65535) { loc_set_error("loc_explain_sites: splits=%d out of 1..%d", splits, mt); return -1; }
    const int per = (mt + splits - 1) / splits;
    if ((int64_t)per * (splits - 1) >= mt) {
        loc_set_error("loc_explain_sites: splits=%d leaves a split without rows (use loc_explain_splits)", splits);
        return -1;
    }
    const int nt = (int)(((int64_t)Ks + EX_NT - 1) / EX_NT);
    hipLaunchKernelGGL(ex_sites_kernel, dim3(nt, splits), dim3(256), 0, (hipStream_t)stream, delta1, n, U, Ks, Hp, Xs,
                       xs_pitch, mov_mean, per, partial);
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_explain_reduce(const double* partial, int splits, int Ks, int n, double* out, void* stream) {
    if (splits < 1 || Ks < 1 || n < 1) {
        loc_set_error("loc_explain_reduce: splits=%d Ks=%d n=%d", splits, Ks, n);
        return -1;
    }
    hipLaunchKernelGGL(ex_reduce_kernel, dim3((unsigned)(((int64_t)Ks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       partial, splits, Ks, n, out);
    LOC_CHECK_LAUNCH();
    return 0;
}
